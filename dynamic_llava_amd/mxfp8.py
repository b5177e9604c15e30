"""MXFP8 decoder weights: the host reference of the format (pure torch, CPU or device).

OCP Microscaling v1.0 MXFP8 laid out along K: every 32 consecutive K elements of one output row share one E8M0 scale 2^e, the elements are FP8 E4M3 in
the OCP ``e4m3fn`` encoding (not the ``fnuz`` one).  Storage: ``q`` uint8 [N, K] (the e4m3fn codes) and ``scale`` uint8 [N, K/32] (the E8M0 code e + 127).

The rule, per block of 32:
  1. amax = max|w|; amax == 0 -> e = 0 and every q = 0;
  2. otherwise e = floor(log2(amax)) - 8 (8 = the e4m3 emax);
  3. e is clamped to [e_min(dtype), 127]: -15 for fp16, -124 for bf16 / fp32.  Every q * 2^e is then exactly representable in the model dtype, the e4m3
     subnormals included;
  4. q = RNE(w / 2^e) to e4m3fn, saturated at +-448 (torch's own float8_e4m3fn cast is not used: it turns values above 448 into NaN);
  5. a NaN or Inf weight is an error.

W' = dequantize_mx8(q, scale, dtype) is exact in ``dtype``, so a model whose weights are replaced by W' is an ordinary model of that dtype: the format has an
exact definition to test against.  Quantisation is idempotent (quantize(W') reproduces (q, scale)) but not reversible (W' != W in general).

dl_quantize_mx8 (csrc/gemv_mx8.hip) is bit-exact to quantize_mx8 for f32, bf16 and f16 sources.
"""
from __future__ import annotations

import torch

BLOCK = 32
E4M3_MAX = 448.0


def e_min(dtype: torch.dtype) -> int:
    """Smallest block exponent for a model of `dtype` (include/dynllava.h dl_mx8_e_min)."""
    if dtype == torch.float16:
        return -15
    if dtype in (torch.bfloat16, torch.float32):
        return -124
    raise ValueError(f"MXFP8: unsupported model dtype {dtype}")


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for integer e in [-126, 127] (built from the exponent bits: exact)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _floor_log2(a: torch.Tensor) -> torch.Tensor:
    """floor(log2(a)) of positive finite fp32 values, fp32 subnormals included."""
    _, ex = torch.frexp(a)  # a = m 2^ex, m in [0.5, 1)
    return ex.to(torch.int32) - 1


def _e4m3_codes(s: torch.Tensor) -> torch.Tensor:
    """RNE of fp32 values s (|s| < 512) to e4m3fn codes, saturated at +-448."""
    a = s.abs()
    ea = torch.where(a > 0, _floor_log2(torch.where(a > 0, a, torch.ones_like(a))), torch.full_like(a, -127, dtype=torch.int32))
    qe = torch.where(ea >= -6, ea - 3, torch.full_like(ea, -9))  # the quantum of a: 2^(floor(log2 a) - 3) in the normal range, 2^-9 below
    quantum = _pow2(qe)
    r = torch.round(a / quantum) * quantum  # torch.round: half to even; a / quantum is exact
    r = torch.clamp(r, max=E4M3_MAX)
    rb = r.view(torch.int32)
    er = (rb >> 23) - 127
    normal = ((er + 7) << 3) | ((rb >> 20) & 7)
    sub = (r * 512.0).to(torch.int32)  # subnormals: multiples of 2^-9
    mag = torch.where(r == 0, torch.zeros_like(rb), torch.where(er >= -6, normal, sub))
    sign = torch.signbit(s).to(torch.int32) << 7
    return (sign | mag).to(torch.uint8)


def _e4m3_values(q: torch.Tensor) -> torch.Tensor:
    """e4m3fn codes -> fp32 values (0x7f / 0xff, the NaN codes, are never written by the quantiser)."""
    c = q.to(torch.int32)
    E = (c >> 3) & 15
    m = (c & 7).to(torch.float32)
    mag = torch.where(E == 0, m * 2.0**-9, (8.0 + m) * _pow2(E - 10))
    return torch.where((c & 0x80) != 0, -mag, mag)


@torch.no_grad()
def quantize_mx8(w: torch.Tensor, dtype: torch.dtype | None = None):
    """w [N, K] (f32 / bf16 / f16; K % 32 == 0) -> (q uint8 [N, K], scale uint8 [N, K/32]).  `dtype`: the model dtype whose e_min applies (default w.dtype).
    Raises ValueError on NaN / Inf.  Runs where w lives."""
    if w.dim() != 2 or w.shape[1] % BLOCK != 0:
        raise ValueError(f"quantize_mx8: need a [N, K] weight with K % {BLOCK} == 0, got {tuple(w.shape)}")
    dtype = w.dtype if dtype is None else dtype
    lo = e_min(dtype)
    wf = w.to(torch.float32)
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_mx8: the weight holds NaN or Inf")
    N, K = wf.shape
    blk = wf.reshape(N, K // BLOCK, BLOCK)
    amax = blk.abs().amax(dim=-1)
    nz = amax > 0
    e = torch.where(nz, _floor_log2(torch.where(nz, amax, torch.ones_like(amax))) - 8, torch.zeros_like(amax, dtype=torch.int32))
    e = torch.clamp(e, lo, 127)
    # w * 2^-e in two exact steps (2^-e alone leaves the fp32 range at e = 127); the kernel does the same
    h1 = e >> 1
    s = (blk * _pow2(-h1)[..., None]) * _pow2(-(e - h1))[..., None]
    q = _e4m3_codes(s)
    q = torch.where(nz[..., None], q, torch.zeros_like(q))
    return q.reshape(N, K).contiguous(), (e + 127).to(torch.uint8).contiguous()


@torch.no_grad()
def dequantize_mx8(q: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(q, scale) -> W' = q * 2^(scale - 127) in `dtype` (exact when scale came from quantize_mx8 for that dtype)."""
    N, K = q.shape
    v = _e4m3_values(q).reshape(N, K // BLOCK, BLOCK) * _pow2(scale.to(torch.int32) - 127)[..., None]
    return v.reshape(N, K).to(dtype)


def mx8_bytes(N: int, K: int) -> int:
    """Bytes of one [N, K] MXFP8 weight (codes + scales)."""
    return N * K + N * (K // BLOCK)
