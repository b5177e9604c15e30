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


# ---- decode batches of 4..32 rows: what the host computes for dl_gemm_mx8 (csrc/gemm_mx8.hip) ----
GEMM_MAX_M = 32          # rows dl_gemm_mx8 takes
GEMM_K_UNIT = 256        # K slices are multiples of the kernel's chunk
_GEMM_WAVES = 8
_GEMM_STAGE_BYTES = 16 * (GEMM_K_UNIT + 16) + 16 * 8  # per wave: 16 code rows of 256 + 16 bytes, 16 x 8 scale bytes
_GEMM_LDS_BYTES = 150 * 1024


def check_decode_weight_format(fmt, max_batch, gemv_max_decode_batch: int) -> None:
    """Argument rule of set_decode_weight_format / load_pretrained_model: fmt is None or "mxfp8"; max_batch is None or an int in [gemv_max_decode_batch, 32] and needs
    fmt == "mxfp8".  Raises ValueError."""
    if fmt not in (None, "mxfp8"):
        raise ValueError(f"decode weight format {fmt!r}: expected None or 'mxfp8'")
    if max_batch is None:
        return
    if fmt is None:
        raise ValueError("max_batch needs the decode weight format 'mxfp8'")
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or not (gemv_max_decode_batch <= max_batch <= GEMM_MAX_M):
        raise ValueError(f"max_batch={max_batch!r}: expected None or an int in [{gemv_max_decode_batch}, {GEMM_MAX_M}]")


def check_kv_cache_format(fmt) -> None:
    """Argument rule of set_kv_cache_format / load_pretrained_model: None (the model dtype) or "mxfp8".  Raises ValueError."""
    if fmt not in (None, "mxfp8"):
        raise ValueError(f"KV cache format {fmt!r}: expected None or 'mxfp8'")


def kv_mx8_bytes(n_layers: int, batch: int, n_kv_heads: int, t_cap: int, head_dim: int) -> int:
    """Bytes of an MXFP8 KV cache (cache.KVSlabCacheMX8): K and V, codes + one scale byte per 32 elements."""
    return n_layers * 2 * batch * n_kv_heads * t_cap * (head_dim + head_dim // BLOCK)


def gemm_mx8_slices(M: int, N: int, K: int, n_slices: int = 0) -> int:
    """The split-K factor dl_gemm_mx8 uses for a call (dl_gemm_mx8_slices); 0 for a shape it rejects.  n_slices 0 = automatic: 4 for the wide projections (at least
    1024 sixteen-neuron tiles), 8 otherwise; raised until one K slice of X (16 or 32 rows of the 16-bit dtype, rows padded by 8 elements) fits the LDS left beside the
    eight waves' staging; never more than K / 256."""
    if not (0 < M <= GEMM_MAX_M and N > 0 and K > 0 and K % GEMM_K_UNIT == 0 and N % 4 == 0 and 0 <= n_slices <= 64):
        return 0
    units = K // GEMM_K_UNIT
    rows = 16 if M <= 16 else 32
    budget = _GEMM_LDS_BYTES - _GEMM_WAVES * _GEMM_STAGE_BYTES
    max_ks = (budget // (rows * 2) - 8) // GEMM_K_UNIT * GEMM_K_UNIT
    s_lds = 1
    while -(-units // s_lds) * GEMM_K_UNIT > max_ks:
        s_lds += 1
    s = n_slices if n_slices > 0 else (4 if (N + 15) // 16 >= 1024 else 8)
    return min(max(s, s_lds), units)


def gemm_mx8_slice_bounds(K: int, slices: int):
    """[(k0, k1)] of every slice: K / 256 units dealt out as evenly as integer division allows (slice s covers units [units*s // slices, units*(s+1) // slices))."""
    units = K // GEMM_K_UNIT
    return [(units * s // slices * GEMM_K_UNIT, units * (s + 1) // slices * GEMM_K_UNIT) for s in range(slices)]


def gemm_mx8_workspace_bytes(M: int, N: int, K: int, n_slices: int = 0) -> int:
    """Bytes of the fp32 workspace of a dl_gemm_mx8 call (dl_gemm_mx8_workspace_bytes): slices x M x N partial sums."""
    return gemm_mx8_slices(M, N, K, n_slices) * M * N * 4
