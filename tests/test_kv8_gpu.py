"""GPU: the opt-in MXFP8 KV cache -- dl_kv_quantize_mx8 against the host rule, dl_attn_decode_rope_kv8 (exhaustive dequantisation through the
attention, every launch form on the hard inputs of oracle/attn_truth.py, argument checks) and the model with set_kv_cache_format("mxfp8").

The format has an exact definition (mxfp8.py along head_dim): a stored row is read as q * 2^e, exact in the model dtype, and the step's new token is
attended at model-dtype precision.  So a decode step computes attention over [dequantised old rows | exact new row] -- which is what the oracle
computes when it is handed the cache's legacy (dequantised) view, and what the fp64 truth is taken on."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attn_cases as ac  # noqa: E402
from oracle import attn_truth as at  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from oracle.ref_cpu import Oracle  # noqa: E402

from dynamic_llava_amd import hip_ops as ops  # noqa: E402
from dynamic_llava_amd.cache import KVSlabCache, KVSlabCacheMX8  # noqa: E402
from dynamic_llava_amd.mxfp8 import dequantize_mx8, e_min, quantize_mx8  # noqa: E402

DTYPES16 = [torch.bfloat16, torch.float16]
DTYPES = [torch.float32] + DTYPES16
ULP = {torch.float32: 2.0**-23, torch.float16: 2.0**-10, torch.bfloat16: 2.0**-7}
GUARD = 256            # guard band (bytes) on either side of every plane
SENTINEL = 0xA5
NAN_CODE, INF_SCALE = 0x7F, 0xFF  # what lies behind kv_len: an e4m3fn NaN and the E8M0 NaN (2^128 as fp32 bits: Inf)
CODES = [c for c in range(256) if c not in (0x7F, 0xFF)]  # the 254 non-NaN codes
LAUNCH_FORMS = [(s, kif, chunk) for kif in (128, 256) for chunk in (0, 256, 100) for s in (1, 3, 4, 32)]  # every keys-in-flight form the library ships


class Planes:
    """The four planes of one layer, each inside its own guard band: codes uint8 [B, nKV, T_cap, d], scales uint8 [B, nKV, T_cap, d/32]."""

    def __init__(self, B, nKV, T_cap, d, fill):
        self.shape_c, self.shape_s = (B, nKV, T_cap, d), (B, nKV, T_cap, d // 32)
        self.buf, self.views = [], []
        for shp, f in ((self.shape_c, fill[0]), (self.shape_s, fill[1]), (self.shape_c, fill[0]), (self.shape_s, fill[1])):
            n = math.prod(shp)
            b = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
            b[GUARD : GUARD + n] = f
            self.buf.append(b)
            self.views.append(b[GUARD : GUARD + n].view(shp))
        self.kq, self.ks, self.vq, self.vs = self.views

    def clone(self):
        p = Planes.__new__(Planes)
        p.shape_c, p.shape_s = self.shape_c, self.shape_s
        p.buf = [b.clone() for b in self.buf]
        p.views = [b[GUARD : b.numel() - GUARD].view(v.shape) for b, v in zip(p.buf, self.views)]
        p.kq, p.ks, p.vq, p.vs = p.views
        return p

    def guards_intact(self):
        return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()) for b in self.buf)


def _q_rows(x, model_dtype):
    """host rule on rows x [..., d] -> (codes [..., d], scales [..., d/32])"""
    d = x.shape[-1]
    q, s = quantize_mx8(x.reshape(-1, d), model_dtype)
    return q.reshape(x.shape), s.reshape(*x.shape[:-1], d // 32)


def _dq_rows(q, s, dtype):
    d = q.shape[-1]
    return dequantize_mx8(q.reshape(-1, d), s.reshape(-1, d // 32), dtype).reshape(q.shape)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. dl_kv_quantize_mx8 bit-exact to the host rule
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _edge_blocks(dtype):
    """32-element blocks: all zero; an amax in [448, 512) * 2^e (saturates); values at the dtype's e_min clamp (fp16: subnormals); mixed signs; -0.0"""
    tiny = 2.0**-24 if dtype == torch.float16 else 2.0**-130
    rows = [
        [0.0] * 32,
        [500.0, -470.0, 464.0, 448.0, 440.0, -511.0] + [1.0] * 26,
        [tiny, -tiny, 3 * tiny, 5 * tiny, -7 * tiny, 2.0**-16 if dtype == torch.float16 else 2.0**-126] + [0.0] * 26,
        [(-1.0) ** i * (i + 1) * 0.37 for i in range(32)],
        [-0.0] * 16 + [0.0] * 8 + [2.0**-3, -(2.0**-3)] + [-0.0] * 6,
        [256.0, 272.0, 304.0, 280.0, 273.0, -272.0, 1.0625, 1.1875, 2.0**-9, 3 * 2.0**-9, 2.0**-10] + [-0.0] * 21,
    ]
    return torch.tensor(rows, dtype=torch.float32).to(dtype)


def _kvq_expected(k_src, v_src, counts, bases, T_dst, model_dtype, like: Planes):
    exp = [torch.full_like(v, SENTINEL).cpu() for v in like.views]
    B, nKV, T_src, d = k_src.shape
    for b in range(B):
        for j in range(counts[b]):
            slot = bases[b] + j
            if 0 <= slot < T_dst and slot < T_src:
                for src, cq, cs in ((k_src, exp[0], exp[1]), (v_src, exp[2], exp[3])):
                    q, s = quantize_mx8(src[b, :, slot].cpu(), model_dtype)  # the pure-torch host rule, on the CPU
                    cq[b, :, slot], cs[b, :, slot] = q, s
    return exp


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "fp16"])
@pytest.mark.parametrize("d", [64, 128])
def test_kv_quantize_bit_exact_to_host_rule(dtype, d):
    B, nKV, T_dst, T_src = 3, 2, 70, 90
    g = torch.Generator().manual_seed(11 + d)
    k_src = (torch.randn(B, nKV, T_src, d, generator=g) * 2).to(dtype)
    v_src = (torch.randn(B, nKV, T_src, d, generator=g) * 0.01).to(dtype)
    edge = _edge_blocks(dtype)
    for r in range(edge.shape[0]):  # the edge blocks sit inside the ranges below, at every block position of a row
        k_src[1, r % nKV, 6 + r, 32 * (r % (d // 32)) : 32 * (r % (d // 32)) + 32] = edge[r]
        v_src[1, (r + 1) % nKV, 40 + r, 32 * ((r + 1) % (d // 32)) : 32 * ((r + 1) % (d // 32)) + 32] = edge[r]
    k_src[2, :, 69, :32] = edge[1]
    k_dev, v_dev = k_src.cuda(), v_src.cuda()
    counts, bases = [0, 64, 1], [0, 5, 69]
    cu = torch.tensor([0, 0, 64, 65], dtype=torch.int32, device="cuda")
    base = torch.tensor(bases, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    for model_dtype in ({dtype, torch.float16} if dtype == torch.float32 else {dtype}):  # (an fp32 slab under fp16's e_min: source and model dtype are separate arguments)
        pl = Planes(B, nKV, T_dst, d, (SENTINEL, SENTINEL))
        ops.kv_quantize_mx8(k_dev, v_dev, pl.kq, pl.ks, pl.vq, pl.vs, cu, base, 64, model_dtype=model_dtype, err=err)
        torch.cuda.synchronize()
        exp = _kvq_expected(k_src, v_src, counts, bases, T_dst, model_dtype, pl)
        for name, got, want in zip(("k codes", "k scales", "v codes", "v scales"), pl.views, exp):
            assert torch.equal(got.cpu(), want), (name, dtype, model_dtype)  # rows in the ranges bit-exact, every other slot still the sentinel
        assert pl.guards_intact() and int(err.item()) == 0
    assert bool((exp[0][1, :, 5:69] != SENTINEL).any()) and bool((exp[1][2, :, 69] != SENTINEL).all())  # (the expectation is not vacuous)

    # a NaN and an Inf each set err_flag
    for bad in (float("nan"), float("inf")):
        kb = k_dev.clone()
        kb[1, 1, 20, 7] = bad
        err.zero_()
        pl2 = Planes(B, nKV, T_dst, d, (SENTINEL, SENTINEL))
        ops.kv_quantize_mx8(kb, v_dev, pl2.kq, pl2.ks, pl2.vq, pl2.vs, cu, base, 64, err=err)
        assert int(err.item()) == 1, bad
    err.zero_()

    # cu_seqlens and kv_base are read on the device: changed between two replays of ONE captured graph; a slot at or past T_cap is dropped
    pl = Planes(B, nKV, T_dst, d, (SENTINEL, SENTINEL))
    fresh = [b.clone() for b in pl.buf]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.kv_quantize_mx8(k_dev, v_dev, pl.kq, pl.ks, pl.vq, pl.vs, cu, base, 64, err=err)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        ops.kv_quantize_mx8(k_dev, v_dev, pl.kq, pl.ks, pl.vq, pl.vs, cu, base, 64, err=err)
    for counts2, bases2 in ((counts, bases), ([2, 3, 0], [1, 68, 10])):
        for b_, f_ in zip(pl.buf, fresh):
            b_.copy_(f_)
        cu.copy_(torch.tensor([0] + list(torch.tensor(counts2).cumsum(0)), dtype=torch.int32))
        base.copy_(torch.tensor(bases2, dtype=torch.int32))
        gr.replay()
        torch.cuda.synchronize()
        exp = _kvq_expected(k_src, v_src, counts2, bases2, T_dst, dtype, pl)
        for got, want in zip(pl.views, exp):
            assert torch.equal(got.cpu(), want), (counts2, bases2)
        assert pl.guards_intact()
    assert bool((exp[0][1, :, 68:70] != SENTINEL).any())  # slots 68, 69 of row 1 written, slot 70 does not exist


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. exhaustive dequantisation through the attention kernel
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _exp_range(dtype):
    """every scale exponent the dtype allows: e_min through the largest e at which 448 * 2^e is still finite in the dtype"""
    hi = 7 if dtype == torch.float16 else 119
    assert math.isfinite(float(torch.tensor(448.0 * 2.0**hi).to(dtype))) and not math.isfinite(float(torch.tensor(448.0 * 2.0 ** (hi + 1)).to(dtype)))
    return list(range(e_min(dtype), hi + 1))


def _bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES16, ids=["bf16", "fp16"])
@pytest.mark.parametrize("d", [128, 64])
def test_exhaustive_dequantisation_of_v_through_the_attention(dtype, d):
    """One slab key per row whose V row enumerates the 254 non-NaN codes (spread over the d channels of several batch rows), for every scale exponent; the
    new token's key scores 1e4 below the slab key, so its softmax weight underflows to 0 (it cannot be masked) and the output must be the dequantised value,
    rounded once: bit-exact."""
    nH, nKV, T_cap = 2, 1, 3
    exps = _exp_range(dtype)
    rows_per_e = -(-len(CODES) // d)
    B = len(exps) * rows_per_e
    codes = torch.tensor(CODES + [0] * (rows_per_e * d - len(CODES)), dtype=torch.uint8).view(rows_per_e, d)
    pl = Planes(B, nKV, T_cap, d, (NAN_CODE, INF_SCALE))
    vq = codes.repeat(len(exps), 1)                                                       # [B, d]
    vs = torch.tensor([e + 127 for e in exps for _ in range(rows_per_e)], dtype=torch.uint8)[:, None].expand(B, d // 32)
    pl.kq[:, 0, 0] = 0x38  # 1.0
    pl.ks[:, 0, 0] = 127
    pl.vq[:, 0, 0] = vq.cuda()
    pl.vs[:, 0, 0] = vs.cuda()
    qkv = torch.empty(B, (nH + 2 * nKV) * d, dtype=dtype)
    qkv[:, : nH * d], qkv[:, nH * d : (nH + nKV) * d], qkv[:, (nH + nKV) * d :] = 16.0, -128.0, 3.0
    # the new token's score relative to the slab key's, and its softmax weight: exp() of it is 0 in fp32 and in fp64
    rel = (16.0 * -128.0 * d - 16.0 * 1.0 * d) / math.sqrt(d)
    assert rel < -1e4 and math.exp(rel) == 0.0 and float(torch.exp(torch.tensor(rel, dtype=torch.float32))) == 0.0
    cos, sin = ac.rope_table(d, 8, 10000.0, dtype)  # position 0: cos = 1, sin = 0 -- RoPE is the identity
    lens = torch.ones(B, dtype=torch.int32, device="cuda")
    pos = torch.zeros(B, dtype=torch.int32, device="cuda")
    want_v = _dq_rows(vq, vs.contiguous(), dtype)
    assert torch.equal(want_v.float(), _dq_rows(vq, vs.contiguous(), torch.float32)) and bool(torch.isfinite(want_v.float()).all())
    want = (1.0 * want_v.double() + 0.0 * 3.0).to(dtype)  # p = 1 and p_new = 0 exactly; (-0.0) + 0.0 = +0.0, as in any sum that starts from zero
    for kif in (128, 256):
        p2 = pl.clone()
        out = torch.full((B, nH * d), float("nan"), dtype=dtype, device="cuda")
        ops.attn_decode_rope_kv8(qkv.cuda(), cos.cuda(), sin.cuda(), pos, lens, p2.kq, p2.ks, p2.vq, p2.vs, out, None, 1, nH, nKV, d, keys_in_flight=kif, chunk_keys=256)
        torch.cuda.synchronize()
        got = out.cpu().view(B, nH, d)
        for h in range(nH):
            bad = (_bits(got[:, h]) != _bits(want)).nonzero()
            assert bad.numel() == 0, f"kif {kif} head {h}: first mismatch at (row, channel) {bad[0].tolist()}: exponent {exps[int(bad[0][0]) // rows_per_e]}, code {int(vq[bad[0][0], bad[0][1]]):#x}"
        # the appended row: the quantised new key / value at slot 1, the slab key untouched
        kq_new, ks_new = _q_rows(torch.full((d,), -128.0, dtype=dtype), dtype)
        vq_new, vs_new = _q_rows(torch.full((d,), 3.0, dtype=dtype), dtype)
        assert torch.equal(p2.kq[:, 0, 1].cpu(), kq_new.expand(B, d)) and torch.equal(p2.ks[:, 0, 1].cpu(), ks_new.expand(B, d // 32))
        assert torch.equal(p2.vq[:, 0, 1].cpu(), vq_new.expand(B, d)) and torch.equal(p2.vs[:, 0, 1].cpu(), vs_new.expand(B, d // 32))
        assert torch.equal(p2.vq[:, 0, 0], pl.vq[:, 0, 0]) and torch.equal(p2.kq[:, 0, 2], pl.kq[:, 0, 2]) and p2.guards_intact()


def _batched_truth(q, k, v):
    """attn_truth.truth for R independent rows at once: q [R, nH, d], k / v [R, Lk, nKV, d] (taken as they are) -> at.Truth with the R rows on the query axis."""
    R, nH, d = q.shape
    Lk, nKV = k.shape[1], k.shape[2]
    n_rep = nH // nKV
    qd = q.double()
    kd, vd = k.double().repeat_interleave(n_rep, dim=2), v.double().repeat_interleave(n_rep, dim=2)  # [R, Lk, nH, d]
    scale = 1.0 / math.sqrt(d)
    s = torch.einsum("rhd,rkhd->rhk", qd, kd) * scale
    sa = torch.einsum("rhd,rkhd->rhk", qd.abs(), kd.abs()) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    l = e.sum(-1, keepdim=True)
    p = e / l
    O = torch.einsum("rhk,rkhd->rhd", p, vd)
    A = torch.einsum("rhk,rkhd->rhd", p, vd.abs())
    return at.Truth(O, A, sa.max(-1).values, torch.full((R,), Lk), l[..., 0], vd.abs().sum(1), float(s.abs().max()), p[..., 0], list(range(nH)))


@pytest.mark.parametrize("dtype", DTYPES16, ids=["bf16", "fp16"])
@pytest.mark.parametrize("d", [128, 64])
def test_exhaustive_dequantisation_of_k_through_the_score(dtype, d):
    """Every non-NaN code at every scale exponent as ONE element of a slab key, read through the score: the query is one-hot on that channel (a power of two,
    2^(3 - e - floor(log2 |code value|)) where the dtype can hold it, so that the score is +-8 * mantissa / sqrt(d): one e4m3 mantissa step moves the softmax
    weight by percents), the key's other channels hold other codes (times q = 0).  Two slab keys and the new token with known scores (s0 as above, 0, 0) and
    values 1, -1, 0.5.  The output is held to attn_truth's per-element bound against the fp64 softmax of the dequantised operands -- bit-equality with the
    once-rounded truth is not implied: the kernel's exponential is v_exp_f32 (not correctly rounded), so its fp32 result may sit an ulp away from the truth's
    and land on the other side of a 16-bit rounding boundary."""
    nH, nKV, T_cap = 2, 1, 4
    exps = _exp_range(dtype)
    lo, hi = (-24, 15) if dtype == torch.float16 else (-133, 127)  # powers of two the dtype holds (subnormals included)
    n = len(CODES)
    vals = dequantize_mx8(torch.tensor(CODES + [0, 0], dtype=torch.uint8)[None], torch.full((1, 8), 127, dtype=torch.uint8)).flatten().tolist()[:n]  # the codes' unit-scale values
    assert len(vals) == n
    fl = [0 if x == 0 else math.floor(math.log2(abs(x))) for x in vals]
    cos, sin = ac.rope_table(d, 8, 10000.0, dtype)
    worst = (0.0, None)
    CH = 32  # exponents per launch
    for e0 in range(0, len(exps), CH):
        es = exps[e0 : e0 + CH]
        B = len(es) * n
        e_of = torch.tensor([e for e in es for _ in range(n)])
        j_of = torch.arange(n).repeat(len(es))
        c_of = j_of % d
        # slab key 0: channel c holds code j, the others the codes that follow it; slab key 1: zeros
        k0 = torch.tensor(CODES, dtype=torch.uint8)[(j_of[:, None] + torch.arange(d)[None, :] - c_of[:, None]) % n]
        pl = Planes(B, nKV, T_cap, d, (NAN_CODE, INF_SCALE))
        sc_e = (e_of + 127).to(torch.uint8)[:, None].expand(B, d // 32).contiguous()
        one = torch.full((B, d // 32), 127, dtype=torch.uint8)
        pl.kq[:, 0, 0], pl.ks[:, 0, 0] = k0.cuda(), sc_e.cuda()
        pl.kq[:, 0, 1], pl.ks[:, 0, 1] = 0, 127
        pl.vq[:, 0, 0], pl.vs[:, 0, 0] = 0x38, 127   # 1.0
        pl.vq[:, 0, 1], pl.vs[:, 0, 1] = 0xB8, 127   # -1.0
        qe = torch.tensor([min(hi, max(lo, 3 - int(e) - fl[int(j)])) for e, j in zip(e_of.tolist(), j_of.tolist())], dtype=torch.float64)
        qkv = torch.zeros(B, (nH + 2 * nKV) * d, dtype=dtype)
        qv = torch.pow(2.0, qe).to(dtype)
        assert torch.equal(qv.double(), torch.pow(2.0, qe))
        qkv[torch.arange(B), c_of] = qv            # head 0
        qkv[torch.arange(B), d + c_of] = -qv       # head 1: the mirrored score
        qkv[:, (nH + nKV) * d :] = 0.5             # the new token: key 0 (score 0), value 0.5
        lens = torch.full((B,), 2, dtype=torch.int32, device="cuda")
        pos = torch.zeros(B, dtype=torch.int32, device="cuda")
        out = torch.full((B, nH * d), float("nan"), dtype=dtype, device="cuda")
        ops.attn_decode_rope_kv8(qkv.cuda(), cos.cuda(), sin.cuda(), pos, lens, pl.kq, pl.ks, pl.vq, pl.vs, out, None, 1, nH, nKV, d, keys_in_flight=128, chunk_keys=0)
        torch.cuda.synchronize()
        kd = torch.stack([_dq_rows(k0, sc_e, dtype), torch.zeros(B, d, dtype=dtype), torch.zeros(B, d, dtype=dtype)], 1)[:, :, None]
        vd = torch.stack([torch.full((B, d), 1.0, dtype=dtype), torch.full((B, d), -1.0, dtype=dtype), torch.full((B, d), 0.5, dtype=dtype)], 1)[:, :, None]
        t = _batched_truth(qkv[:, : nH * d].view(B, nH, d), kd, vd)
        r, _, i = at.worst_ratio(out.cpu().view(B, nH, d), t, d, dtype)
        if r > worst[0]:
            row = i // (nH * d)
            worst = (r, f"exponent {int(e_of[row])} code {CODES[int(j_of[row])]:#x}")
        assert pl.guards_intact()
        if e0 == 0:  # the scores really move: not every weight is 1/3
            assert float((t.P0 - 1 / 3).abs().max()) > 0.3
    print(f"K through the score, {dtype} d={d}: worst err / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5. hard inputs, every launch form
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _run_hard(dist, dtype, nH, nKV, d, forms=LAUNCH_FORMS, outputs=None):
    """`outputs`: a list that receives, per launch form, the output slice and the appended rows of the four planes; the truth is then not evaluated
    (tools/attn_error_table.py --digest)."""
    qkv, k0, v0, cos, sin = ac.build_decode("rope", dist, dtype, nH, nKV, d)
    B, T_cap = len(ac.DECODE_KV_LEN), ac.DECODE_T_CAP
    lens = torch.tensor(ac.DECODE_KV_LEN, dtype=torch.int32).cuda()
    posd = torch.tensor(ac.DECODE_POS, dtype=torch.int32).cuda()
    cu = torch.arange(0, B + 1, dtype=torch.int32).cuda()
    cosd, sind, qkvd = cos.cuda(), sin.cuda(), qkv.cuda()
    # the rotated q and the rotated new key / value row: dl_rope_kv_write's (bit-exact against the oracle in tests/test_kernels_gpu.py), as run_decode takes them
    ka, va, qa = k0.cuda(), v0.cuda(), qkvd.clone()
    ops.rope_kv_write(qa, cosd, sind, cu, None, posd, lens, ka, va, nH, nKV, d)
    torch.cuda.synchronize()
    q_ref, k_rot, v_rot = qa.cpu()[:, : nH * d].view(B, nH, d), ka.cpu(), va.cpu()
    # the planes: host-quantised rows [0, T), NaN code / Inf scale behind kv_len
    pl0 = Planes(B, nKV, T_cap, d, (NAN_CODE, INF_SCALE))
    exp = [v.cpu().clone() for v in pl0.views]  # expected contents after the launch
    truths = []
    for b, T in enumerate(ac.DECODE_KV_LEN):
        k_old, v_old = k0[b, :, :T], v0[b, :, :T]
        (kq, ks), (vq, vs) = _q_rows(k_old, dtype), _q_rows(v_old, dtype)
        exp[0][b, :, :T], exp[1][b, :, :T], exp[2][b, :, :T], exp[3][b, :, :T] = kq, ks, vq, vs
        k_new, v_new = k_rot[b, :, T], v_rot[b, :, T]  # [nKV, d]
        kk = torch.cat([_dq_rows(kq, ks, dtype).transpose(0, 1), k_new[None]])  # [T + 1, nKV, d]
        vv = torch.cat([_dq_rows(vq, vs, dtype).transpose(0, 1), v_new[None]])
        if outputs is None:
            truths.append(at.truth(q_ref[b][None], kk, vv, heads=ac._heads(nH)))
    for v_, e_ in zip(pl0.views, exp):
        v_.copy_(e_.cuda())
    for b, T in enumerate(ac.DECODE_KV_LEN):  # after the launch: the appended codes and scales = quantize_mx8 of dl_rope_kv_write's rotated key row and value row
        (exp[0][b, :, T], exp[1][b, :, T]), (exp[2][b, :, T], exp[3][b, :, T]) = _q_rows(k_rot[b, :, T], dtype), _q_rows(v_rot[b, :, T], dtype)
    ws = ops.attn_decode_workspace(B, nH, d, 32, "cuda")
    res = {}
    for form in forms:
        n_splits, kif, chunk = form
        pl = pl0.clone()
        qb = qkvd.clone()
        out = torch.full((B, nH * d + 2 * ac.PAD_COLS), float("nan"), dtype=dtype, device="cuda")
        o = out[:, ac.PAD_COLS : ac.PAD_COLS + nH * d]
        ops.attn_decode_rope_kv8(qb, cosd, sind, posd, lens, pl.kq, pl.ks, pl.vq, pl.vs, o, ws, n_splits, nH, nKV, d, keys_in_flight=kif, chunk_keys=chunk)
        torch.cuda.synchronize()
        assert torch.equal(qb, qkvd), f"{form}: qkv was modified"
        w = out.cpu()
        assert bool(torch.isnan(w[:, : ac.PAD_COLS]).all()) and bool(torch.isnan(w[:, ac.PAD_COLS + nH * d :]).all()), f"{form}: written outside the output slice"
        for name, got, want in zip(("k codes", "k scales", "v codes", "v scales"), pl.views, exp):
            assert torch.equal(got.cpu(), want), f"{form}: {name} after the append (appended row = quantize_mx8 of the rotated row; every other slot unchanged)"
        assert pl.guards_intact(), form
        got = w[:, ac.PAD_COLS : ac.PAD_COLS + nH * d].reshape(B, nH, d)
        if outputs is not None:
            outputs.append(got.contiguous())
            outputs.extend(x[torch.arange(B, device="cuda"), :, lens.long()].cpu().contiguous() for x in pl.views)
        worst = (0.0, 0.0, "")
        for b, t in enumerate(truths):
            r, ulps, i = at.worst_ratio(got[b][None][:, t.heads], t, d, dtype)
            if r > worst[0]:
                worst = (r, ulps, f"row {b} (kv_len {ac.DECODE_KV_LEN[b]}) head {t.heads[i // d]} dim {i % d}")
            worst = (worst[0], max(worst[1], ulps), worst[2])
        res[form] = worst
    return res


def _assert_hard(res, what):
    worst = max(res.items(), key=lambda kv: kv[1][0])
    print(f"{what}: worst err / bound {worst[1][0]:.3f} ({worst[1][1]:.2f} ulp) at (n_splits, keys_in_flight, chunk_keys) = {worst[0]}, {worst[1][2]}")
    bad = {k: v for k, v in res.items() if not v[0] <= 1.0}
    assert not bad, f"{what}: outside the bound: {bad}"


@pytest.mark.parametrize("dtype", DTYPES16, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", ac.DECODE_HEADS, ids=lambda h: "h%dkv%dd%d" % h)
@pytest.mark.parametrize("dist", ac.DECODE_DISTS, ids=lambda e: e[0])
def test_hard_inputs_every_launch_form(dist, heads, dtype):
    _assert_hard(_run_hard(dist, dtype, *heads), f"{dist[0]} {heads} {dtype}")


@pytest.mark.parametrize("dist", ac.DECODE_DISTS, ids=lambda e: e[0])
def test_hard_inputs_every_launch_form_fp32(dist):
    _assert_hard(_run_hard(dist, torch.float32, *ac.DECODE_HEADS[1]), f"{dist[0]} {ac.DECODE_HEADS[1]} fp32")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "fp16"])
def test_full_row_writes_nothing(dtype):
    """kv_len = T_cap: the token is attended (over T_cap stored rows and itself) and nothing is written; its neighbour row appends as usual."""
    nH, nKV, d, T_cap = 4, 2, 128, 130
    g = torch.Generator().manual_seed(5)
    B, kv = 2, [T_cap, 7]
    k0, v0 = torch.randn(B, nKV, T_cap, d, generator=g).to(dtype), torch.randn(B, nKV, T_cap, d, generator=g).to(dtype)
    qkv = torch.randn(B, (nH + 2 * nKV) * d, generator=g).to(dtype)
    cos, sin = ac.rope_table(d, 512, 10000.0, dtype)
    lens, posd = torch.tensor(kv, dtype=torch.int32).cuda(), torch.tensor([300, 9], dtype=torch.int32).cuda()
    # rotated rows through dl_rope_kv_write on a slab with one spare slot
    ka, va, qa = torch.zeros(B, nKV, T_cap + 1, d, dtype=dtype).cuda(), torch.zeros(B, nKV, T_cap + 1, d, dtype=dtype).cuda(), qkv.cuda()
    ops.rope_kv_write(qa, cos.cuda(), sin.cuda(), torch.arange(0, B + 1, dtype=torch.int32).cuda(), None, posd, lens, ka, va, nH, nKV, d)
    pl0 = Planes(B, nKV, T_cap, d, (NAN_CODE, INF_SCALE))
    truths = []
    for b, T in enumerate(kv):
        (kq, ks), (vq, vs) = _q_rows(k0[b, :, :T], dtype), _q_rows(v0[b, :, :T], dtype)
        pl0.kq[b, :, :T], pl0.ks[b, :, :T], pl0.vq[b, :, :T], pl0.vs[b, :, :T] = kq.cuda(), ks.cuda(), vq.cuda(), vs.cuda()
        kk = torch.cat([_dq_rows(kq, ks, dtype).transpose(0, 1), ka[b, :, T].cpu()[None]])
        vv = torch.cat([_dq_rows(vq, vs, dtype).transpose(0, 1), va[b, :, T].cpu()[None]])
        truths.append(at.truth(qa.cpu()[b, : nH * d].view(1, nH, d), kk, vv))
    ws = ops.attn_decode_workspace(B, nH, d, 32, "cuda")
    for n_splits, kif, chunk in [(1, 128, 256), (1, 256, 0), (3, 128, 0), (4, 128, 100), (32, 256, 0)]:
        pl = pl0.clone()
        out = torch.full((B, nH * d), float("nan"), dtype=dtype, device="cuda")
        ops.attn_decode_rope_kv8(qkv.cuda(), cos.cuda(), sin.cuda(), posd, lens, pl.kq, pl.ks, pl.vq, pl.vs, out, ws, n_splits, nH, nKV, d, keys_in_flight=kif, chunk_keys=chunk)
        torch.cuda.synchronize()
        for got, before in zip(pl.views, pl0.views):
            assert torch.equal(got[0], before[0]), "the full row's planes were written"
            assert torch.equal(got[1, :, :7], before[1, :, :7]) and torch.equal(got[1, :, 8:], before[1, :, 8:])
        assert bool((pl.kq[1, :, 7] != NAN_CODE).any()) and pl.guards_intact()
        for b, t in enumerate(truths):
            r, _, _ = at.worst_ratio(out.cpu()[b].view(1, nH, d), t, d, dtype)
            assert r <= 1.0, (n_splits, kif, chunk, b, r)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 6. bad arguments
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing():
    dtype, nH, nKV, T_cap, B = torch.bfloat16, 2, 1, 8, 1
    lib = ops.lib()
    p = lambda t: None if t is None else t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def call(d, planes, n_splits=1, kif=128):
        pl = Planes(B, nKV, T_cap, max(32, d // 32 * 32), (0, 127))
        qkv = torch.zeros(B, (nH + 2 * nKV) * d, dtype=dtype, device="cuda")
        cos = torch.ones(16, d, dtype=dtype, device="cuda")
        out = torch.full((B, nH * d), 7.0, dtype=dtype, device="cuda")
        lens = torch.zeros(B, dtype=torch.int32, device="cuda")
        views = [v if keep else None for v, keep in zip(pl.views, planes)]
        before = [b.clone() for b in pl.buf]
        rc = lib.dl_attn_decode_rope_kv8(p(qkv), qkv.stride(0), p(cos), p(cos), 16, p(lens), p(lens), p(views[0]), p(views[1]), p(views[2]), p(views[3]), pl.kq.stride(0), pl.kq.stride(1),
                                         T_cap, p(out), out.stride(0), None, n_splits, kif, 0, B, nH, nKV, d, ops.DL_BF16, st)
        torch.cuda.synchronize()
        assert bool((out.float() == 7.0).all()) and all(torch.equal(a, b) for a, b in zip(pl.buf, before)), "a rejected call launched something"
        return rc, lib.dl_last_error().decode()

    ERR_ARG = call(128, (True, True, True, True), n_splits=0)[0]
    assert ERR_ARG != 0
    for planes in ((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False)):
        rc, msg = call(128, planes)
        assert rc == ERR_ARG and "NULL plane" in msg, msg
    rc, msg = call(96, (True,) * 4)
    assert rc == ERR_ARG and "96" in msg and "unsupported" in msg, msg
    rc, msg = call(80, (True,) * 4)
    assert rc == ERR_ARG and "multiple of 32" in msg, msg
    rc, msg = call(128, (True,) * 4, n_splits=0)
    assert rc == ERR_ARG and "n_splits" in msg, msg
    rc, msg = call(128, (True,) * 4, kif=64)
    assert rc == ERR_ARG and "keys_in_flight" in msg, msg
    # the quantiser: head_dim must be a multiple of the scale block; NULL planes
    src = torch.zeros(1, 1, 8, 64, dtype=dtype, device="cuda")
    pl = Planes(1, 1, 8, 64, (SENTINEL, SENTINEL))
    cu = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    z = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.dl_kv_quantize_mx8(p(src), p(src), src.stride(0), src.stride(1), 8, p(pl.kq), None, p(pl.vq), p(pl.vs), pl.kq.stride(0), pl.kq.stride(1), 8, p(cu), p(z), 1, 1, 1, 64,
                                ops.DL_BF16, ops.DL_BF16, None, st)
    assert rc == ERR_ARG and "NULL" in lib.dl_last_error().decode()
    rc = lib.dl_kv_quantize_mx8(p(src), p(src), src.stride(0), src.stride(1), 8, p(pl.kq), p(pl.ks), p(pl.vq), p(pl.vs), pl.kq.stride(0), pl.kq.stride(1), 8, p(cu), p(z), 1, 1, 1, 48,
                                ops.DL_BF16, ops.DL_BF16, None, st)
    assert rc == ERR_ARG and "multiple of 32" in lib.dl_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in pl.buf)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 7.-13. the model with set_kv_cache_format("mxfp8")
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _build(cfg_ns, sd, clip, dtype, kv=None):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig

    m = build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg_ns), sd, clip.state_dict() if clip is not None else None, dtype=dtype, device="cuda")
    if kv is not None:
        m.set_kv_cache_format(kv)
    return m


def _tiny(seed=2):
    cfg = fx.tiny_config()
    return cfg, fx.make_state_dict(cfg, seed=seed, predictor_gain=50.0), fx.build_clip(cfg, seed=1)


def _batch(cfg, B, seed=0):
    prompts = [fx.make_prompt(cfg, 2 + (3 * b) % 7, 4 + (5 * b) % 11, seed=seed + b) for b in range(B)]
    n = max(p.shape[0] for p in prompts)
    ids, am = torch.zeros(B, n, dtype=torch.long), torch.zeros(B, n, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]] = p
        am[b, : p.shape[0]] = 1
    return ids, am, prompts


def _legacy_clone(pkv, dtype=None):
    """the cache's legacy view (dequantised rows of the padded length) and lengths, cloned to the CPU: what the oracle is handed before a step"""
    layers = tuple((k.cpu().clone() if dtype is None else k.cpu().to(dtype), v.cpu().clone() if dtype is None else v.cpu().to(dtype)) for k, v in pkv[0])
    return layers, [x.clone() for x in pkv[1]]


def _oracle_step(orc, tok, legacy, hip_decision, hip_logit, hip_dtype, counter):
    """one oracle step on the handed cache; a keep / evict decision that sits on the boundary follows the model's (test_mxfp8_gpu's rule) and is counted"""
    l_, p_ = orc.forward(tok, past_key_values=copy.deepcopy(legacy))
    if bool(orc.records["text_decision"][0, 0]) != hip_decision:
        assert fx.decision_may_differ(orc.records["text_logit"][0, 0], orc.dtype, hip_logit, hip_dtype)
        orc.force_text_decision = torch.tensor([[int(hip_decision)]])
        l_, p_ = orc.forward(tok, past_key_values=copy.deepcopy(legacy))
        orc.force_text_decision = None
        counter[0] += 1
    return l_, p_


def test_fp32_tiny_b1_against_the_oracle_on_the_dequantised_cache():
    dtype = torch.float32
    cfg, sd, clip = _tiny()
    off = _build(cfg, sd, clip, dtype)
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    assert model.knobs()["kv_cache_format"] == "mxfp8" and off.knobs()["kv_cache_format"] is None
    ids = fx.make_prompt(cfg, 5, 7)[None]
    images = fx.make_images(cfg, 1)
    forced = fx.make_forced_tokens(cfg, 8, 1, seed=5)
    o = Oracle(cfg, {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}, dtype, clip=clip)
    model.debug_records = {}
    n_forced = [0]
    with torch.no_grad():
        out_off = off(ids.cuda(), images=images.cuda())
        out = model(ids.cuda(), images=images.cuda())
        assert torch.equal(out.logits, out_off.logits), "prefill logits must be bit-identical to the format-off model's"
        pkv, pkv_off = out.past_key_values, out_off.past_key_values
        assert isinstance(pkv, KVSlabCacheMX8) and pkv.kv_format == "mxfp8" and pkv_off.kv_format is None
        assert pkv[1][0].tolist() == pkv_off[1][0].tolist() and pkv[1][-1].tolist() == pkv_off[1][-1].tolist()
        # after the prefill every layer's planes are bit-equal to quantize_mx8 of the format-off model's slab rows
        for i in range(cfg.num_hidden_layers):
            T = int(pkv[1][i][0])
            for slab, codes, scales in ((pkv_off.k[i], pkv.k[i], pkv.ks[i]), (pkv_off.v[i], pkv.v[i], pkv.vs[i])):
                q, s = _q_rows(slab[:, :, :T].cpu(), dtype)
                assert torch.equal(codes[:, :, :T].cpu(), q) and torch.equal(scales[:, :, :T].cpu(), s), f"layer {i}"
        for j in range(8):
            legacy = _legacy_clone(pkv)  # BEFORE the step
            out = model(forced[j][:, None].cuda(), past_key_values=pkv)
            pkv = out.past_key_values
            hd = bool(model.debug_records["text_decision"][0])
            l, p = _oracle_step(o, forced[j][:, None], legacy, hd, model.debug_records["text_logit"].float().cpu()[0], dtype, n_forced)
            assert float((out.logits[0, -1].cpu() - l[0, -1]).abs().max()) < 1e-3, j
            assert int(p[1][-1][0]) == int(pkv[1][-1][0]) and int(p[1][0][0]) == int(pkv[1][0][0]), j
    assert n_forced[0] <= fx.MAX_FORCED_DECISIONS


def test_bf16_tiny_noise_class_against_an_fp32_oracle_on_the_same_cache():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny()
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    off = _build(cfg, sd, clip, dtype)
    clip16 = copy.deepcopy(clip).to(dtype)
    sd16 = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    o, o32 = Oracle(cfg, sd16, dtype, clip=clip16), Oracle(cfg, sd16, torch.float32, clip=clip16)
    ids = fx.make_prompt(cfg, 5, 7)[None]
    images = fx.make_images(cfg, 1).to(dtype)
    forced = fx.make_forced_tokens(cfg, 8, 1, seed=5)
    model.debug_records = {}
    n_forced = [0]
    with torch.no_grad():
        out = model(ids.cuda(), images=images.cuda())
        assert torch.equal(out.logits, off(ids.cuda(), images=images.cuda()).logits)
        pkv = out.past_key_values
        for j in range(8):
            legacy = _legacy_clone(pkv)
            legacy32 = _legacy_clone(pkv, torch.float32)
            out = model(forced[j][:, None].cuda(), past_key_values=pkv)
            pkv = out.past_key_values
            hd = bool(model.debug_records["text_decision"][0])
            htl = model.debug_records["text_logit"].float().cpu()[0]
            l, p = _oracle_step(o, forced[j][:, None], legacy, hd, htl, dtype, n_forced)
            l32, p32 = _oracle_step(o32, forced[j][:, None], legacy32, hd, htl, dtype, n_forced)
            e_hip = float((out.logits[0, -1].float().cpu() - l32[0, -1]).abs().max())
            e_ref = float((l[0, -1].float() - l32[0, -1]).abs().max())
            assert e_hip <= 2.0 * e_ref + 2 * ULP[dtype] * float(l32[0, -1].abs().max()), (j, e_hip, e_ref)
            assert int(p[1][-1][0]) == int(pkv[1][-1][0]) and int(p[1][0][0]) == int(pkv[1][0][0]), j
    assert n_forced[0] <= 2 * fx.MAX_FORCED_DECISIONS


@pytest.mark.parametrize("B", [2, 3])
def test_batched_rows_equal_their_b1_runs(B):
    dtype = torch.float32
    cfg, sd, clip = _tiny()
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    prompts = [fx.make_prompt(cfg, 5, 7, seed=0), fx.make_prompt(cfg, 2, 15, seed=1), fx.make_prompt(cfg, 9, 3, seed=2)][:B]
    images = fx.make_images(cfg, B, seed=3)
    n = max(p.shape[0] for p in prompts)
    ids, am = torch.zeros(B, n, dtype=torch.long), torch.zeros(B, n, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]], am[b, : p.shape[0]] = p, 1
    gen = model.generate(ids.cuda(), attention_mask=am.cuda(), images=images.cuda(), max_new_tokens=6, eos_token_id=None).cpu()
    assert model.last_cache.kv_format == "mxfp8"
    for b in range(B):
        one = model.generate(prompts[b][None].cuda(), images=images[b : b + 1].cuda(), max_new_tokens=6, eos_token_id=None).cpu()
        assert gen[b].tolist() == one[0].tolist(), b


def _gen(model, ids, am, images, n=10):
    return model.generate(ids.cuda(), attention_mask=am.cuda(), images=images.cuda(), max_new_tokens=n, eos_token_id=None, output_scores=True, return_dict_in_generate=True)


def _same(a, b):
    return torch.equal(a["sequences"], b["sequences"]) and all(torch.equal(x, y) for x, y in zip(a["scores"], b["scores"]))


def _generate_equals_forward_loop(model, ids, am, images, n):
    """generate() on the captured graph against an eager forward() loop of the same model fed generate's tokens: tokens, lengths, and bit-equal logits"""
    model.use_hip_graph = True
    res = _gen(model, ids, am, images, n)
    lens_gen = [x.clone() for x in res["past_key_values"][1]]
    assert res["past_key_values"].kv_format == "mxfp8"
    model.use_hip_graph = False
    with torch.no_grad():
        o = model(ids.cuda(), attention_mask=am.cuda(), images=images.cuda())
        pkv = o.past_key_values
        for j in range(1, n):
            o = model(res["sequences"][:, j - 1 : j], past_key_values=pkv)
            pkv = o.past_key_values
            assert torch.equal(o.logits[:, -1].float(), res["scores"][j].float()), f"decode step {j}: forward() loop and generate() differ"
            assert torch.equal(o.logits[:, -1].argmax(-1), res["sequences"][:, j]), j
    assert all(torch.equal(a, b) for a, b in zip(lens_gen, pkv[1])), "KV lengths of generate() and of the forward() loop"
    model.use_hip_graph = True
    return res


def test_b8_small_m_route():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny()
    B = 8
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    ids, am, _ = _batch(cfg, B)
    images = fx.make_images(cfg, B, seed=3).to(dtype)
    _generate_equals_forward_loop(model, ids, am, images, 8)
    st = model._dstate
    assert st.B == B and not st.use_gemv and (st.use_smallm or st.use_lp_mlp)


def test_b4_mxfp8_weights_route():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny()
    B = 4
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    model.set_decode_weight_format("mxfp8", max_batch=8)
    assert model.knobs()["kv_cache_format"] == "mxfp8" and model.knobs()["decode_weight_format"] == "mxfp8"
    ids, am, _ = _batch(cfg, B)
    images = fx.make_images(cfg, B, seed=3).to(dtype)
    _generate_equals_forward_loop(model, ids, am, images, 8)
    assert model._dstate.B == B and model._dstate.use_mx8_gemm


@pytest.mark.parametrize("weights", [None, "mxfp8"])
def test_graph_and_eager_bit_identical_and_generate_equals_forward_loop(weights):
    """B = 1 (the GEMV step; with MXFP8 weights: dl_gemv_mx8): all four combinations of the two formats run."""
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny()
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    if weights:
        model.set_decode_weight_format(weights)
        assert model.kv_cache_format == "mxfp8"
    ids, am, _ = _batch(cfg, 1)
    images = fx.make_images(cfg, 1, seed=3).to(dtype)
    outs = {}
    for graph in (True, False):
        model.use_hip_graph = graph
        outs[graph] = _gen(model, ids, am, images, 10)
    assert _same(outs[True], outs[False]), "hipGraph replay == eager launches"
    _generate_equals_forward_loop(model, ids, am, images, 10)


def test_switching_off_and_pooled_cache_lifecycle():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny()
    model = _build(cfg, sd, clip, dtype)
    ids, am, _ = _batch(cfg, 1)
    ids2 = fx.make_prompt(cfg, 9, 13, seed=7)[None]
    images = fx.make_images(cfg, 1, seed=3).to(dtype)
    gen = lambda i: model.generate(i.cuda(), images=images.cuda(), max_new_tokens=8, eos_token_id=None, output_scores=True, return_dict_in_generate=True)
    tok = lambda i: model.generate(i.cuda(), images=images.cuda(), max_new_tokens=8, eos_token_id=None)
    base, base2 = gen(ids), gen(ids2)
    model.set_kv_cache_format("mxfp8")
    assert model._cache_pool is None and model._dstate is None and model._prefill_graphs == {}
    a1 = tok(ids)  # pooled cache: first sighting, capture, replay
    pool = model._cache_pool
    assert isinstance(pool, KVSlabCacheMX8)
    a2, a3 = tok(ids), tok(ids)
    assert model._cache_pool is pool and torch.equal(a1, a2) and torch.equal(a1, a3)
    b1 = tok(ids2)  # another prompt length on the same pooled planes
    assert model._cache_pool is pool
    b2 = tok(ids2)
    assert torch.equal(b1, b2) and torch.equal(tok(ids), a1)
    k8, k8_2 = gen(ids), gen(ids2)  # (return_dict hands the cache to the caller: the pool is rebuilt next time)
    assert torch.equal(k8["sequences"], a1) and torch.equal(k8_2["sequences"], b1) and k8["past_key_values"].kv_format == "mxfp8"
    assert torch.equal(tok(ids), a1) and isinstance(model._cache_pool, KVSlabCacheMX8) and model._cache_pool is not pool
    # the prefill is unchanged arithmetic: the first token's scores are the format-off model's
    assert torch.equal(k8["scores"][0], base["scores"][0]) and torch.equal(k8_2["scores"][0], base2["scores"][0])
    model.set_kv_cache_format(None)
    assert model._cache_pool is None and model.knobs()["kv_cache_format"] is None
    back, back2 = gen(ids), gen(ids2)
    assert _same(back, base) and _same(back2, base2), "switching the format off reproduces the original model bit for bit"
    assert back["past_key_values"].kv_format is None and type(back["past_key_values"]) is KVSlabCache
    with pytest.raises(ValueError):
        model.set_kv_cache_format("fp8")


def test_memory_and_unsupported_calls():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny()
    assert cfg.hidden_size // cfg.num_attention_heads == 128
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    off = _build(cfg, sd, clip, dtype)
    ids, am, _ = _batch(cfg, 1)
    images = fx.make_images(cfg, 1, seed=3).to(dtype)
    res = _gen(model, ids, am, images, 4)
    res_off = _gen(off, ids, am, images, 4)
    c8, c16 = res["past_key_values"], res_off["past_key_values"]
    assert c8.t_cap == c16.t_cap and c8.nbytes() / c16.nbytes() == 132 / 256 and round(c8.nbytes() / c16.nbytes(), 3) == 0.516
    assert c8.nbytes() == c8.slab.numel() + c8.scales.numel() and c16.nbytes() == c16.slab.numel() * 2
    # not built in this mode: a multi-token chunk on a non-empty cache (with and without the instruct predictor), generate(past_key_values=...)
    chunk = fx.make_forced_tokens(cfg, 3, 1, seed=9).view(1, 3)
    with pytest.raises(NotImplementedError, match="mxfp8"):
        model(chunk.cuda(), past_key_values=c8)
    with pytest.raises(NotImplementedError, match="mxfp8"):
        model.generate(chunk.cuda(), past_key_values=c8, max_new_tokens=2, eos_token_id=None)
    cfg_i = fx.tiny_config(use_instruct_predictor=True)
    sd_i = fx.make_state_dict(cfg_i, seed=2, predictor_gain=50.0)
    mi = _build(cfg_i, sd_i, clip, dtype, "mxfp8")
    with torch.no_grad():
        ci = mi(ids.cuda(), images=images.cuda()).past_key_values
    assert ci.kv_format == "mxfp8"
    with pytest.raises(NotImplementedError, match="mxfp8"):
        mi(chunk.cuda(), past_key_values=ci)
    # use_cache=False keeps its model-dtype scratch cache and is unaffected
    with torch.no_grad():
        a = model(ids.cuda(), images=images.cuda(), use_cache=False).logits
        b = off(ids.cuda(), images=images.cuda(), use_cache=False).logits
    assert torch.equal(a, b) and model._scratch_cache.kv_format is None
    # the format-off model refuses nothing it did before
    with torch.no_grad():
        off(chunk.cuda(), past_key_values=c16)
