"""MXFP8 KV cache, host side: the cache class on the CPU, and the reference the GPU tests compare against -- the fp64 truth must be taken on the
operands the kernel reads (the dequantised slab rows and the exact new row), not on the unquantised ones."""

import pytest
import torch

from dynamic_llava_amd import mxfp8
from dynamic_llava_amd.cache import KVSlabCache, KVSlabCacheMX8
from oracle import attn_cases as ac
from oracle import attn_truth as at

DTYPES = [torch.bfloat16, torch.float16]


def _rows(L, B, nKV, T, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, nKV, T, d, generator=g).to(dtype), (torch.randn(B, nKV, T, d, generator=g) * 3).to(dtype)) for _ in range(L)]


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32])
@pytest.mark.parametrize("d", [64, 128])
def test_cache_class_on_cpu(dtype, d):
    L, SL, B, nKV, T_cap = 3, 1, 2, 2, 40
    c = KVSlabCacheMX8(L, SL, B, nKV, d, T_cap, dtype, "cpu")
    assert isinstance(c, KVSlabCache) and c.kv_format == "mxfp8" and KVSlabCache.kv_format is None
    assert c.slab.shape == (L, 2, B, nKV, T_cap, d) and c.slab.dtype == torch.uint8
    assert c.scales.shape == (L, 2, B, nKV, T_cap, d // 32) and c.scales.dtype == torch.uint8
    for i in range(L):
        assert c.k[i].shape == c.v[i].shape == (B, nKV, T_cap, d) and c.ks[i].shape == c.vs[i].shape == (B, nKV, T_cap, d // 32)
        assert c.k[i].data_ptr() == c.slab[i, 0].data_ptr() and c.vs[i].data_ptr() == c.scales[i, 1].data_ptr()
    assert c.nbytes() == L * 2 * B * nKV * T_cap * (d + d // 32) == mxfp8.kv_mx8_bytes(L, B, nKV, T_cap, d)
    assert c.dtype == dtype  # the model dtype: its e_min clamps the block exponents

    # import of a legacy tuple with the host rule; the legacy view is dequantize_mx8 of the planes
    T = 9
    layers = _rows(L, B, nKV, T, d, dtype, seed=d)
    lens = [torch.tensor([T, T - 2]) for _ in range(L)]
    c = KVSlabCache.from_legacy_cache((layers, lens), SL, t_cap_extra=5, kv_format="mxfp8")
    assert isinstance(c, KVSlabCacheMX8) and c.t_cap == T + 5 and c.full_len_host == [T, T - 2] and c.lens.tolist() == [[T, T - 2], [T, T - 2]]
    for i in range(L):
        for x, codes, scales, got in ((layers[i][0], c.k[i], c.ks[i], c[0][i][0]), (layers[i][1], c.v[i], c.vs[i], c[0][i][1])):
            q, s = mxfp8.quantize_mx8(x.reshape(-1, d), dtype)
            assert torch.equal(codes[:, :, :T].reshape(-1, d), q) and torch.equal(scales[:, :, :T].reshape(-1, d // 32), s)
            assert got.dtype == dtype and got.shape == (B, nKV, T, d)
            assert torch.equal(got, mxfp8.dequantize_mx8(q, s, dtype).reshape(B, nKV, T, d))
            # every dequantised value is exact in the model dtype
            assert torch.equal(got.float(), mxfp8.dequantize_mx8(q, s, torch.float32).reshape(B, nKV, T, d))
    # idempotent: quantising K' again gives the same codes
    c2 = KVSlabCache.from_legacy_cache(([c[0][i] for i in range(L)], c[1]), SL, t_cap_extra=5, kv_format="mxfp8")
    assert torch.equal(c2.slab[:, :, :, :, :T], c.slab[:, :, :, :, :T]) and torch.equal(c2.scales[:, :, :, :, :T], c.scales[:, :, :, :, :T])
    assert KVSlabCacheMX8.from_legacy_cache((layers, lens), SL).kv_format == "mxfp8"
    assert KVSlabCache.from_legacy_cache((layers, lens), SL).kv_format is None  # the default is unchanged
    with pytest.raises(ValueError, match="fp4"):
        KVSlabCache.from_legacy_cache((layers, lens), SL, kv_format="fp4")

    # ensure_capacity keeps the contents (and the bookkeeping follows the base class)
    before = (c.slab[:, :, :, :, :T].clone(), c.scales[:, :, :, :, :T].clone(), c.t_cap, c.logical_cap, c.sparse_cap)
    assert not c.ensure_capacity(5) and c.ensure_capacity(6)
    assert c.t_cap > before[2] and c.logical_cap - before[3] == c.sparse_cap - before[4] == c.t_cap - before[2]
    assert c.slab.shape[4] == c.scales.shape[4] == c.t_cap and c.k[1].data_ptr() == c.slab[1, 0].data_ptr() and c.ks[1].data_ptr() == c.scales[1, 0].data_ptr()
    assert torch.equal(c.slab[:, :, :, :, :T], before[0]) and torch.equal(c.scales[:, :, :, :, :T], before[1])
    assert c.nbytes() == L * 2 * B * nKV * c.t_cap * (d + d // 32)
    # the scratch the prefill appends through is one layer's slab
    sk, sv = c.prefill_scratch()
    assert sk.shape == sv.shape == (B, nKV, c.t_cap, d) and sk.dtype == dtype


def test_cache_refuses_what_the_format_is_not_defined_for():
    with pytest.raises(ValueError, match="multiple of 32"):
        KVSlabCacheMX8(1, 0, 1, 1, 48, 8, torch.bfloat16, "cpu")
    with pytest.raises(ValueError, match="dtype"):
        KVSlabCacheMX8(1, 0, 1, 1, 64, 8, torch.float64, "cpu")
    with pytest.raises(ValueError):
        mxfp8.check_kv_cache_format("fp8")
    mxfp8.check_kv_cache_format(None)
    mxfp8.check_kv_cache_format("mxfp8")


def test_memory_ratio_of_the_format():
    """d + d/32 bytes per row against 2 d: 0.516 of a 16-bit slab at d = 128 (0.258 of an fp32 one)."""
    a = KVSlabCacheMX8(2, 1, 1, 2, 128, 16, torch.bfloat16, "cpu")
    b = KVSlabCache(2, 1, 1, 2, 128, 16, torch.bfloat16, "cpu")
    assert a.nbytes() / b.nbytes() == 132 / 256
    assert round(a.nbytes() / b.nbytes(), 3) == 0.516


def rope_rows(x, cos, sin, pos):
    """x [..., d] in the model dtype -> x * cos + rotate_half(x) * sin at position `pos`, every operation rounded to the dtype (DML:283-284)."""
    d = x.shape[-1]
    c, s = cos[pos], sin[pos]
    rot = torch.cat([-x[..., d // 2 :], x[..., : d // 2]], dim=-1)
    return (x * c) + (rot * s)


def dequantised(x, dtype):
    """x [..., d] -> the values a kernel reads back from the MXFP8 planes."""
    d = x.shape[-1]
    q, s = mxfp8.quantize_mx8(x.reshape(-1, d), dtype)
    out = mxfp8.dequantize_mx8(q, s, dtype)
    assert torch.equal(out.float(), mxfp8.dequantize_mx8(q, s, torch.float32)), "a dequantised value is not exact in the model dtype"
    return out.reshape(x.shape)


def kv8_operands(dist_entry, dtype, nH, nKV, d, seed=0):
    """Per row of attn_cases.build_decode's batch: (rotated q [1, nH, d], K, V [T + 1, nKV, d] unquantised, K', V' = [dequantised rows [0, T) | exact new row])."""
    qkv, k0, v0, cos, sin = ac.build_decode("rope", dist_entry, dtype, nH, nKV, d, seed)
    out = []
    for b, T in enumerate(ac.DECODE_KV_LEN):
        pos = ac.DECODE_POS[b]
        q = rope_rows(qkv[b, : nH * d].view(nH, d), cos, sin, pos)[None]
        k_new = rope_rows(qkv[b, nH * d : (nH + nKV) * d].view(nKV, d), cos, sin, pos)[None]
        v_new = qkv[b, (nH + nKV) * d :].view(nKV, d)[None]
        k_old, v_old = k0[b, :, :T].transpose(0, 1), v0[b, :, :T].transpose(0, 1)
        k, v = torch.cat([k_old, k_new]), torch.cat([v_old, v_new])
        kq, vq = torch.cat([dequantised(k_old, dtype), k_new]), torch.cat([dequantised(v_old, dtype), v_new])
        out.append((q, k, v, kq, vq))
    return out


@pytest.mark.parametrize("dist", ac.DECODE_DISTS, ids=lambda e: e[0])
def test_truth_must_be_taken_on_the_dequantised_operands(dist):
    """bf16 and fp16, heads (8, 2, 128) and (4, 4, 64): the emulated kernel on [dequantised rows | exact new row] stays inside the bound of the truth on THOSE
    operands in every cell, and the truth on the unquantised operands lies outside that bound for every distribution -- so a kernel that drops a scale or reads the
    wrong block cannot pass the GPU test, nor can a test that compares with the wrong truth.  (Per cell the shift is 6x .. 2600x the bound, except where the new
    token -- which is exact -- carries the row: `newtok` shows 0.95x at d = 64 in bf16, 2.5x .. 12.5x in its other cells; hence the maximum over the cells.)"""
    shift_max = 0.0
    for nH, nKV, d in [(8, 2, 128), (4, 4, 64)]:
        for dtype in DTYPES:
            worst_in, worst_out = 0.0, 0.0
            for b, (q, k, v, kq, vq) in enumerate(kv8_operands(dist, dtype, nH, nKV, d)):
                t_q = at.truth(q, kq, vq)
                r_in, _, _ = at.worst_ratio(at.emulate(q, kq, vq), t_q, d, dtype)
                worst_in = max(worst_in, r_in)
                # how far the truth on the unquantised operands sits from the one on the operands the kernel reads, in units of the bound
                shift = float(((at.truth(q, k, v).O - t_q.O).abs() / at.bound(t_q, d, dtype)).max())
                worst_out = max(worst_out, shift)
                if ac.DECODE_KV_LEN[b] == 0:
                    assert shift == 0.0  # nothing is read from the planes: the new row is exact
            print(f"{dist[0]} h{nH}kv{nKV}d{d} {dtype}: emulation / bound {worst_in:.3f}, shift of the unquantised truth / bound {worst_out:.2f}")
            assert worst_in <= 1.0, (nH, nKV, d, dtype, worst_in)
            shift_max = max(shift_max, worst_out)
    assert shift_max > 1.0, shift_max
