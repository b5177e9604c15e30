"""GPU, kernel level: dl_kv_fork (the length-aware, replicated KV-slab copy behind generate(num_return_sequences=n)) against a torch-indexing restatement, bit for bit.

A copy has no tolerance: every comparison is torch.equal on bytes.  The destination is a strided view of a larger, sentinel-filled allocation with guard bands around
both buffers, and the WHOLE allocation is compared, so a byte written anywhere it should not be fails the case; a second launch must leave equal bits.  Shapes are the
smallest that reach every branch: 16-byte accesses (aligned capacities 64 / 128), the narrower routes (odd capacities 37 / 50 with 2- and 4-byte rows; bases skewed
by 1, 2 and 8 bytes), byte tails (a span that is no multiple of the access), more than one chunk per span (512-byte rows x 64 live slots = 2 chunks of 16 KiB), ragged
lengths with 0, 1, exactly T_cap and one above both capacities."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 256
L = 3


def _buffer(shape, skew, gen=None):
    """uint8 tensor of `shape` inside a flat allocation with guard bands (the leading one skewed by `skew` bytes) -> (flat, view)."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((GUARD + skew + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = flat[GUARD + skew : GUARD + skew + n].view(shape)
    if gen is not None:
        view.copy_(torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8))
    return flat, view


def _restated(src, dst_big, B, n_rep, H, sparse_layer, lens, cap):
    """What dst's allocation must hold: slots [0, min(len, cap)) of source (l, p, b, h) at rows b * n_rep + r, everything else as it was."""
    want = dst_big.clone()
    for l, b, r in itertools.product(range(L), range(B), range(n_rep)):
        n = max(0, min(int(lens[int(l >= sparse_layer)][b]), cap))
        want[l, :, b * n_rep + r, :H, :n, :] = src[l, :, b, :, :n, :]
    return want


def _lens(B, Ts, Td, roll):
    g0 = [Ts, 1, max(Ts, Td) + 70]  # exactly the source capacity; one slot; above both capacities: clamped, never overrun
    g1 = [0, 7, Ts - 1]
    rot = lambda x: (x[roll % 3 :] + x[: roll % 3])[:B]
    return [rot(g0), rot(g1)]


CAPS = [(37, 50), (64, 128), (50, 37)]  # (source, destination): odd ones force the narrow routes for small rows; the last clamps at the DESTINATION's capacity


@pytest.mark.parametrize("caps", CAPS, ids=lambda c: f"T{c[0]}to{c[1]}")
@pytest.mark.parametrize("row_bytes", [2, 4, 128, 256, 512])
def test_fork_matches_the_restatement_on_every_route(row_bytes, caps):
    from dynamic_llava_amd import hip_ops as ops

    Ts, Td = caps
    gen = torch.Generator().manual_seed(row_bytes * 1000 + Ts)
    for i, (sl, B, n_rep, H) in enumerate(itertools.product((0, 1, 3), (1, 3), (1, 2, 5), (1, 2))):
        skew_s, skew_d = (0, 1, 8, 2)[i % 4], (0, 0, 8, 4)[(i // 2) % 4]
        src_flat, src = _buffer((L, 2, B, H, Ts, row_bytes), skew_s, gen)
        # dst: a view of a larger allocation (one more row, one more head): its row and plane strides are not those of a dense tensor
        big_flat, big = _buffer((L, 2, B * n_rep + 1, H + 1, Td, row_bytes), skew_d)
        dst = big[:, :, : B * n_rep, :H]
        lens = _lens(B, Ts, Td, i)
        src_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
        dst_lens = torch.full((2, B * n_rep), -9, dtype=torch.int32, device="cuda") if i % 2 == 0 else None
        max_len = 5 if i % 7 == 3 else None  # the host bound clamps too
        src_before = src_flat.clone()
        want = _restated(src, big, B, n_rep, H, sl, lens, min(Ts, Td, 5 if max_len else 1 << 30))
        ops.kv_fork_arrays(src, dst, sl, n_rep, src_lens, dst_lens, max_len)
        got1 = big_flat.clone()
        ops.kv_fork_arrays(src, dst, sl, n_rep, src_lens, dst_lens, max_len)
        torch.cuda.synchronize()
        case = (sl, B, n_rep, H, skew_s, skew_d, max_len)
        assert torch.equal(big, want), case
        assert bool((big_flat[: GUARD + skew_d] == SENTINEL).all()) and bool((big_flat[-GUARD:] == SENTINEL).all()), case
        assert torch.equal(got1, big_flat), case  # a second launch: equal bits
        assert torch.equal(src_flat, src_before), case
        if dst_lens is not None:
            assert torch.equal(dst_lens, src_lens.repeat_interleave(n_rep, dim=1)), case  # the source's values as they are, unclamped


def test_captured_launch_follows_the_device_lengths():
    from dynamic_llava_amd import hip_ops as ops

    B, n_rep, H, Ts, Td, w, sl = 3, 2, 2, 64, 128, 256, 1
    gen = torch.Generator().manual_seed(5)
    _, src = _buffer((L, 2, B, H, Ts, w), 0, gen)
    big_flat, big = _buffer((L, 2, B * n_rep + 1, H + 1, Td, w), 0)
    dst = big[:, :, : B * n_rep, :H]
    first, second = [[3, 64, 0], [9, 1, 20]], [[64, 0, 17], [2, 33, 1]]
    src_lens = torch.tensor(first, dtype=torch.int32, device="cuda")
    dst_lens = torch.zeros((2, B * n_rep), dtype=torch.int32, device="cuda")
    want1 = _restated(src, big, B, n_rep, H, sl, first, Ts)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.kv_fork_arrays(src, dst, sl, n_rep, src_lens, dst_lens)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    big_flat.fill_(SENTINEL)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.kv_fork_arrays(src, dst, sl, n_rep, src_lens, dst_lens)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(big, want1) and torch.equal(dst_lens, src_lens.repeat_interleave(n_rep, dim=1))
    big_flat.fill_(SENTINEL)
    src_lens.copy_(torch.tensor(second, dtype=torch.int32))
    want2 = _restated(src, big, B, n_rep, H, sl, second, Ts)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(big, want2) and not torch.equal(want1, want2) and torch.equal(dst_lens, src_lens.repeat_interleave(n_rep, dim=1))


@pytest.mark.parametrize("fmt", [None, "mxfp8"])
def test_cache_front_door(fmt):
    """hip_ops.kv_fork on KVSlabCache (bf16 slab) and KVSlabCacheMX8 (codes + scale bytes: d / 32 = 2 bytes per row)."""
    from dynamic_llava_amd import hip_ops as ops
    from dynamic_llava_amd.cache import KVSlabCache, KVSlabCacheMX8

    cls = KVSlabCacheMX8 if fmt else KVSlabCache
    B, n, nKV, d, sl = 2, 3, 2, 64, 1
    src = cls(L, sl, B, nKV, d, 37, torch.bfloat16, "cuda")
    dst = cls(L, sl, B * n, nKV, d, 50, torch.bfloat16, "cuda")
    gen = torch.Generator().manual_seed(9)
    arrays = [("slab", src.slab.element_size())] + ([("scales", 1)] if fmt else [])
    for name, _ in arrays:
        s_ = getattr(src, name)
        s_.view(torch.uint8).copy_(torch.randint(0, 256, s_.view(torch.uint8).shape, generator=gen, dtype=torch.uint8))
        getattr(dst, name).view(torch.uint8).fill_(SENTINEL)
    lens = [[37, 12], [5, 0]]
    src.lens.copy_(torch.tensor(lens, dtype=torch.int32))
    ops.kv_fork(src, dst, n)
    torch.cuda.synchronize()
    assert torch.equal(dst.lens, src.lens.repeat_interleave(n, dim=1))
    for name, _ in arrays:
        s_, d_ = getattr(src, name).view(torch.uint8), getattr(dst, name).view(torch.uint8)
        want = torch.full_like(d_, SENTINEL)
        for l, b, r in itertools.product(range(L), range(B), range(n)):
            m = lens[int(l >= sl)][b]
            want[l, :, b * n + r, :, :m] = s_[l, :, b, :, :m]
        assert torch.equal(d_, want), name
    with pytest.raises(ops.HipOpsError):
        ops.kv_fork(src, dst, 2)  # 2 x 2 rows do not fill a destination of 6
