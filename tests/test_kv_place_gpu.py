"""GPU: dl_kv_place (through ops.kv_place / ops.kv_place_arrays) -- the row-mapped, length-aware slab copy that puts a prefill made on a source cache into its rows
of a wider decode cache.  Pure byte movement: every comparison is exact.  Both KV formats, ragged lengths including 0 and t_cap, identity / permuted / strided
maps, the destination's slots past a row's length and its unmapped rows keep their bytes (guard pattern), the lengths travel, an out-of-range entry is skipped with
the rest intact, and the same inside a captured graph."""
import pytest
import torch

pytestmark = pytest.mark.gpu

L, SL, NKV, D = 3, 1, 2, 32
GUARD = 0x5A


def _cache(fmt, B, t_cap, dtype=torch.bfloat16):
    from dynamic_llava_amd.cache import KVSlabCache, KVSlabCacheMX8

    cls = KVSlabCacheMX8 if fmt == "mxfp8" else KVSlabCache
    return cls(L, SL, B, NKV, D, t_cap, dtype, "cuda")


def _arrays(c):
    return [c.slab] + ([c.scales] if c.kv_format == "mxfp8" else [])


def _fill(c, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    for a in _arrays(c):
        a.view(torch.uint8).copy_(torch.randint(0, 256, a.view(torch.uint8).shape, generator=g, dtype=torch.uint8).cuda())
    if lens is not None:
        c.lens.copy_(torch.tensor(lens, dtype=torch.int32))


def _expect(src, dst_before, dst_lens_before, src_rows, dst_rows, max_len=None):
    """The destination's arrays and lengths after the copy, computed on the CPU from snapshots."""
    want = [a.clone() for a in dst_before]
    want_lens = dst_lens_before.clone()
    s_lens = src.lens.cpu()
    B_src, B_dst = src.batch, want[0].shape[2]
    for s, d in zip(src_rows, dst_rows):
        if not (0 <= s < B_src and 0 <= d < B_dst):
            continue
        want_lens[:, d] = s_lens[:, s]
        for a, w in zip(_arrays(src), want):
            T = min(a.shape[4], w.shape[4]) if max_len is None else min(a.shape[4], w.shape[4], max_len)
            for l in range(L):
                n = max(0, min(int(s_lens[1 if l >= SL else 0, s]), T))
                w[l, :, d, :, :n] = a[l, :, s, :, :n].cpu()
    return want, want_lens


def _place(src, dst, src_rows, dst_rows, max_len=None, checked=True):
    from dynamic_llava_amd import hip_ops as ops

    if checked:
        maps = ops.kv_place_maps(src_rows, dst_rows, src.batch, dst.batch, "cuda")
    else:
        maps = (torch.tensor(src_rows, dtype=torch.int32, device="cuda"), torch.tensor(dst_rows, dtype=torch.int32, device="cuda"))
    ops.kv_place(src, dst, *maps, max_len=max_len)
    torch.cuda.synchronize()
    return maps


def _same(dst, want, want_lens):
    return all(torch.equal(a.cpu().view(torch.uint8), w.view(torch.uint8)) for a, w in zip(_arrays(dst), want)) and torch.equal(dst.lens.cpu(), want_lens)


@pytest.mark.parametrize("fmt", [None, "mxfp8"], ids=["model_dtype", "mxfp8"])
@pytest.mark.parametrize("name,src_rows,dst_rows", [("identity", [0, 1, 2], [0, 1, 2]), ("second_half", [0, 1, 2], [3, 4, 5]), ("permuted", [2, 0, 1], [1, 5, 3]),
                                                     ("strided", [0, 2], [0, 4]), ("one_row_twice", [1, 1], [2, 3])])
def test_rows_lengths_and_guards(fmt, name, src_rows, dst_rows):
    T_SRC, T_DST = 40, 56
    src, dst = _cache(fmt, 3, T_SRC), _cache(fmt, 6, T_DST)
    _fill(src, 1, lens=[[40, 0, 17], [33, 0, 5]])  # ragged: t_cap, 0 and odd lengths; the evicted group shorter
    _fill(dst, 2, lens=[[9] * 6, [8] * 6])
    for a in _arrays(dst):
        a.view(torch.uint8).fill_(GUARD)
    before, lens_before = [a.cpu() for a in _arrays(dst)], dst.lens.cpu()
    src_before = [a.clone() for a in _arrays(src)]
    _place(src, dst, src_rows, dst_rows)
    want, want_lens = _expect(src, before, lens_before, src_rows, dst_rows)
    assert _same(dst, want, want_lens), name
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(_arrays(src), src_before))  # the source is only read
    # what must still hold the guard pattern: unmapped rows entirely, mapped rows past the source row's length
    codes = dst.slab.cpu().view(torch.uint8)
    for d in set(range(6)) - set(dst_rows):
        assert bool((codes[:, :, d] == GUARD).all()), (name, d)
    s_lens = src.lens.cpu()
    for s, d in zip(src_rows, dst_rows):
        for l in range(L):
            n = int(s_lens[1 if l >= SL else 0, s])
            assert bool((codes[l, :, d, :, n:] == GUARD).all()), (name, l, d)


@pytest.mark.parametrize("fmt", [None, "mxfp8"], ids=["model_dtype", "mxfp8"])
def test_host_bound_caps_the_copy_and_a_smaller_destination_is_respected(fmt):
    src, dst = _cache(fmt, 2, 48), _cache(fmt, 2, 24)
    _fill(src, 3, lens=[[48, 30], [48, 2]])  # longer than the destination's capacity: the span is cut at it, never past it
    _fill(dst, 4, lens=[[0, 0], [0, 0]])
    before, lens_before = [a.cpu() for a in _arrays(dst)], dst.lens.cpu()
    _place(src, dst, [0, 1], [1, 0])
    want, want_lens = _expect(src, before, lens_before, [0, 1], [1, 0])
    assert _same(dst, want, want_lens)
    _fill(dst, 5, lens=[[0, 0], [0, 0]])
    before, lens_before = [a.cpu() for a in _arrays(dst)], dst.lens.cpu()
    _place(src, dst, [0, 1], [0, 1], max_len=7)  # the host bound sizes the grid: slots past it are not copied
    want, want_lens = _expect(src, before, lens_before, [0, 1], [0, 1], max_len=7)
    assert _same(dst, want, want_lens)


@pytest.mark.parametrize("fmt", [None, "mxfp8"], ids=["model_dtype", "mxfp8"])
def test_an_entry_outside_its_cache_is_skipped_the_rest_intact(fmt):
    from dynamic_llava_amd import hip_ops as ops

    src, dst = _cache(fmt, 3, 32), _cache(fmt, 4, 32)
    _fill(src, 6, lens=[[32, 10, 3], [20, 10, 0]])
    _fill(dst, 7, lens=[[1] * 4, [1] * 4])
    before, lens_before = [a.cpu() for a in _arrays(dst)], dst.lens.cpu()
    src_rows, dst_rows = [0, 3, 1, -1, 2], [2, 0, 4, 1, 3]  # source row 3 and -1, destination row 4: outside
    for bad in ((src_rows, dst_rows), ([0, 0], [1, 1]), ([0], [0, 1]), ([], [])):
        with pytest.raises(ops.HipOpsError, match="no valid map"):  # the host check refuses them ...
            ops.kv_place_maps(*bad, 3, 4, "cuda")
    _place(src, dst, src_rows, dst_rows, checked=False)  # ... and the kernel, handed them anyway, skips them without touching memory outside
    want, want_lens = _expect(src, before, lens_before, src_rows, dst_rows)
    assert _same(dst, want, want_lens)
    assert torch.equal(dst.lens.cpu()[:, :2], lens_before[:, :2])  # rows 0 and 1 were the targets of the skipped entries


def test_inside_a_captured_graph_the_lengths_are_device_data():
    from dynamic_llava_amd import hip_ops as ops

    src, dst = _cache(None, 2, 64), _cache(None, 4, 64)
    _fill(src, 8, lens=[[5, 9], [5, 9]])
    maps = ops.kv_place_maps([0, 1], [2, 3], 2, 4, "cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.kv_place(src, dst, *maps, max_len=64)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.kv_place(src, dst, *maps, max_len=64)
    for seed, lens in ((9, [[64, 0], [31, 0]]), (10, [[1, 63], [1, 40]])):  # new contents, new lengths: the same graph
        _fill(src, seed, lens=lens)
        _fill(dst, seed + 100, lens=[[2] * 4, [2] * 4])
        before, lens_before = [a.cpu() for a in _arrays(dst)], dst.lens.cpu()
        g.replay()
        torch.cuda.synchronize()
        want, want_lens = _expect(src, before, lens_before, [0, 1], [2, 3])
        assert _same(dst, want, want_lens), seed


def test_argument_checks():
    from dynamic_llava_amd import hip_ops as ops

    lib = ops.lib()
    src, dst = _cache(None, 2, 16), _cache(None, 2, 16)
    maps = ops.kv_place_maps([0, 1], [0, 1], 2, 2, "cuda")
    es = src.slab.element_size()
    ss, ds = [src.slab.stride(i) * es for i in range(4)], [dst.slab.stride(i) * es for i in range(4)]

    def call(**kw):
        a = dict(src=src.slab.data_ptr(), dst=dst.slab.data_ptr(), n_layers=L, sl=SL, bs=2, bd=2, n=2, sr=maps[0].data_ptr(), dr=maps[1].data_ptr(), nkv=NKV, rb=D * es, ts=16, td=16,
                 sl_ptr=src.lens.data_ptr(), max_len=16)
        a.update(kw)
        return lib.dl_kv_place(a["src"], a["dst"], *ss, *ds, a["n_layers"], a["sl"], a["bs"], a["bd"], a["n"], a["sr"], a["dr"], a["nkv"], a["rb"], a["ts"], a["td"], a["sl_ptr"], 2,
                               dst.lens.data_ptr(), 2, a["max_len"], None)

    for bad in (dict(src=None), dict(dst=None), dict(sr=None), dict(dr=None), dict(sl_ptr=None), dict(n=0), dict(bs=0), dict(bd=0), dict(rb=0), dict(nkv=0), dict(n_layers=0), dict(sl=L + 1),
                dict(sl=-1), dict(ts=-1), dict(max_len=-1), dict(n=40000)):
        assert call(**bad) == -1 and b"dl_kv_place" in lib.dl_last_error(), bad
    assert call() == 0
    torch.cuda.synchronize()
