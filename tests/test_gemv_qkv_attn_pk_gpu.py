"""GPU: dl_gemv_qkv_attn_pk (the fused q|k|v + attention launch with the projection rows streamed as lossless 12-bit packed bf16) must return
dl_gemv_qkv_attn's bits on the unpacked matrix -- the projection row, h_out, the K/V slabs after the append and the attention output -- on every split
count and head dim, with escapes of every kind, on a grid so small that every streaming workgroup runs several (and a ragged last) pass, and on views
that end exactly at the end of their storage.  Bad arguments are refused with DL_ERR_ARG before anything is launched."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import bf16pack as bp  # noqa: E402
from dynamic_llava_amd import hip_ops as ops  # noqa: E402

BF = torch.bfloat16
EPS = 1e-5


def _bits(t):
    return t.view(torch.int16)


def _rnd(g, *shape, s=0.02):
    return (torch.randn(*shape, device="cuda", generator=g) * s).to(BF)


def _pack(w):
    p = bp.pack(w, force=True)
    assert torch.equal(_bits(bp.unpack(p)), _bits(w))  # the format is lossless on this very matrix
    return p


class _Case:
    """One layer's operands: the matrix (bf16 and packed), the norm weight, RoPE tables, K/V slabs with T_old valid rows, a granule buffer."""

    def __init__(self, nH, nKV, d, H, T_old, seed=11, W=None):
        from oracle.ref_cpu import rope_table

        g = self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.nH, self.nKV, self.d, self.H, self.T_old = nH, nKV, d, H, T_old
        self.N = (nH + 2 * nKV) * d
        self.W = _rnd(g, self.N, H) if W is None else W
        self.p = _pack(self.W)
        self.nw = 1 + _rnd(g, H, s=0.1)
        self.T_cap = T_old + 40
        self.cos, self.sin = (t.cuda() for t in rope_table(d, self.T_cap + 8, 10000.0, BF))
        self.err = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.gran = ops.gemv_qkv_attn_workspace(nH, nKV, d, "cuda")
        self.k0, self.v0 = _rnd(g, 1, nKV, self.T_cap, d, s=1.0), _rnd(g, 1, nKV, self.T_cap, d, s=1.0)

    def step_inputs(self, step, with_delta=True):
        h0, delta = _rnd(self.g, 1, self.H, s=1.0), (_rnd(self.g, 1, self.H, s=1.0) if with_delta else None)
        lens = torch.tensor([self.T_old + step], dtype=torch.int32, device="cuda")
        pos = torch.tensor([self.T_old + step + 3], dtype=torch.int32, device="cuda")
        return h0, delta, lens, pos

    def run(self, packed, h0, delta, lens, pos, tag, n_splits=1, grid_cap=0, p=None):
        """-> (qkv, h_out, k slab, v slab, out) of one launch on copies of the slabs."""
        k, v = self.k0.clone(), self.v0.clone()
        qkv = torch.full((1, self.N), 3.0, dtype=BF, device="cuda")
        ho = torch.full((1, self.H), 5.0, dtype=BF, device="cuda")
        out = torch.full((1, self.nH * self.d), 7.0, dtype=BF, device="cuda")
        fn, wt = (ops.gemv_qkv_attn_pk, p or self.p) if packed else (ops.gemv_qkv_attn, self.W)
        fn(wt, qkv, h0, ho, delta, self.nw, EPS, self.cos, self.sin, pos, lens, k, v, out, self.gran, tag, self.nH, self.nKV, self.d, err=self.err,
           n_splits=n_splits, grid_cap=grid_cap)
        return qkv, ho, k, v, out


def _assert_same(got, want, what):
    for name, a, b in zip(("qkv", "h_out", "k slab", "v slab", "attention output"), got, want):
        assert torch.equal(_bits(a), _bits(b)), (what, name, (_bits(a) != _bits(b)).nonzero()[:6].tolist())


@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("nH,nKV,d,H,T_old", [(8, 4, 64, 1024, 37), (8, 8, 128, 2048, 0), (32, 32, 128, 4096, 199), (32, 32, 128, 4096, 255), (40, 40, 128, 5120, 130)])
def test_bit_equal_to_the_bf16_fused_launch(nH, nKV, d, H, T_old, with_delta):
    """One pair per row with GQA and head dim 64; an empty cache; the product's shape; the trip boundary; five pairs per row (a pass of four and one of one).
    Six steps on one granule buffer, two call tags per step (no stale granule may be consumed), with and without delta."""
    c = _Case(nH, nKV, d, H, T_old)
    for step in range(6):
        h0, delta, lens, pos = c.step_inputs(step, with_delta)
        want = c.run(False, h0, delta, lens, pos, 100 + step)
        first = None
        for tag in (step, 200 + step):
            got = c.run(True, h0, delta, lens, pos, tag)
            _assert_same(got, want, (step, tag))
            if first is None:
                first = got
            else:
                _assert_same(got, first, (step, tag, "other tag"))
        if not with_delta:
            assert bool((want[1] == 5.0).all())  # h_out untouched without delta
        c.k0, c.v0 = want[2], want[3]  # the appended row stays for the next step
    assert int(c.err.item()) == 0


@pytest.mark.parametrize("T_old", [700, 100])
def test_several_attention_workgroups_per_head(T_old):
    """n_splits 2, 3, 4 (the MULTI instantiation) on the product's shape; T_old = 100 leaves the later attention workgroups of a head empty."""
    c = _Case(32, 32, 128, 4096, T_old, seed=12)
    for step in range(2):
        h0, delta, lens, pos = c.step_inputs(step)
        for ns in (2, 3, 4):
            want = c.run(False, h0, delta, lens, pos, 8 * ns + step, n_splits=ns)
            got = c.run(True, h0, delta, lens, pos, 64 + 8 * ns + step, n_splits=ns)
            _assert_same(got, want, (step, ns))
        c.k0, c.v0 = want[2], want[3]
    assert int(c.err.item()) == 0


@pytest.mark.parametrize("nH,nKV,d,H,T_old,grid_cap", [(8, 4, 64, 1024, 37, 47), (32, 32, 128, 4096, 199, 132), (40, 40, 128, 5120, 130, 113)])
def test_small_grid_runs_several_passes_and_a_ragged_last_one(nH, nKV, d, H, T_old, grid_cap):
    """grid_cap leaves 39 / 100 / 73 streaming workgroups: each runs many row groups (the prefetched header of the next group, clamped at N - 1) and the
    number of groups (N / 4 or N / 8 with one or two rows per wave) is no multiple of the workgroups, so the last pass is ragged."""
    c = _Case(nH, nKV, d, H, T_old, seed=13)
    n_gemv = grid_cap - nH
    assert (c.N // 4) % n_gemv != 0 and (c.N // 8) % n_gemv != 0 and c.N // 8 > 3 * n_gemv
    for step in range(2):
        h0, delta, lens, pos = c.step_inputs(step)
        want = c.run(False, h0, delta, lens, pos, step)
        got = c.run(True, h0, delta, lens, pos, 10 + step, grid_cap=grid_cap)
        _assert_same(got, want, step)
        c.k0, c.v0 = want[2], want[3]
    assert int(c.err.item()) == 0


def _clean_matrix(g, N, K):
    """Magnitudes in [0.004, 0.06] with random signs: four exponents, all inside any window pack() can choose -- the only escapes are the planted ones."""
    mag = 0.004 + 0.056 * torch.rand(N, K, device="cuda", generator=g)
    sign = torch.where(torch.rand(N, K, device="cuda", generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).to(BF)


def _from_bits(v):
    return torch.tensor([v - 65536 if v >= 32768 else v], dtype=torch.int16).view(BF).item()


@pytest.mark.parametrize("special", [False, True])
def test_planted_escapes(special):
    """+-0, a subnormal, the largest finite value and a tiny value outside the window, in row 0, row N - 1, a q row, a k row and a v row; in the first and
    the last span; in two spans of one row and in all spans of another (more than one flagged span in a pass: the dependent-load path).  special: Inf and
    NaN instead of the finite values; bits are compared all the same."""
    nH, nKV, d, K = 8, 4, 64, 4096
    N, nspan = (nH + 2 * nKV) * d, K // 512
    g = torch.Generator(device="cuda").manual_seed(14)
    W = _clean_matrix(g, N, K)
    big, tiny, sub = _from_bits(0x7F7F), 1.0e-30, 1.0e-40  # the largest finite bf16; far below the window; a bf16 subnormal
    if special:
        big, tiny = float("inf"), float("nan")
    q_row, k_row, v_row = 100, nH * d + 88, (nH + nKV) * d + 132
    plant = {}  # row -> span mask

    def put(row, col, val):
        W[row, col] = val
        plant[row] = plant.get(row, 0) | (1 << (col // 512))

    put(0, 0, 0.0)  # row 0, first span, first element
    put(N - 1, K - 1, big)  # the last element of the matrix: last span of the last row, the END of the pool
    put(q_row, 3 * 512 + 17, -0.0)
    put(k_row, 5, sub)  # two spans of one row: the first ...
    put(k_row, K - 9, tiny)  # ... and the last
    for s in range(nspan):  # every span of a v row
        put(v_row, 512 * s + 3 * s, -0.0 if s & 1 else big)
    put(v_row + 1, 512 + 1, -sub)  # two neighbouring spans
    put(v_row + 1, 1024 + 2, 0.0)
    c = _Case(nH, nKV, d, K, 37, seed=15, W=W)
    want_mask = torch.zeros(N, dtype=torch.int64)
    for r, mk in plant.items():
        want_mask[r] = mk
    got_mask = c.p.hdr[:, 0].cpu().to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got_mask, want_mask), (got_mask != want_mask).nonzero()[:8].tolist()
    assert c.p.n_pool == sum(bin(mk).count("1") for mk in plant.values())
    for step in range(2):
        h0, delta, lens, pos = c.step_inputs(step)
        want = c.run(False, h0, delta, lens, pos, step)
        got = c.run(True, h0, delta, lens, pos, 10 + step)
        _assert_same(got, want, step)
        got = c.run(True, h0, delta, lens, pos, 20 + step, n_splits=2, grid_cap=47)  # the same rows as a workgroup's later passes
        _assert_same(got[:4], c.run(False, h0, delta, lens, pos, 30 + step, n_splits=2)[:4], (step, "small grid"))
        c.k0, c.v0 = want[2], want[3]
    assert int(c.err.item()) == 0


def _tail_view(t):
    flat = t.reshape(-1)
    pad = 64 // flat.element_size()
    buf = torch.empty(pad + flat.numel(), dtype=flat.dtype, device="cuda")
    buf[pad:] = flat
    v = buf[pad:].view(t.shape)
    assert v.data_ptr() + v.numel() * v.element_size() == buf.data_ptr() + buf.numel() * buf.element_size()
    return v


def test_views_that_end_at_the_end_of_their_storage():
    """data / hdr / pool are views whose last byte is the last byte of their storage: the kernel needs no slack behind what pack() allocated."""
    nH, nKV, d, K = 8, 4, 64, 1024
    g = torch.Generator(device="cuda").manual_seed(16)
    W = _rnd(g, (nH + 2 * nKV) * d, K)
    W[-1, K - 1] = 0.0  # the last row's last span is read from the END of the pool
    c = _Case(nH, nKV, d, K, 37, seed=17, W=W)
    q = dataclasses.replace(c.p, data=_tail_view(c.p.data), hdr=_tail_view(c.p.hdr), pool=_tail_view(c.p.pool))
    h0, delta, lens, pos = c.step_inputs(0)
    want = c.run(False, h0, delta, lens, pos, 1)
    for ns, cap in ((1, 0), (2, 47)):
        _assert_same(c.run(True, h0, delta, lens, pos, 2 + ns, n_splits=ns, grid_cap=cap, p=q)[:4], want[:4], ns)
    _assert_same(c.run(True, h0, delta, lens, pos, 9, p=q), want, "one attention workgroup per head")
    assert int(c.err.item()) == 0


def _raw_call(c, p, K=None, h=None, dtype=None, n_splits=1, data_ptr=None, data_bytes=None, hdr_rows=None, pool_spans=None, hb=None):
    """The C entry point itself (the Python wrapper's own assertions are not what is tested): -> (return code, the buffers it may have written)."""
    K = c.H if K is None else K
    h = torch.ones(1, K, dtype=BF, device="cuda") if h is None else h
    k, v = c.k0.clone(), c.v0.clone()
    outs = [torch.full((1, c.N), 3.0, dtype=BF, device="cuda"), torch.full((1, K), 5.0, dtype=BF, device="cuda"), k, v, torch.full((1, c.nH * c.d), 7.0, dtype=BF, device="cuda")]
    P = ops._p
    lens = torch.tensor([c.T_old], dtype=torch.int32, device="cuda")
    nw = torch.ones(K, dtype=BF, device="cuda")
    rc = ops.lib().dl_gemv_qkv_attn_pk(
        P(p.data) if data_ptr is None else data_ptr, p.data.numel() if data_bytes is None else data_bytes, P(p.hdr), p.hdr.shape[0] if hdr_rows is None else hdr_rows,
        P(p.pool), p.pool.numel() // 1024 if pool_spans is None else pool_spans, int(p.hb) if hb is None else hb, K, P(h), P(outs[1]), P(h), P(nw), EPS, P(outs[0]),
        P(c.cos), P(c.sin), c.cos.shape[0], P(lens), P(lens), P(k), P(v), k.stride(0), k.stride(1), k.shape[2], P(outs[4]), P(c.gran), 1, P(c.err), n_splits, c.nH, c.nKV, c.d,
        ops.dtype_code(BF if dtype is None else dtype), 0, ops._stream())
    torch.cuda.synchronize()
    return rc, outs


def test_entry_point_refuses_bad_arguments():
    nH, nKV, d = 8, 4, 64
    c = _Case(nH, nKV, d, 1024, 37, seed=18)
    g = torch.Generator(device="cuda").manual_seed(19)
    untouched = lambda outs: bool((outs[0] == 3.0).all() and (outs[1] == 5.0).all() and (outs[4] == 7.0).all()) and torch.equal(outs[2], c.k0) and torch.equal(outs[3], c.v0)
    rc, outs = _raw_call(c, c.p)
    assert rc == 0 and not untouched(outs)  # the helper's argument list is right: the good call goes through
    p1536, p9216 = _pack(_rnd(g, c.N, 1536)), _pack(_rnd(g, c.N, 9216))
    shifted = torch.empty(c.p.data.numel() + 16, dtype=torch.uint8, device="cuda")
    shifted[8:8 + c.p.data.numel()] = c.p.data
    bad = {
        "K = 1536": dict(p=p1536, K=1536),
        "K = 9216": dict(p=p9216, K=9216),
        "hb = 121": dict(p=c.p, hb=121),
        "data_bytes one row short": dict(p=c.p, data_bytes=c.p.data.numel() - c.p.row_bytes),
        "hdr_rows = N - 1": dict(p=c.p, hdr_rows=c.N - 1),
        "pool_spans = 0": dict(p=c.p, pool_spans=0),
        "misaligned data": dict(p=c.p, data_ptr=shifted.data_ptr() + 8),
        "fp16": dict(p=c.p, dtype=torch.float16),
        "n_splits = 5": dict(p=c.p, n_splits=5),
    }
    for what, kw in bad.items():
        rc, outs = _raw_call(c, **kw)
        assert rc == -1, (what, rc)  # DL_ERR_ARG
        assert untouched(outs), what
        assert ops.lib().dl_last_error().decode().startswith("dl_gemv_qkv_attn_pk"), what
    assert int(c.err.item()) == 0
