"""GPU: dl_gemv_pk on long rows (plain prologue, 8192 < K <= 16384: x staged in LDS as two zero-padded segment images, a row shared by a wave pair, a
runtime loop of passes) must return dl_gemv's bits on the unpacked matrix: every tail shape of the two segments, escapes in every position of a pass,
workgroups that run many passes, the sign of zero, views that end with their storage, and refused sizes."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import bf16pack as bp  # noqa: E402
from dynamic_llava_amd import hip_ops as ops  # noqa: E402

# 8256: the smallest long row (low half 9 spans, high half 7 spans + 8 chunks); 11008: a one-span tail low, half a span high; 13824: 14 spans low (whole
# pairs + padding), 13 high; 16384: whole pairs only, the largest LDS image, no padded chunk at all
KS = [8256, 11008, 13824, 16384]


def _bits(t):
    return t.view(torch.int16)


def _segments(K):
    """[(first element, one past the last element)] of the two halves of a row."""
    nvec = K // 8
    hv = ((nvec + 1) // 2 + 63) // 64 * 64
    assert bp.segments(K) == [(0, hv), (hv, nvec - hv)]
    return [(0, hv * 8), (hv * 8, K)]


def _weights(N, K, seed):
    """N(0, 0.02) with planted escapes (0.0 and the 1e4-scale values lie outside every window that holds N(0, 0.02)); needs N >= 24."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(N, K, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    (l0, l1), (h0, h1) = _segments(K)
    w[0, 0] = 0.0
    w[0, 17] = 1.0e4
    w[0, 18] = -1.0e4
    w[1, 5] = -0.0
    w[2, K // 3] = 1.0e-40  # bf16 subnormals
    w[2, K // 3 + 1] = -3.0e-39
    w[N - 1, K - 8:] = -1.5e4  # the last chunk of the last row
    w[N // 2] = 0.0  # a row of zeros: every span from the pool
    w[N // 2 + 1, ::512] = 7.0e3  # an escape in every span
    # spans 0 and 1 of a segment are in its first pass whatever the pass length; 6, 7 and 12 begin later passes where the segment is that long
    for row, (s0, s1) in ((3, (l0, l1)), (4, (h0, h1))):
        for span in (0, 1, 6, 7, 12):
            e = s0 + span * 512 + 37 * (span + 1)
            if e < s1:
                w[row, e] = 0.0
    w[5, 0:1024] = 3.0e4  # two flagged spans next to each other, raw in every lane ...
    w[5, 6 * 512 + 9] = 0.0  # ... and one in the next pass
    w[6, l1 - 1] = 0.0  # the last element of the low half: its tail slot
    w[7, h0] = 0.0  # the first element of the high half
    w[8, K - 1] = 0.0  # the high half's tail slot (a partial span unless K % 512 == 0)
    w[9, l1 - 1] = 2.0e4  # both tails and both heads in one row
    w[9, h0] = 2.0e4
    w[9, K - 1] = 2.0e4
    w[9, 0] = 2.0e4
    w[10, l1 - 512] = 0.0  # the first element of the low half's last span
    w[11, (K - 1) // 512 * 512] = 0.0  # ... and of the high half's
    return w


def _x(K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(1, K, generator=g, device="cuda").to(torch.bfloat16)


def _packed(w):
    p = bp.pack(w, force=True)
    assert torch.equal(_bits(bp.unpack(p)), _bits(w))
    assert p.n_pool >= 24  # the planted escapes are there
    return p


_CACHE = {}


def _case(N, K):
    """(w, packed, x, dl_gemv's result): built once per shape and left unchanged."""
    if (N, K) not in _CACHE:
        w, x = _weights(N, K, N + K), _x(K, 7)
        want = ops.gemv(w, torch.empty(1, N, dtype=torch.bfloat16, device="cuda"), x=x)
        torch.cuda.synchronize()
        assert torch.isfinite(want.float()).all()
        _CACHE[(N, K)] = (w, _packed(w), x, want)
    return _CACHE[(N, K)]


@pytest.mark.parametrize("K", KS)
def test_long_rows_are_bit_equal_to_gemv(K):
    """N = 41 at the default cap: one pass per workgroup, the last workgroup with rows past N."""
    N = 41
    w, p, x, want = _case(N, K)
    got = ops.gemv_pk(p, torch.full((1, N), 3.0, dtype=torch.bfloat16, device="cuda"), x=x)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)), (K, (_bits(got) != _bits(want)).nonzero()[:8].tolist())


@pytest.mark.parametrize("K", KS)
def test_long_rows_on_three_workgroups(K):
    """N = 203 on a grid of at most three workgroups: every workgroup runs many passes (prefetched headers, LDS image reused) and a ragged last one whose
    rows past N are clamped duplicates."""
    N = 203
    w, p, x, want = _case(N, K)
    got = ops.gemv_pk(p, torch.full((1, N), 3.0, dtype=torch.bfloat16, device="cuda"), x=x, grid_cap=3)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)), (K, (_bits(got) != _bits(want)).nonzero()[:8].tolist())


@pytest.mark.parametrize("K", KS)
def test_sign_of_zero(K):
    """Rows of +0 weights against an all-negative x: every product is -0, and whatever dl_gemv's padded chunks and its fixed order of additions make of
    the sign is what the packed kernel must return (next to ordinary rows)."""
    N = 41
    w = _case(N, K)[0].clone()
    w[N // 2] = 0.0
    w[12] = 0.0
    w[N - 1] = 0.0
    assert (_bits(w[12]) == 0).all()
    x = (-(_x(K, 9).float().abs() + 0.125)).to(torch.bfloat16)
    assert (x < 0).all()
    p = _packed(w)
    want = ops.gemv(w, torch.full((1, N), 3.0, dtype=torch.bfloat16, device="cuda"), x=x)
    got = ops.gemv_pk(p, torch.full((1, N), 3.0, dtype=torch.bfloat16, device="cuda"), x=x)
    torch.cuda.synchronize()
    assert (want[0, [12, N // 2, N - 1]] == 0).all()
    assert torch.equal(_bits(got), _bits(want)), (K, _bits(got)[0, [12, N // 2, N - 1]].tolist(), _bits(want)[0, [12, N // 2, N - 1]].tolist())


def test_views_that_end_at_the_end_of_their_storage():
    """data / hdr / pool / x are views whose last byte is the last byte of their storage (a read past the end leaves the tensor's memory)."""

    def tail_view(t):
        flat = t.reshape(-1)
        pad = 64 // flat.element_size()
        buf = torch.empty(pad + flat.numel(), dtype=flat.dtype, device="cuda")
        buf[pad:] = flat
        v = buf[pad:].view(t.shape)
        assert v.data_ptr() + v.numel() * v.element_size() == buf.data_ptr() + buf.numel() * buf.element_size()
        return v

    for K in (8256, 11008):
        N = 41
        w, p, x, _ = _case(N, K)
        w = w.clone()
        w[N - 1, K - 1] = 0.0  # the last row's last span is read from the END of the pool
        p = _packed(w)
        q = dataclasses.replace(p, data=tail_view(p.data), hdr=tail_view(p.hdr), pool=tail_view(p.pool))
        xv = tail_view(x)
        y0 = ops.gemv(w, torch.empty(1, N, dtype=torch.bfloat16, device="cuda"), x=x)
        y1 = ops.gemv_pk(q, torch.empty(1, N, dtype=torch.bfloat16, device="cuda"), x=xv)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y1), _bits(y0)), K


def test_entry_point_refuses_bad_sizes():
    """DL_ERR_ARG (rc = -1) and no launch: y keeps its fill."""
    N, K = 41, 11008
    w, p, x, _ = _case(N, K)
    y = torch.full((1, N), 3.0, dtype=torch.bfloat16, device="cuda")

    def refused(q, xx, **kw):
        with pytest.raises(ops.HipOpsError, match=r"rc=-1"):
            ops.gemv_pk(q, y, x=xx, **kw)

    refused(dataclasses.replace(p, data=p.data[: p.data.numel() - 16]), x)  # fewer packed bytes than N rows need
    refused(dataclasses.replace(p, hdr=p.hdr[: N - 1]), x)  # fewer headers than rows
    refused(dataclasses.replace(p, hb=121), x)
    refused(dataclasses.replace(p, K=16448), torch.zeros(1, 16448, dtype=torch.bfloat16, device="cuda"))  # K > 16384
    refused(dataclasses.replace(p, K=11000), x)  # K % 64 != 0
    refused(p, torch.zeros(1, K + 8, dtype=torch.bfloat16, device="cuda")[:, 4:])  # x not 16-byte aligned
    refused(p, x, grid_cap=-1)
    torch.cuda.synchronize()
    assert (y == 3.0).all()
