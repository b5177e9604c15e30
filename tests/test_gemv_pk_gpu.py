"""GPU: dl_gemv_pk (batch-1 GEMV on losslessly packed 12-bit bf16 weights, bf16pack.py) must return dl_gemv's bits on the same weights and inputs --
every launch shape of the batch-1 decode step, escapes of every kind, and views that end exactly at the end of their storage."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import bf16pack as bp  # noqa: E402
from dynamic_llava_amd import hip_ops as ops  # noqa: E402

A, PAIR = ops.GEMV_ADDNORM, ops.GEMV_OUT_SILU_PAIR


def _bits(t):
    return t.view(torch.int16)


def _weights(N, K, seed):
    """N(0, 0.02) with planted zeros, subnormals, 1e4-scale values and escapes at the row ends (finite only)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn(N, K, generator=g, device="cuda") * 0.02).to(torch.bfloat16)
    w[0, 0] = 0.0
    w[0, K - 1] = 1.0e4
    w[1, 5] = -0.0
    w[2, K // 2] = 1.0e-40  # bf16 subnormal
    w[2, K // 2 + 1] = -3.0e-39
    w[3, 100:110] = 2.5e4
    w[N - 1, K - 8:] = -1.5e4  # last chunk of the last row
    w[N - 1, 0] = 1.0e-30
    w[N // 2] = 0.0  # a row of zeros: every span from the pool
    w[N // 2 + 1, ::512] = 7.0e3  # an escape in every span
    if K >= 2048:
        w[5, 512:1024] = 3.0e4  # two flagged spans next to each other ...
        w[5, 1030] = 0.0
    w[5, K - 3] = 0.0  # ... and one more at the row end
    if K % 512:
        w[6, K - (K % 512) + 3] = 0.0  # the ragged last span
    if K > 8192:
        hv = ((K // 8 + 1) // 2 + 63) // 64 * 64 * 8  # first element of the high half
        w[7, hv - 1] = 0.0
        w[8, hv] = 0.0
        w[9, hv - 512] = 9.0e3
        w[9, hv + 511] = 9.0e3
    return w


def _x(K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(1, K, generator=g, device="cuda").to(torch.bfloat16)


def _packed(w):
    p = bp.pack(w, force=True)
    assert torch.equal(_bits(bp.unpack(p)), _bits(w))
    assert p.n_pool >= 8  # the planted escapes are there
    return p


@pytest.mark.parametrize("N,K", [(70, 4096), (66, 5120), (34, 11008), (34, 13824), (37, 2112), (33, 8192)])
def test_plain_is_bit_equal_to_gemv(N, K):
    """x in registers (K <= 4096: two rows per wave, K <= 8192: one) and the halves kernel (K = 11008: 10.5 chunks per lane in the high half, odd span
    boundary between the halves; 13824); N not a multiple of the rows per workgroup; K = 2112: whole pairs + a ragged rest."""
    w, x = _weights(N, K, N + K), _x(K, 7)
    p = _packed(w)
    want = ops.gemv(w, torch.empty(1, N, dtype=torch.bfloat16, device="cuda"), x=x)
    got = ops.gemv_pk(p, torch.full((1, N), 3.0, dtype=torch.bfloat16, device="cuda"), x=x)
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all()
    assert torch.equal(_bits(got), _bits(want)), (N, K, (got != want).nonzero()[:8].tolist())


@pytest.mark.parametrize("N,K,with_delta,grid_cap", [(96, 4096, True, 0), (96, 4096, False, 0), (1000, 4096, True, 24), (1001, 5120, True, 16), (50, 1024, True, 0)])
def test_addnorm_is_bit_equal_to_gemv(N, K, with_delta, grid_cap):
    """add + rmsnorm prologue; [1000, 4096] on 24 workgroups: every workgroup takes several row groups (prefetched headers); K = 5120: a pass of four pairs
    and one of one; K = 1024: fewer pairs than are requested before the prologue."""
    w = _weights(N, K, N + K + 1)
    p = _packed(w)
    h = _x(K, 11)
    delta = _x(K, 12) if with_delta else None
    nw = (1.0 + 0.1 * _x(K, 13)).reshape(K).contiguous()
    outs = []
    for fn, wt in ((ops.gemv, w), (ops.gemv_pk, p)):
        y = torch.full((1, N), 3.0, dtype=torch.bfloat16, device="cuda")
        h_out = torch.full((1, K), 5.0, dtype=torch.bfloat16, device="cuda")
        fn(wt, y, mode=A, h_in=h, h_out=h_out, delta=delta, norm_w=nw, eps=1e-5, grid_cap=grid_cap)
        outs.append((y, h_out))
    torch.cuda.synchronize()
    (y0, ho0), (y1, ho1) = outs
    assert torch.isfinite(y0.float()).all()
    assert torch.equal(_bits(y1), _bits(y0)), (y1 != y0).nonzero()[:8].tolist()
    assert torch.equal(_bits(ho1), _bits(ho0))  # h_out (untouched without delta)
    if with_delta:
        assert torch.equal(ho1, (h.float() + delta.float()).to(torch.bfloat16))


@pytest.mark.parametrize("N,K,grid_cap", [(2 * 88, 4096, 0), (2 * 90, 5120, 0), (2 * 301, 4096, 8)])
def test_addnorm_silu_pair_is_bit_equal_to_gemv(N, K, grid_cap):
    w = _weights(N, K, N + K + 2)
    p = _packed(w)
    h, delta = _x(K, 21), _x(K, 22)
    nw = (1.0 + 0.1 * _x(K, 23)).reshape(K).contiguous()
    outs = []
    for fn, wt in ((ops.gemv, w), (ops.gemv_pk, p)):
        y = torch.full((1, N // 2), 3.0, dtype=torch.bfloat16, device="cuda")
        h_out = torch.empty((1, K), dtype=torch.bfloat16, device="cuda")
        fn(wt, y, mode=A | PAIR, h_in=h, h_out=h_out, delta=delta, norm_w=nw, eps=1e-5, grid_cap=grid_cap)
        outs.append((y, h_out))
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0][0].float()).all()
    assert torch.equal(_bits(outs[1][0]), _bits(outs[0][0])) and torch.equal(_bits(outs[1][1]), _bits(outs[0][1]))


def test_views_that_end_at_the_end_of_their_storage():
    """The kernel needs no slack behind what pack() allocated: data / hdr / pool are views whose last byte is the last byte of their storage, each storage an
    allocation of its own size class (a read past the end leaves the tensor's memory)."""
    import dataclasses

    for N, K, mode in ((70, 4096, 0), (34, 11008, 0), (96, 4096, A), (2 * 88, 4096, A | PAIR)):
        w = _weights(N, K, 99 + N)
        w[N - 1, K - 1] = 0.0  # the last row's last span is read from the END of the pool
        p = _packed(w)

        def tail_view(t):
            flat = t.reshape(-1)
            pad = 64 // flat.element_size()
            buf = torch.empty(pad + flat.numel(), dtype=flat.dtype, device="cuda")
            buf[pad:] = flat
            v = buf[pad:].view(t.shape)
            assert v.data_ptr() + v.numel() * v.element_size() == buf.data_ptr() + buf.numel() * buf.element_size()
            return v

        q = dataclasses.replace(p, data=tail_view(p.data), hdr=tail_view(p.hdr), pool=tail_view(p.pool))
        n_y = N // 2 if mode & PAIR else N
        y0 = torch.empty(1, n_y, dtype=torch.bfloat16, device="cuda")
        y1 = torch.empty(1, n_y, dtype=torch.bfloat16, device="cuda")
        if mode == 0:
            x = _x(K, 31)
            ops.gemv(w, y0, x=x)
            ops.gemv_pk(q, y1, x=x)
        else:
            h, delta, nw = _x(K, 32), _x(K, 33), (1.0 + 0.1 * _x(K, 34)).reshape(K).contiguous()
            ops.gemv(w, y0, mode=mode, h_in=h, h_out=torch.empty_like(h), delta=delta, norm_w=nw, eps=1e-5)
            ops.gemv_pk(q, y1, mode=mode, h_in=h, h_out=torch.empty_like(h), delta=delta, norm_w=nw, eps=1e-5)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y1), _bits(y0)), (N, K, mode)


def test_entry_point_refuses_bad_sizes():
    w = _weights(40, 4096, 5)
    p = _packed(w)
    x, y = _x(4096, 1), torch.empty(1, 40, dtype=torch.bfloat16, device="cuda")
    import dataclasses

    with pytest.raises(ops.HipOpsError):  # fewer packed bytes than N rows need
        ops.gemv_pk(dataclasses.replace(p, data=p.data[: p.data.numel() - 16]), y, x=x)
    with pytest.raises(ops.HipOpsError):  # fewer headers than rows
        ops.gemv_pk(dataclasses.replace(p, hdr=p.hdr[:39]), y, x=x)
    with pytest.raises(ops.HipOpsError):
        ops.gemv_pk(dataclasses.replace(p, hb=121), y, x=x)
    p2 = _packed(_weights(40, 2112, 6))
    h = _x(2112, 2)
    with pytest.raises(ops.HipOpsError):  # the ADDNORM prologue takes whole pairs only
        ops.gemv_pk(p2, y, mode=A, h_in=h, norm_w=h.reshape(-1))
    assert not ops.gemv_pk_ok(A, 2112, torch.bfloat16) and ops.gemv_pk_ok(0, 2112, torch.bfloat16) and not ops.gemv_pk_ok(0, 4096, torch.float16)
