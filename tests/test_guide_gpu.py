"""GPU: dl_logits_guide and dl_pair_follow (through ops.logits_guide / ops.pair_follow) against the rule in dynamic_llava_amd/guidance.py, bit for bit.

What is compared.  Kernel and rule read the same logits; maxima, subtractions, the three operations of step 2, the threshold and the -inf cases are the same fp32
operations in both.  The one thing the CPU cannot reproduce is the device's expf / logf inside lse (the situation of dl_decode_logprobs, tests/test_logprobs_gpu.py),
so the rule is evaluated with the two lse values that dl_decode_logprobs reports for the same rows on the device -- "the same bits output_logprobs reports" -- and
then every element must be torch.equal.  The rule evaluated entirely on the CPU is compared too: it may differ only through lse, by at most
s * (e_c + e_u) + e_u plus one ulp of each of the five roundings that follow, e = score_cases.device_tol's lse term, and never in which entries are -inf away from the
cutoff threshold."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import guidance as G  # noqa: E402

SENT = -12345.0
GUARD = 64
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _logits(V, dtype, P, seed, pad=0):
    """[2 P, V] logits in `dtype` (row stride V + pad): rows [:P] conditional, rows [P:] a re-noised, shifted copy (the negative rows)."""
    g = torch.Generator().manual_seed(seed * 7919 + V)
    c = torch.randn((P, V), generator=g) * 4.0
    u = 0.7 * c + torch.randn((P, V), generator=g) * 2.0
    x = torch.cat([c, u]).to(dtype)
    if pad:
        big = torch.full((2 * P, V + pad), 99.0, dtype=dtype)  # (the padding holds a value that would change every maximum if it were read)
        big[:, :V] = x
        return big.cuda()[:, :V]
    return x.cuda()


def _device_lse(xd):
    """lse of every row as dl_decode_logprobs reports it: -top_logprobs[.., 0] (entry 0 is the maximum: -((m - m) + lse))."""
    from dynamic_llava_amd import hip_ops as ops

    R = xd.shape[0]
    lp = torch.zeros((R, 1), dtype=torch.float32, device="cuda")
    top_lp, top_ids = torch.zeros((R, 1, 1), dtype=torch.float32, device="cuda"), torch.zeros((R, 1, 1), dtype=torch.int64, device="cuda")
    ops.decode_logprobs(xd, torch.zeros(R, dtype=torch.int64, device="cuda"), torch.ones(R, dtype=torch.int32, device="cuda"), lp, 1, top_lp, top_ids)
    return (-top_lp[:, 0, 0]).cpu()


def _run(xd, scale, cutoff, params=None):
    """One launch into a guard-banded buffer -> (out [2 P, V] on the CPU, guards intact, logits unchanged)."""
    from dynamic_llava_amd import hip_ops as ops

    R, V = xd.shape
    before = xd.clone()
    buf = torch.full((R * V + 2 * GUARD,), SENT, dtype=torch.float32, device="cuda")
    out = buf[GUARD : GUARD + R * V].view(R, V)
    if params is None:
        params = ops.guide_params_block("cuda")
        params.copy_(ops.guide_params_words(scale, cutoff))
    ops.logits_guide(xd, out, params)
    torch.cuda.synchronize()
    ok = bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + R * V :] == SENT).all()) and torch.equal(before.view(torch.int16 if xd.element_size() == 2 else torch.int32), xd.view(torch.int16 if xd.element_size() == 2 else torch.int32))
    return out.cpu(), ok


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(xd, scale, cutoff, tag):
    """The kernel on xd against the rule: exact with the device's lse; the all-CPU rule within the lse tolerance."""
    import score_cases as cs

    P, V = xd.shape[0] // 2, xd.shape[1]
    out, ok = _run(xd, scale, cutoff)
    assert ok, (tag, "guard band or logits touched")
    assert torch.equal(_bits(out[:P]), _bits(out[P:])), (tag, "the rows of a pair differ")
    x, lse = xd.float().cpu(), _device_lse(xd)
    n_diff = 0
    for p in range(P):
        ref = G.guide_row(x[p], x[P + p], scale, cutoff, lse=(lse[p], lse[P + p]))
        assert torch.equal(_bits(out[p]), _bits(ref)), (tag, p, int((_bits(out[p]) != _bits(ref)).sum()))
        cpu = G.guide_row(x[p], x[P + p], scale, cutoff)
        lc_ref, lse_c = G.row_logprobs(x[p])
        lu_ref, lse_u = G.row_logprobs(x[P + p])
        e_c, e_u = (cs.device_tol(V, float(l), 0.0) for l in (lse_c, lse_u))  # (the lse terms of the bound; the logprob's own ulp is added below)
        both = torch.isfinite(out[p]) & torch.isfinite(cpu)
        ulp = lambda t: torch.ldexp(torch.ones_like(t), torch.frexp(t.abs().clamp_min(1e-30))[1] - 24)
        tol = scale * (e_c + e_u) + e_u + 2 * ((scale + 1) * (ulp(lc_ref) + ulp(lu_ref)) + ulp(cpu.nan_to_num(neginf=0.0)) + scale * ulp((lc_ref - lu_ref).nan_to_num(nan=0.0, posinf=0.0, neginf=0.0)))
        assert bool(((out[p] - cpu).abs()[both] <= tol[both]).all()), (tag, p, float(((out[p] - cpu).abs()[both] / tol[both]).max()))
        flipped = torch.isfinite(out[p]) != torch.isfinite(cpu)
        if cutoff is None:
            assert not bool(flipped.any()), (tag, p)
        else:  # an entry may change sides of the cutoff only where its log-probability sits on the threshold
            thr = (-lse_c) + torch.tensor(G.log_beta(cutoff), dtype=torch.float32)
            assert bool(((lc_ref - thr).abs()[flipped] <= e_c + 2 * ulp(lc_ref)[flipped]).all()), (tag, p)
        n_diff += int((_bits(out[p]) != _bits(cpu)).sum())
    return n_diff


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", [1, 7, 8, 2049, 32000, 32776, 65536])
def test_kernel_matches_the_rule(V, dtype):
    """Scalar tail, one chunk, both register branches and the cap; 1 and 3 pairs; s = 0, the cutoff on and off."""
    total = 0
    for P in (1, 3):
        xd = _logits(V, dtype, P, seed=P)
        for scale, cutoff in ((1.5, None), (0.0, None), (3.0, 0.1)):
            total += _check(xd, scale, cutoff, (V, dtype, P, scale, cutoff))
    print(f"V={V} {dtype}: elements whose bits differ from the all-CPU rule (device expf / logf in lse): {total}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_padded_stride_minus_inf_and_a_tied_maximum(dtype):
    V, P = 2049, 3
    xd = _logits(V, dtype, P, seed=11, pad=24)
    assert xd.stride(0) == V + 24
    _check(xd, 2.0, 0.05, ("stride", dtype))
    x = _logits(V, dtype, P, seed=12).clone()
    x[0, 5], x[P + 0, 9], x[1, 77], x[P + 1, 77] = float("-inf"), float("-inf"), float("-inf"), float("-inf")
    x[2, 100] = x[2].max()  # the maximum twice in a conditional row
    x[2, 2000] = x[2, 100]
    x[P + 2, 2000] = x[P + 2, 100]  # (the same negative logit under both: their guided scores are then the same bits)
    x[P + 1, 3] = x[P + 1].float().max().to(dtype)
    x[P + 1, 4] = x[P + 1, 3]
    for scale, cutoff in ((1.5, None), (0.0, None), (3.0, 0.2)):
        _check(x, scale, cutoff, ("inf/ties", dtype, scale, cutoff))
        out, _ = _run(x, scale, cutoff)
        assert torch.isneginf(out[0, 5]) and torch.isneginf(out[0, 9]) and torch.isneginf(out[1, 77]) and not torch.isnan(out).any()
        assert torch.isfinite(out[2, 100]) and torch.equal(_bits(out[2, 100]), _bits(out[2, 2000]))  # the conditional argmax survives; tied entries share their bits


def test_eager_and_captured_graph_with_another_parameter_block_agree():
    from dynamic_llava_amd import hip_ops as ops

    V, P = 32000, 2
    xd = _logits(V, torch.bfloat16, P, seed=21)
    params = ops.guide_params_block("cuda")
    params.copy_(ops.guide_params_words(1.5, None))
    out = torch.full((2 * P, V), SENT, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.logits_guide(xd, out, params)  # warm-up
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.logits_guide(xd, out, params)
    for scale, cutoff in ((1.5, None), (3.0, 0.1), (0.0, 0.5)):
        params.copy_(ops.guide_params_words(scale, cutoff))  # another setting: device data, the same graph
        out.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        eager, ok = _run(xd, scale, cutoff)
        assert ok and torch.equal(_bits(out.cpu()), _bits(eager)), (scale, cutoff)


def test_argument_checks():
    from dynamic_llava_amd import hip_ops as ops

    lib = ops.lib()
    x = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    out, prm = torch.zeros((2, 8), dtype=torch.float32, device="cuda"), ops.guide_params_block("cuda")
    p = lambda t: t.data_ptr()
    ok = dict(logits=p(x), dt=ops.dtype_code(torch.float32), stride=8, V=8, n=1, out=p(out), prm=p(prm))
    for bad in (dict(logits=None), dict(out=None), dict(prm=None), dict(n=0), dict(V=0), dict(V=65537, stride=65537), dict(stride=7), dict(out=p(x)), dict(dt=99)):
        a = dict(ok, **bad)
        assert lib.dl_logits_guide(a["logits"], a["dt"], a["stride"], a["V"], a["n"], a["out"], a["prm"], None) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 0).all())


def test_pair_follow_moves_exactly_three_fields():
    from dynamic_llava_amd import hip_ops as ops

    P, CAP = 3, 4
    g = torch.Generator().manual_seed(5)
    for steps in ([1, 2, 4], [0, 5, 3], [4, 4, 0]):  # a step of 0 (nothing committed) and one past out_cap write no slot
        nxt = torch.randint(0, 1000, (2 * P,), generator=g)
        out_ids = torch.randint(0, 1000, (2 * P, CAP), generator=g)
        step = torch.tensor(steps + [7, 0, 2], dtype=torch.int32)  # (the negative rows' own counters are never read)
        fin = torch.tensor([1, 0, 1, 0, 1, 0], dtype=torch.int32)
        lens = torch.randint(0, 50, (2, 2 * P), generator=g).to(torch.int32)
        pad = 8
        buf = torch.full((2 * P * CAP + 2 * pad,), -7, dtype=torch.int64)
        buf[pad : pad + 2 * P * CAP] = out_ids.reshape(-1)
        d = dict(nxt=nxt.cuda(), buf=buf.cuda(), step=step.cuda(), fin=fin.cuda(), lens=lens.cuda())
        view = d["buf"][pad : pad + 2 * P * CAP].view(2 * P, CAP)
        ops.pair_follow(d["nxt"], view, d["step"], d["fin"])
        torch.cuda.synchronize()
        want_nxt, want_out, want_fin = nxt.clone(), out_ids.clone(), fin.clone()
        want_nxt[P:], want_fin[P:] = nxt[:P], fin[:P]
        for b, s in enumerate(steps):
            if 0 <= s - 1 < CAP:
                want_out[P + b, s - 1] = out_ids[b, s - 1]
        assert torch.equal(d["nxt"].cpu(), want_nxt) and torch.equal(view.cpu(), want_out) and torch.equal(d["fin"].cpu(), want_fin)
        assert torch.equal(d["step"].cpu(), step) and torch.equal(d["lens"].cpu(), lens)  # the counters and the KV lengths stay each row's own
        got = d["buf"].cpu()
        assert bool((got[:pad] == -7).all()) and bool((got[pad + 2 * P * CAP :] == -7).all())
    lib = ops.lib()
    assert lib.dl_pair_follow(0, d["nxt"].data_ptr(), view.data_ptr(), CAP, d["step"].data_ptr(), d["fin"].data_ptr(), None) == -1
    assert lib.dl_pair_follow(P, None, view.data_ptr(), CAP, d["step"].data_ptr(), d["fin"].data_ptr(), None) == -1
    assert lib.dl_pair_follow(P, d["nxt"].data_ptr(), view.data_ptr(), 0, d["step"].data_ptr(), d["fin"].data_ptr(), None) == -1
