"""The yardstick of tests/test_train_policy_gpu.py, checked without a GPU (oracle/train_truth.py; docs/train_policy_error_budget.md):

* the fp64 truth is the restated reference (oracle.ref_cpu.sdpa_with_policy) and its gradients with the row maximum held constant;
* a tiled fp32 emulation of the arithmetic train_policy.hip documents lies inside the derived per-element bound for every output, input,
  policy, dtype and both backward geometries;
* every mutant of that emulation -- bugs of the kind these kernels can have -- is outside the bound on a named input;
* a kernel without the eps / N leak terms passes the old criterion of tests/test_train_ops_gpu.py on N(0,1) inputs and fails the bound on
  `leak_rows`: why the per-element test exists;
* how far the gradient through max_j (which the kernels do not propagate) moves each gradient, as a ratio to the bound, per input.
"""
import itertools
import math

import pytest
import torch

from oracle import ref_cpu as O
from oracle import train_truth as tt

DTYPES = (torch.bfloat16, torch.float16)
LENGTHS = (1, 15, 17, 63, 64, 65, 127, 128, 129, 200)
KINDS = ("causal", "additive", "bool", "none", "soft", "batch1", "keypad", "leftpad")
COMBOS = list(itertools.product(tt.INPUTS, tt.POLICIES, DTYPES))


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _ratios(c, t, tol, mutant=None, bwd_keys=64):
    r = tt.worst_ratios(tt.emulate(c, mutant, bwd_keys=bwd_keys), t, tol, c.q.dtype)
    return {n: r[n][0] for n in tt.OUTPUTS}, r


@pytest.mark.parametrize("kind", ["causal", "soft", "keypad", "none"])
def test_truth_is_the_restated_reference(kind):
    c = tt.make_case("gauss", 2, 3, 70, 64, torch.bfloat16, kind, "pattern", seed=1)
    t = tt.truth(c)
    # forward: the closed form == ref64 == ref_cpu.sdpa_with_policy on fp64 operands (which exponentiates in fp32: agreement to fp32 rounding)
    bias = None if c.bias is None else c.bias.double()
    o_ref = O.sdpa_with_policy(c.q.double(), c.k.double(), c.v.double(), attn_mask=bias, is_causal=c.causal, policy=c.policy.double()[:, :, None])
    assert float((t.out - o_ref.double()).abs().max()) <= 1e-5 * float(t.out.abs().max())
    # gradients, max as a constant: the header's formulas == fp64 autograd with the maximum detached, to rounding
    const = tt.autograd_grads(c, detach_max=True)
    for n in tt.OUTPUTS:
        assert float((const[n] - getattr(t, n)).abs().max()) <= 1e-11 * float(getattr(t, n).abs().max()), n
    # second set: fp64 autograd of ref64 == autograd of the restated reference itself (fp32 inside), to fp32 rounding
    full = tt.autograd_grads(c)
    q, k, v, pol = (x.double().clone().requires_grad_(True) for x in (c.q, c.k, c.v, c.policy))
    O.sdpa_with_policy(q, k, v, attn_mask=bias, is_causal=c.causal, policy=pol[:, :, None]).backward(c.do.double())
    for n, g in zip(tt.OUTPUTS[1:], (q.grad, k.grad, v.grad, pol.grad)):
        assert float((full[n] - g).abs().max()) <= 2e-5 * float(g.abs().max()), n


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", tt.INPUTS)
def test_inputs_have_their_property(name, dtype):
    c = tt.make_case(name, 2, 2, 200, 64, dtype, "causal", "pattern")
    print(name, _name(dtype), tt.check_property(c))


@pytest.mark.parametrize("idx", range(len(COMBOS)), ids=[f"{n}-{p}-{_name(d)}" for n, p, d in COMBOS])
def test_emulation_is_inside_the_bound(idx):
    name, policy, dtype = COMBOS[idx]
    L, d, kind = LENGTHS[(3 * idx + idx // 10) % len(LENGTHS)], (64, 128)[(idx // 2) % 2], KINDS[(5 * idx + idx // 8) % len(KINDS)]
    c = tt.make_case(name, 2, 2, L, d, dtype, kind, policy, seed=idx, n_eps=2 * L if idx % 7 == 3 else 0)
    t = tt.truth(c)
    tol = tt.bound(t, c)
    for bk in (64, 128):
        worst, full = _ratios(c, t, tol, bwd_keys=bk)
        print(f"{name} {policy} {_name(dtype)} L={L} d={d} {kind} keys/wg={bk}: {tt.format_ratios(full)}")
        assert max(worst.values()) < 1.0, (bk, worst)


@pytest.mark.parametrize("policy", tt.POLICIES)
@pytest.mark.parametrize("name", tt.INPUTS)
def test_emulation_is_inside_the_bound_at_every_length(name, policy):
    """Every input x policy at every length; head_dim, dtype, mask form and backward geometry alternate along the lengths, shifted per
    (input, policy) so that each length meets both dtypes, both head dims and all eight mask forms across the table."""
    shift = tt.INPUTS.index(name) * len(tt.POLICIES) + tt.POLICIES.index(policy)
    for i, L in enumerate(LENGTHS):
        j = i + shift
        d, dtype, kind, bk = (64, 128)[j % 2], DTYPES[(j // 2) % 2], KINDS[j % len(KINDS)], (64, 128)[(j // 4) % 2]
        c = tt.make_case(name, 2, 2, L, d, dtype, kind, policy, seed=L + shift)
        t = tt.truth(c)
        worst, full = _ratios(c, t, tt.bound(t, c), bwd_keys=bk)
        print(f"{name} {policy} {_name(dtype)} L={L} d={d} {kind} keys/wg={bk}: {tt.format_ratios(full)}")
        assert max(worst.values()) < 1.0, (L, d, _name(dtype), kind, worst)


# mutant -> (input, mask kind, backward geometry, outputs of which at least one must leave the bound)
MUTANT_CASES = {
    "leak_dropped": ("leak_rows", "causal", 64, ("out", "dv")),
    "self_first_tile_only": ("gauss", "causal", 64, ("out",)),
    "dpolicy_with_diagonal": ("gauss", "causal", 64, ("dpolicy",)),
    "policy_one_late_last_tile": ("gauss", "additive", 64, ("out", "dpolicy")),
    "causal_skip_one_wave": ("gauss", "causal", 64, ("out", "dk")),
    "first_qtile_one_late_128": ("late_peak", "causal", 128, ("dk", "dv", "dpolicy")),
    "stats_from_head0": ("late_peak", "causal", 64, ("dq", "dk", "dv")),
    "bias_row_stride_ignored": ("gauss", "soft", 64, ("out",)),
    "l_not_rescaled": ("late_peak", "causal", 64, ("out",)),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mutant", tt.MUTANTS)
def test_every_mutant_is_outside_the_bound(mutant, dtype):
    name, kind, bk, outs = MUTANT_CASES[mutant]
    c = tt.make_case(name, 2, 2, 150, 64, dtype, kind, "pattern")
    t = tt.truth(c)
    tol = tt.bound(t, c)
    base, _ = _ratios(c, t, tol, bwd_keys=bk)
    worst, full = _ratios(c, t, tol, mutant, bk)
    print(f"{mutant} on {name} ({kind}, {bk} keys per workgroup, {_name(dtype)}): {tt.format_ratios(full)}")
    assert max(base.values()) < 1.0
    assert max(worst[n] for n in outs) > 1.0, worst


def _old_criterion(c, got):
    """tests/test_train_ops_gpu.py before the per-element bound: max|got - fp32 truth| <= 2 max|eager dtype oracle - truth| + 1e-3 max|truth|."""
    def oracle(dtype):
        q, k, v, pol = (x.detach().to(dtype).clone().requires_grad_(True) for x in (c.q, c.k, c.v, c.policy[:, :, None]))
        o = O.sdpa_with_policy(q, k, v, is_causal=True, policy=pol)
        o.backward(c.do.to(dtype))
        return [x.detach().float() for x in (o, q.grad, k.grad, v.grad, pol.grad[:, :, 0])]
    truth, noisy = oracle(torch.float32), oracle(c.q.dtype)
    res = {}
    for n, t, nz in zip(tt.OUTPUTS, truth, noisy):
        err, ref_err, mag = float((got[n].float() - t).abs().max()), float((nz - t).abs().max()), float(t.abs().max())
        res[n] = (err, 2 * ref_err + 1e-3 * mag)
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_leak_mutant_passes_the_old_criterion_and_fails_the_bound(dtype):
    """B=2, H=2, L=131, d=64, causal, the old test's policy: without both eps / N terms the old criterion still holds on N(0,1) inputs (every
    row has Dn >= 1: the leak is ~1e-8 of the row); on `leak_rows`, at the same shape, the per-element bound catches it in out and dv."""
    c = tt.make_case("gauss", 2, 2, 131, 64, dtype, "causal", "pattern")
    mut = tt.emulate(c, "leak_dropped")
    for n, (err, bar) in _old_criterion(c, mut).items():
        print(f"gauss, leak dropped, old criterion: {n} err {err:.3e} <= {bar:.3e}")
        assert err <= bar, n
    ok = tt.emulate(c)
    moved = {n: float((mut[n].double() - ok[n].double()).abs().max()) for n in ("out", "dv")}
    print("gauss: dropping the leak moves", moved)
    c = tt.make_case("leak_rows", 2, 2, 131, 64, dtype, "causal", "pattern")
    t = tt.truth(c)
    tol = tt.bound(t, c)
    worst, full = _ratios(c, t, tol, "leak_dropped")
    print(f"leak_rows ({tt.check_property(c, t)}), leak dropped: {tt.format_ratios(full)}")
    assert worst["out"] > 1.0 and worst["dv"] > 1.0
    assert max(_ratios(c, t, tol)[0].values()) < 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("name", tt.INPUTS)
def test_gradient_through_the_row_maximum(name, dtype):
    """|full autograd - max-as-constant gradients| / bound, per input (B=2, H=2, L=131, d=64, causal).  Below 1 where every row's maximum is
    a kept key or its own (Dn_i >= 1: the term is O(eps)); recorded where dropped keys lead rows (O(eps / Dn_i))."""
    c = tt.make_case(name, 2, 2, 131, 64, dtype, "causal", "pattern")
    t = tt.truth(c)
    tol = tt.bound(t, c)
    full = tt.autograd_grads(c)
    ratio = {n: float(((full[n] - getattr(t, n)).abs() / tol[n].clamp_min(1e-300)).max()) for n in tt.OUTPUTS}
    absd = {n: float((full[n] - getattr(t, n)).abs().max()) for n in tt.OUTPUTS}
    print(f"max-gradient deviation {name} {_name(dtype)} (min Dn {float(t.Dn.min()):.3e}): " + "; ".join(f"{n} {ratio[n]:.3g} (abs {absd[n]:.3g})" for n in tt.OUTPUTS[1:]))
    assert ratio["out"] == 0.0 and absd["dv"] <= 1e-12 * float(t.dv.abs().max())  # the forward and dV do not depend on it
    if name in tt.MAXGRAD_BELOW_BOUND:
        assert max(ratio.values()) < 1.0, ratio


def test_gumbel_truth_flags_what_the_roundings_can_flip():
    for dtype in (torch.float32,) + DTYPES:
        lp, g, prev, dk = tt.gumbel_inputs(257, dtype)
        t = tt.gumbel_truth(lp, g, prev, dk, 0.7)
        ties = torch.arange(257) % 8 == 1
        assert not bool(t["determined"][ties].any()) and bool(t["dec0"][ties].all())
        assert float(t["determined"].float().mean()) > 0.6
        assert bool(torch.isfinite(t["dlogp"]).all()) and int((prev == 0).sum()) > 0
        # the eager expression in the dtype agrees wherever the decision is determined
        keep = O.gumbel_hard_keep(lp[None], g[None], 0.7, prev[None, :, None])[0, :, 0]
        dec = keep.float() > 0.5
        sel = t["determined"] & (prev.float() != 0)
        assert torch.equal(dec[sel], t["dec0"][sel])
