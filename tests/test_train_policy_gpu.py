"""csrc/train_policy.hip on the GPU, per element: the policy attention forward and its two-pass backward (every entry of
oracle/train_cases.py: length edges, mask and bias forms, layouts, both backward geometries) and the Gumbel hard keep forward and backward,
against the fp64 truth of oracle/train_truth.py under its derived bounds (docs/train_policy_error_budget.md).  The yardstick itself is
checked without a GPU in tests/test_train_truth_cpu.py."""
import pytest
import torch

from oracle import train_cases as tc
from oracle import train_truth as tt

pytestmark = pytest.mark.gpu


def _name(dtype):
    return str(dtype).replace("torch.", "")


@pytest.mark.parametrize("dtype", tc.DTYPES, ids=_name)
@pytest.mark.parametrize("entry", tc.TABLE, ids=lambda e: e.id)
def test_policy_attention_entry(entry, dtype):
    from dynamic_llava_amd import hip_ops as ops
    from dynamic_llava_amd.train_ops import scaled_dot_product_attention_with_policy as sdpa

    res = tc.run_entry(ops, sdpa, entry, dtype)
    print(f"{entry.id} {_name(dtype)}: {tt.format_ratios(res)}")
    bad = {n: r for n, r in res.items() if not r[0] < 1.0}
    assert not bad, f"{entry.id} {_name(dtype)}: outside the per-element bound: {tt.format_ratios(bad)}"


def test_both_backward_forms_are_driven():
    """The table reaches the 4-wave and the 8-wave backward at head_dim 128; head_dim 64 only ever yields 4 (also far above the threshold)."""
    from dynamic_llava_amd import hip_ops as ops

    seen = {64: set(), 128: set()}
    for e in tc.TABLE:
        w = ops.attn_policy_bwd_waves(e.B, e.H, e.L, e.d)
        assert w == e.waves, e.id
        seen[e.d].add(w)
    assert seen[128] == {4, 8} and seen[64] == {4}
    assert ops.attn_policy_bwd_waves(2, 64, 130, 64) == 4 and ops.attn_policy_bwd_waves(8, 32, 2048, 64) == 4
    # the threshold itself: B * H * ceil(L / 128) >= 256
    assert ops.attn_policy_bwd_waves(2, 64, 128, 128) == 4 and ops.attn_policy_bwd_waves(2, 64, 129, 128) == 8 and ops.attn_policy_bwd_waves(1, 85, 257, 128) == 4
    assert ops.attn_policy_bwd_waves(1, 1, 16, 32) == 0  # a shape the launch refuses


GUMBEL_N = (1, 255, 256, 257, 3 * 576)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=_name)
@pytest.mark.parametrize("tau", [0.1, 0.7, 1.0, 5.0])
def test_gumbel_hard_keep_per_element(tau, dtype):
    from dynamic_llava_amd.train_ops import gumbel_hard_keep

    U = tt.ULP[dtype]
    for n in GUMBEL_N:
        lp, g, prev, dk = tt.gumbel_inputs(n, dtype)
        t = tt.gumbel_truth(lp, g, prev, dk, tau)
        runs = []
        for _ in range(2):
            lpd, pd = lp[None].cuda().requires_grad_(True), prev[None, :, None].cuda().requires_grad_(True)
            keep = gumbel_hard_keep(lpd, tau, pd, gumbels=g[None].cuda())
            keep.backward(dk[None, :, None].cuda())
            torch.cuda.synchronize()
            runs.append((keep.detach().cpu()[0, :, 0], lpd.grad.cpu()[0], pd.grad.cpu()[0, :, 0]))
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.int32 if dtype == torch.float32 else torch.int16), b.view(torch.int32 if dtype == torch.float32 else torch.int16)), "two launches differ"
        keep, dlogp, dprev = (x.double() for x in runs[0])
        assert bool(torch.isfinite(keep).all() and torch.isfinite(dlogp).all() and torch.isfinite(dprev).all())
        p, dkd = prev.double(), dk.double()
        # keep: within one ULP of {0, prev}; the decision it shows must be the truth's wherever the roundings cannot flip it
        e0, e1 = keep.abs(), (keep - p).abs()
        assert bool((torch.minimum(e0, e1) <= U * p.abs()).all()), f"n={n}: keep is not within one ULP of {{0, prev}}"
        want = torch.where(t["dec0"], p, torch.zeros_like(p))
        det = t["determined"]
        assert bool(((keep - want).abs() <= U * p.abs())[det].all()), f"n={n}: a determined decision differs"
        # dprev = dkeep * ret0 shows the decision also where prev == 0
        wantd = torch.where(t["dec0"], dkd, torch.zeros_like(dkd))
        r_prev_any = torch.minimum(dprev.abs(), (dprev - dkd).abs()) / t["tol_dprev"].clamp_min(1e-300)
        r_prev = ((dprev - wantd).abs() / t["tol_dprev"].clamp_min(1e-300))[det]
        r_logp = (dlogp - t["dlogp"]).abs() / t["tol_dlogp"].clamp_min(1e-300)
        r_logp = torch.where((dlogp - t["dlogp"]).abs() == 0, torch.zeros_like(r_logp), r_logp)
        i = int(r_logp.argmax())
        ulps = float((dlogp - t["dlogp"]).abs().flatten()[i] / (U * t["dlogp"].abs().flatten()[i]).clamp_min(1e-300))
        print(f"gumbel {_name(dtype)} tau={tau} n={n}: {int(det.sum())} of {n} decisions determined; dlogp worst err/tol {float(r_logp.max()):.3f} ({ulps:.2g} ulp at {divmod(i, 2)}); "
              f"dprev worst err/tol {float(r_prev_any.max()):.3f}")
        assert float(r_prev_any.max()) <= 1.0 and (r_prev.numel() == 0 or float(r_prev.max()) <= 1.0), f"n={n}: dprev"
        assert float(r_logp.max()) <= 1.0, f"n={n}: dlogp outside its bound at {divmod(i, 2)}"
