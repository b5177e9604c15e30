"""CPU: the hard rows of oracle/rowwise_truth.py and the feasible-set criterion.  (i) the oracle's expressions satisfy the criterion on every case of the GPU
table, within the caps on the undecided share; (ii) every small mutant of the specified arithmetic is caught on the rows made for it; (iii) most of them pass
the assertions the norm and activation kernels were tested with so far; (iv) the GPU runner is consistent with the specified arithmetic and reports a
truncating store and a write past the row; (v) the measured constants are re-derived; (vi) the table names every branch the dispatch sources hold."""
import os

import pytest
import torch

from oracle import linear_truth as lt
from oracle import ref_cpu as orc
from oracle import rowwise_cases as rc
from oracle import rowwise_truth as rt

BF16, F16, F32 = rt.BF16, rt.F16, rt.F32
DTYPES = [BF16, F16, F32]
DT_ID = {BF16: "bf16", F16: "fp16", F32: "fp32"}
EPS = rc.EPS
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynamic_llava_amd", "csrc")


def _ops():
    from dynamic_llava_amd import hip_ops

    hip_ops.load_library()  # host queries only
    return hip_ops


def _dry(kernel, entry, ops_cls=None):
    R = rc.Runner((ops_cls or rc.ReferenceOps)(_ops()), device="cpu")
    rc.TABLES[kernel][1](R, entry)
    R.finish()
    return R


# ------------------------------------------------------------------------------------------------------------------------------
# (i) the reference on every case
# ------------------------------------------------------------------------------------------------------------------------------
FULL = ("rmsnorm", "add_rmsnorm_parts", "rmsnorm_packed", "layernorm", "layernorm_rows", "compact_tokens", "activations")


@pytest.mark.parametrize("kernel", FULL)
def test_reference_satisfies_the_criterion_on_every_case(kernel):
    """Every entry of the norm and activation tables through the runner, on oracle/ref_cpu.py's expressions: 0 elements outside their feasible set, the
    undecided share of every launch inside its cap (lattice 0.5 %, generic RMSNorm and activations 2 %; LayerNorm generic rows: printed, no cap)."""
    worst = {}
    for e in rc.TABLES[kernel][0]:
        R = _dry(kernel, e)
        assert R.n > 0 and not R.bad, (e["id"], R.bad[:2])
        for tag, u in R.undecided.items():
            cls = "lattice" if " lattice " in tag else ("generic" if " generic " in tag else "other")
            worst[cls] = max(worst.get(cls, 0.0), u)
    print(f"\n{kernel}: largest undecided share " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
    assert worst.get("lattice", 0.0) <= rc.CAP_LATTICE


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_layernorm_expression_satisfies_the_criterion(dtype):
    """The specified expression (x - mean) * rstd * w + b, evaluated in fp32 in both summation orders and cast, lies inside the budget on every row of the
    table.  F.layer_norm in fp32 then cast is recorded next to it and not asserted: torch's CPU kernel evaluates (x * rstd + (-mean * rstd)) * w + b, whose
    roundings are relative to |x| rstd and not to |x - mean| rstd, so a handful of its elements leave a budget derived for the other expression."""
    outside = n = 0
    for H in rc.H_BLOCK[dtype]:
        if H < 8:
            continue
        w, b = rc.weight(H, dtype), rc.bias(H, dtype)
        for cls in ("lattice", "generic"):
            x = rc.rows("ln", cls, H, dtype).to(dtype)
            F = rc.truth("ln", x, w, b, cls)
            for order in (0, 1):
                assert bool(F.ok(rt.emulate_layernorm(x, w, b, EPS, order=order)).all()), (H, cls, order)
            y = torch.nn.functional.layer_norm(x.float(), (H,), w.float(), b.float(), EPS).to(dtype)
            outside += int((~F.ok(y)).sum())
            n += y.numel()
            if cls == "lattice":
                assert torch.equal(rt.emulate_layernorm(x, w, b, EPS)[2], b)  # the constant row: exactly the bias
    print(f"\n{DT_ID[dtype]}: F.layer_norm (torch's CPU kernel, another expression) outside the budget in {outside} of {n}")


# ------------------------------------------------------------------------------------------------------------------------------
# (ii) mutants
# ------------------------------------------------------------------------------------------------------------------------------
# mutant -> (row class, H for 16-bit / fp32, dtypes that cannot show it and why)
RMS_CATCHERS = {
    "weight_before_cast": ("generic", (2056, 1028), {F32: "no cast between the two products in fp32"}),
    "truncated_store": ("lattice", (2056, 1028), {F32: "an fp32 store does not round"}),
    "rstd_16bit": ("lattice", (2056, 1028), {}),
    "padded_count": ("lattice", (264, 132), {}),
    "eps_lost": ("lattice", (2056, 1028), {}),
    "eps_outside_root": ("lattice", (2056, 1028), {}),
    "last_vector_dropped": ("lattice", (2056, 1028), {}),
    "reread_vector0_counted": ("lattice", (264, 132), {}),
}
LN_CATCHERS = {
    "one_pass_variance": ("generic", (2056, 1028), {BF16: "not claimed: adjacent bf16 levels bound mu / sigma at 2^8, E[x^2] - mu^2 then keeps 8 of 24 bits -- bf16's own 8 (0 or 1 element seen)"}),
    "extra_rounding_before_affine": ("lattice", (1032, 516), {F32: "no cast in fp32"}),
    "truncated_store": ("lattice", (1032, 516), {F32: "an fp32 store does not round"}),
    "padded_count": ("lattice", (520, 260), {}),
    "eps_lost": ("lattice", (1032, 516), {}),
    "last_vector_dropped": ("lattice", (1032, 516), {}),
    "reread_vector0_counted": ("lattice", (520, 260), {}),
}


def _outside(F, y):
    return int((~F.ok(y)).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_every_norm_mutant_is_caught_on_its_rows(dtype):
    """The mutant table of docs/rowwise_exactness.md: elements outside their feasible set per (mutant, row class).  The class named in *_CATCHERS must see >= 1,
    the unmutated expression 0 on both classes and in both summation orders; where a dtype is listed as unable to show a mutant nothing is claimed (fp32,
    where the mutated step does not exist, must see exactly 0)."""
    assert set(RMS_CATCHERS) == set(rt.RMS_MUTANTS) and set(LN_CATCHERS) == set(rt.LN_MUTANTS)
    print()
    for family, catchers, emulate in (("rms", RMS_CATCHERS, rt.emulate_rmsnorm), ("ln", LN_CATCHERS, rt.emulate_layernorm)):
        for mutant, (cls, Hs, cannot) in catchers.items():
            H = Hs[1] if dtype == F32 else Hs[0]
            w, b = rc.weight(H, dtype), rc.bias(H, dtype)
            counts = {}
            for c in ("lattice", "generic"):
                x = rc.rows(family, c, H, dtype).to(dtype)
                F = rc.truth(family, x, w, b, c)
                args = (x, w, EPS) if family == "rms" else (x, w, b, EPS)
                for order in (0, 1):
                    assert _outside(F, emulate(*args, order=order)) == 0, (family, c, H, order)
                counts[c] = _outside(F, emulate(*args, mutant=mutant))
            print(f"  {DT_ID[dtype]} {family:3s} {mutant:30s} H {H:5d}  lattice {counts['lattice']:6d}  generic {counts['generic']:6d}" + (f"   (cannot show: {cannot[dtype]})" if dtype in cannot else ""))
            if dtype in cannot:
                assert dtype != F32 or counts[cls] == 0, (mutant, "is listed as not showable but is seen: claim it")
            else:
                assert counts[cls] >= 1, (family, mutant, cls, H)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_slice_mutants_at_the_batch_boundary(dtype):
    """A slice lost or counted twice where the second batch of kPartsBatch = 8 slices begins: the residual stream itself differs (it is compared with ==)."""
    H = 264 if dtype != F32 else 132
    for ns in (9, 17):
        h0, p, _, x = rc.parts_case("rms", "lattice", H, dtype, ns)
        assert torch.equal(rt.emulate_add_parts(h0, p), x)
        for mutant in rt.PARTS_MUTANTS:
            assert lt.count_diff(rt.emulate_add_parts(h0, p, mutant), x) >= 1, (mutant, ns)
    h0, p, _, x = rc.parts_case("rms", "lattice", H, dtype, 8)  # (eight slices: one full batch, the mutants have nothing to touch)
    assert all(torch.equal(rt.emulate_add_parts(h0, p, m), x) for m in rt.PARTS_MUTANTS)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_activation_mutants_over_every_input(dtype):
    """silu without the inner rounding, the fast form without its guard (a relative error of 2^-20) and a truncating store, over all finite gates x the eight up
    values; the oracle's expressions: 0 outside, undecided share <= 2 %.  (fp32 has no inner rounding and no guard: the mutants do not exist there.)"""
    gu, fin = rc.act_inputs(dtype)
    I = gu.shape[1] // 2
    g, u = gu[:, :I][:, fin], gu[:, I:][:, fin]
    F = rt.silu_mul_truth(g, u)
    assert _outside(F, rt.emulate_silu_mul(g, u)) == 0 and F.undecided() <= rc.CAP_GENERIC
    Q = rt.quick_gelu_truth(g[0])
    assert _outside(Q, rt.emulate_quick_gelu(g[0])) == 0 and Q.undecided() <= rc.CAP_GENERIC
    n_und = int(((F.lo[0] != F.hi[0])).sum())
    print(f"\n{DT_ID[dtype]}: {n_und} of {g.shape[1]} gates undecided at rho_act = {rt.RHO_ACT:.2e} (up = 1); quick_gelu {int((Q.lo != Q.hi).sum())}")
    for mutant in rt.ACT_MUTANTS:
        bad = _outside(F, rt.emulate_silu_mul(g, u, mutant))
        print(f"  {mutant:26s} outside {bad}")
        assert bad >= 1, mutant
    over, _ = rt.exp_overflows(g[0].double())
    zone = over & (rt.to_t(rt.silu64(g[0].double()), dtype) != 0)  # the fp64 truth would not round to zero, the fp32 expression gives -0
    assert int(zone.sum()) == (17 if dtype == BF16 else 0)
    assert bool((F.lo[0][over] == 0).all() and (F.hi[0][over] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------
# (iii) what the older assertions let through
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_mutants_pass_the_older_assertions_on_the_older_inputs(dtype):
    """Records the gap: randn rows with 1 + 0.1 randn weights at H = 4096 (tests/test_kernels_gpu.py: test_rmsnorm, test_add_layernorm), _close_ulp(1 ulp) and,
    for the wave-per-row LayerNorm, 1 ulp + atol 1e-3 (test_layernorm_rows_family_vs_fp32).  `exact` is the share of equal elements (asserted > 0.99 for
    dl_rmsnorm only).  The mutants asserted below stay inside those bounds there; on the lattice rows each is caught (test above)."""
    g = torch.Generator().manual_seed(1)
    H = 4096
    x = torch.randn(8, H, generator=g).to(dtype)
    w = (1 + 0.1 * torch.randn(H, generator=g)).to(dtype)
    b = (0.1 * torch.randn(H, generator=g)).to(dtype)
    ref = orc.rmsnorm(x, w, EPS)
    print()
    res = {}
    for m in (None,) + rt.RMS_MUTANTS:
        y = rt.emulate_rmsnorm(x, w, EPS, mutant=m, order=1)
        res["rms", m] = (lt.old_close_ulp_bad(y, ref, dtype, 1.0, 0.0), float((y == ref).float().mean()))
        print(f"  {DT_ID[dtype]} rmsnorm   {str(m):30s} outside 1 ulp {res['rms', m][0]:6d}   exact {res['rms', m][1]:.4f}")
    ref_ln = torch.nn.functional.layer_norm(x.float(), (H,), w.float(), b.float(), EPS)
    for m in (None,) + rt.LN_MUTANTS:
        y = rt.emulate_layernorm(x, w, b, EPS, mutant=m, order=1)
        res["ln", m] = (lt.old_close_ulp_bad(y, ref_ln.to(dtype), dtype, 1.0, 2e-6), lt.old_close_ulp_bad(y, ref_ln, dtype, 1.0, 1e-3))
        print(f"  {DT_ID[dtype]} layernorm {str(m):30s} outside 1 ulp + 2e-6 {res['ln', m][0]:6d}   outside 1 ulp + 1e-3 {res['ln', m][1]:6d}")
    assert res["rms", None] == (0, 1.0) and res["ln", None][0] == 0
    # RMSNorm: bf16 lets six of the eight through the 1-ulp bound (all but dl_rmsnorm are held to nothing else); two of them also keep > 0.99 exact
    if dtype == BF16:
        for m in ("weight_before_cast", "truncated_store", "padded_count", "eps_lost", "eps_outside_root", "reread_vector0_counted"):
            assert res["rms", m][0] == 0, (m, "no longer passes the old bound: update docs/rowwise_exactness.md")
        assert res["rms", "eps_lost"][1] > 0.99 and res["rms", "eps_outside_root"][1] > 0.99
        assert res["rms", "weight_before_cast"][1] < 0.99 and res["rms", "truncated_store"][1] < 0.99  # (the exact share, where it is asserted, does catch these)
    # the old shapes are whole passes: a padded count and re-read lanes cannot show at all, in any dtype
    for m in ("padded_count", "reread_vector0_counted"):
        assert res["rms", m] == (0, 1.0) and res["ln", m] == (0, 0)
    # LayerNorm: no exact share anywhere; 1 ulp + 2e-6 passes three more, 1 ulp + 1e-3 (the wave-per-row family) also the extra rounding
    for m in ("one_pass_variance", "truncated_store", "eps_lost"):
        assert res["ln", m] == (0, 0), m
    assert res["ln", "extra_rounding_before_affine"][0] > 0 and res["ln", "extra_rounding_before_affine"][1] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# (iv) the runner
# ------------------------------------------------------------------------------------------------------------------------------
def _dry_entries():
    out = []
    for kernel, (table, _) in rc.TABLES.items():
        if kernel in FULL:
            continue  # run in full above
        small = [e for e in table if e.get("K", 0) <= 4104]
        for e in (small[0], small[len(small) // 2], small[-1]):
            out.append(pytest.param(kernel, e, id=e["id"]))
    return out


@pytest.mark.parametrize("kernel,entry", _dry_entries())
def test_gpu_table_is_consistent_with_the_specified_arithmetic(kernel, entry):
    """The prologue and epilogue runners of tests/test_rowwise_exact_gpu.py on the CPU stand-in: every check passes, so a GPU failure is a finding about the
    kernel and not about the table."""
    R = _dry(kernel, entry)
    assert R.n > 0 and not R.bad, R.bad[:2]


def test_runner_reports_a_truncating_store_a_write_past_the_row_and_a_touched_stream():
    class Truncating(rc.ReferenceOps):
        def rmsnorm(self, x, w, eps, out=None, packed=False):
            xn = (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)
            return out.copy_(lt.truncate(w.double() * xn.double(), x.dtype))

    class PastTheRow(rc.ReferenceOps):
        def rmsnorm(self, x, w, eps, out=None, packed=False):
            super().rmsnorm(x, w, eps, out=out, packed=packed)
            out.as_strided((1,), (1,), out.storage_offset() + out.numel()).fill_(0)
            return out

    class PastTheStream(rc.ReferenceOps):
        def add_rmsnorm(self, h, delta, w, eps, out=None, packed=False):
            r = super().add_rmsnorm(h, delta, w, eps, out=out, packed=packed)
            h.as_strided((1,), (1,), h.storage_offset() - 1).fill_(0)
            return r

    class Unrepeatable(rc.ReferenceOps):
        calls = 0

        def rmsnorm(self, x, w, eps, out=None, packed=False):
            super().rmsnorm(x, w, eps, out=out, packed=packed)
            Unrepeatable.calls += 1
            if Unrepeatable.calls % 2 == 0:
                out.view(-1)[0] = -out.view(-1)[0] + 1
            return out

    entry = rc.RMS_TABLE[2]  # bf16, H = 2056
    for cls, key in ((Truncating, "differing"), (PastTheRow, "guard_intact"), (Unrepeatable, "second_launch_same")):
        R = _dry("rmsnorm", entry, cls)
        assert R.bad and any((b[key] > 0) if key == "differing" else (b[key] is False) for b in R.bad), (cls.__name__, R.bad[:1])
    R = _dry("rmsnorm", entry, PastTheStream)
    assert R.bad and any("workspace guard band" in b["tag"] for b in R.bad)


# ------------------------------------------------------------------------------------------------------------------------------
# (v) the measured constants
# ------------------------------------------------------------------------------------------------------------------------------
def _matches(constant, measured, floor=0.0):
    """constant = max(floor, 4 x measured rounded up to two digits); a re-measurement may move by a few percent with torch's summation kernels."""
    want = max(floor, 4 * measured)
    return 0.8 * constant <= want <= constant * (1 + 1e-9)


def test_rho_generic_is_four_times_the_measured_deviation():
    """Over every generic statistic of the GPU table, in two fp32 orders that belong to no kernel (torch.sum; 256 strided lanes, then a tree)."""
    worst = {"rms": 0.0, "ln r": 0.0, "ln mean": 0.0}
    for family, tag, x in rc.generic_rows_of_the_table():
        if family == "rms":
            worst["rms"] = max(worst["rms"], rt.measure_rho_rms(x))
        else:
            dr, dm = rt.measure_rho_ln(x)
            worst["ln r"], worst["ln mean"] = max(worst["ln r"], dr), max(worst["ln mean"], dm)
    m = max(worst.values())
    print(f"\nlargest deviation: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"; x 4 = {4 * m:.3e}; RHO_GENERIC = {rt.RHO_GENERIC:.3e}; floor 2^-22 = {2.0**-22:.3e}")
    assert _matches(rt.RHO_GENERIC, m, 2.0**-22)
    assert rt.RHO_LATTICE == 2.0**-22


def test_rho_act_and_gelu_bound_are_four_times_the_measured_deviation():
    act = max(rt.measure_rho_act(dt) for dt in (BF16, F16))
    gelu = max(rt.measure_gelu_abs(dt) for dt in (BF16, F16))
    print(f"\nexp / divide: {act:.3e} x 4 = {4 * act:.3e}, RHO_ACT = {rt.RHO_ACT:.3e};  GELU: {gelu:.3e} |x| x 4 = {4 * gelu:.3e}, GELU_ABS = {rt.GELU_ABS:.3e}")
    assert _matches(rt.RHO_ACT, act, 2.0**-22) and _matches(rt.GELU_ABS, gelu)


def test_rounding_of_the_ends_is_monotone_and_exact_on_16_bit_values():
    for dt in (BF16, F16):
        v = rt.all_values(dt)
        v = v[torch.isfinite(v.float())]
        assert torch.equal(rt.to_t(v.double(), dt), v)
        s = torch.sort(v.double()).values
        mid = (s[1:] + s[:-1]) / 2
        assert bool((rt.to_t(mid, dt).double()[1:] >= rt.to_t(mid, dt).double()[:-1]).all())


# ------------------------------------------------------------------------------------------------------------------------------
# (vi) completeness
# ------------------------------------------------------------------------------------------------------------------------------
def test_table_names_every_branch_in_the_dispatch_sources():
    """LN_WAVE_CASE, the NS conditions, kMaxVecPerThread, kPartsBatch and MAXC read out of csrc/: the table holds every vectors-per-lane case (each with a
    ragged and a full last pass where both exist), both NS forms and the generic loop, both prologue branches, a slice count on either side of the batch size
    and one that is no multiple of it, and the first H past the largest row.  A new case fails here until the table follows."""
    src = rc.branches_in_sources(CSRC)
    assert src["threads"] == 256 and src["gemv_threads"] == 256
    # wave-per-row LayerNorm
    vpls = {e["vpl"] for e in rc.LN_WAVE_TABLE}
    assert vpls == set(src["ln_wave_cases"]), (vpls, src["ln_wave_cases"])
    for v in src["ln_wave_cases"]:
        kinds = {e["ragged"] for e in rc.LN_WAVE_TABLE if e["vpl"] == v}
        assert True in kinds or v == 1 and False in kinds, v
    assert any(e["ragged"] for e in rc.LN_WAVE_TABLE if e["vpl"] == 1)  # H = 8: one lane holds the row
    assert rc.vpl(rc.H_WAVE_REFUSED) not in src["ln_wave_cases"]
    assert src["ns_forms"] == [2, 4] and src["ns_max_vpl"] == [2]
    insts = rc.driven()
    for dt in ("bf16_t", "f16_t"):
        for v in src["ln_wave_cases"]:
            for add in (0, 1):
                assert f"layernorm_wave_kernel<{dt},{add},{v},0>" in insts
            for ns in (2, 4):
                assert f"layernorm_wave_kernel<{dt},2,{v},{ns if v <= 2 else 0}>" in insts
            assert f"layernorm_wave_kernel<{dt},2,{v},0>" in insts
    # block-per-row kernels
    for dt in DTYPES:
        limit = src["threads"] * src["max_vec_per_thread"] * rt.VEC[dt]
        assert rc.H_BLOCK[dt][-1] == limit and rc.H_REFUSED[dt] == limit + rt.VEC[dt]
        passes = {e["passes"] for e in rc.RMS_TABLE if e["dtype"] == dt}
        assert {1, 2, src["max_vec_per_thread"]} <= passes
        pairs = {e["pairs"] for e in rc.RMS_PARTS_TABLE if e["dtype"] == dt}
        assert {1, 2, src["max_vec_per_thread"] // 2} <= pairs
        assert any(e["H"] // rt.VEC[dt] == 257 for e in rc.RMS_PARTS_TABLE if e["dtype"] == dt)  # a pair whose second vector one lane holds
    pb = src["parts_batch"]
    assert pb in rc.PARTS_SLICES and pb + 1 in rc.PARTS_SLICES and 2 * pb + 1 in rc.PARTS_SLICES and any(n < pb for n in rc.PARTS_SLICES)
    # gemv_build_x
    for dt in DTYPES:
        assert rc.MAXC_K[dt] == src["gemv_threads"] * src["maxc"] * rt.VEC[dt]
        branches = {e["branch"] for e in rc.BUILD_X_TABLE if e["dtype"] == dt and e["mode"] == rc.ADDNORM}
        assert branches == {"registers", "lds"}
        assert any(e["K"] == rc.MAXC_K[dt] + 8 for e in rc.BUILD_X_TABLE if e["dtype"] == dt) or dt == F32  # the first K on the LDS branch (16-bit)


def test_linear_family_omissions_are_retired():
    """The 108 instantiations oracle/linear_cases.py listed as omitted (fp32 prologues and SiLU-pair epilogues of dl_gemv / dl_gemv_mx8, the GELU / QuickGELU
    epilogues of dl_linear_tiles) are driven by this table: driven + omitted == all still holds, with nothing omitted."""
    from oracle import linear_cases as lc

    everything = lc.instantiations_in_sources(CSRC)
    here = rc.driven() & everything
    assert len(here) >= 108
    assert not lc.omitted()
    assert lc.driven() == everything
