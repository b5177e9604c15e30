"""CPU: the integer-lattice cases of oracle/linear_truth.py have exactly one right answer, an emulation of the specified arithmetic finds it in
every tiling and summation order, and every small mutant of that emulation is caught on the family made for it -- while the mutants marked below
pass the tolerances the linear kernels were tested with so far (gaussian inputs), which is the gap tests/test_linear_exact_gpu.py closes."""
import math

import pytest
import torch

from oracle import linear_truth as lt

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
M, N, K = 20, 64, 512  # emulation shape: a ragged last row tile (rows 16..19), four 16-wide strips, 16 scale blocks
TILINGS = [(1, 1, "forward"), (2, 4, "forward"), (3, 8, "reverse"), (8, 2, "tree"), (5, 3, "tree")]  # (k slices, lanes, order)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for dt in DTYPES:
        for fam in lt.FAMILIES:
            out[fam, dt] = lt.make_case(fam, M, N, K, dt, seed=1, cuts=(K // 8 * 3 // 8 * 8, 256))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_premises_hold_on_the_reference_alone(cases, dtype):
    lt.check_premises(cases["small_a", dtype], others=(cases["small_b", dtype],))
    lt.check_premises(cases["small_b", dtype], others=(cases["small_a", dtype],))
    lt.check_premises(cases["wide", dtype])
    lt.check_premises(cases["outlier", dtype], others=(cases["small_b", dtype],))
    bs = lt.blockscale(cases["wide", dtype])
    lt.check_blockscale(bs)
    lt.check_premises(bs)
    # both sides of every named cut, k = 0 and k = K - 1 carry a non-zero of the sparse operand
    for fam, op in (("small_a", "x"), ("small_b", "w")):
        c = cases[fam, dtype]
        occ = (getattr(c, op) != 0).any(0)
        for k in (0, K - 1) + tuple(k for cut in c.cuts for k in (cut - 1, cut)) + tuple(k for cut in range(32, K, 32) for k in (cut - 1, cut)):
            assert bool(occ[k]), (fam, k)


def test_rounding_helpers():
    t = torch.tensor([256.0, 257.0, 258.0, 259.0, -257.0, 2049.0, 3.0, 0.0625 * 3], dtype=torch.float64)
    assert lt.representable(t, torch.bfloat16).tolist() == [True, False, True, False, False, False, True, True]
    assert lt.is_tie(t, torch.bfloat16).tolist() == [False, True, False, True, True, False, False, False]
    assert lt.rne(t, torch.bfloat16).tolist() == [256.0, 256.0, 258.0, 260.0, -256.0, 2048.0, 3.0, 0.1875]  # ties to even
    assert lt.truncate(t, torch.bfloat16).tolist() == [256.0, 256.0, 258.0, 258.0, -256.0, 2048.0, 3.0, 0.1875]
    assert lt.is_tie(torch.tensor([2049.0], dtype=torch.float64), torch.float16).tolist() == [True]
    for dt in (torch.bfloat16, torch.float16):
        assert lt.silu_is_identity_on((0.0, 16.0, 32.0), dt) and not lt.silu_is_identity_on((2.0,), dt)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.values())
def test_emulation_equals_expected_in_every_tiling(cases, dtype):
    for fam in lt.FAMILIES:
        c = cases[fam, dtype]
        exp = c.expected()
        for n_slices, lanes, order in TILINGS:
            assert torch.equal(lt.emulate(c.x, c.w, dtype, n_slices, lanes, order), exp), (fam, n_slices, lanes, order)
        # the fp32 partial sums of a k range are the truth of that range
        bounds = [(0, 192), (192, 448), (448, K)]
        parts = c.expected_parts(bounds)
        assert torch.equal(parts.double().sum(0), c.truth)
        for (k0, k1), p in zip(bounds, parts):
            assert torch.equal(lt.emulate(c.x[:, k0:k1], c.w[:, k0:k1], torch.float32, 2, 4, "tree"), p)
    # MXFP8: codes at unit scale, one fp32 partial per 32-block, 2^e applied to it
    from dynamic_llava_amd import mxfp8

    for base in ("small_a", "wide"):
        bs = lt.blockscale(cases[base, dtype])
        q, sc = lt.check_blockscale(bs)
        codes = mxfp8._e4m3_values(q)
        e = sc.to(torch.int32) - 127
        for n_slices, lanes, order in TILINGS[:3]:
            assert torch.equal(lt.emulate(bs.x, codes, dtype, n_slices, lanes, order, scale_e=e), bs.expected()), (base, n_slices, lanes, order)


def test_bias_residual_and_prologue_cases_are_exact():
    for dt in (torch.bfloat16, torch.float16):
        c = lt.make_case("wide", 5, 48, 256, dt, bias=True, resid=True)
        t = lt.rne(c.truth + c.bias.double(), dt)
        assert torch.equal(c.expected(), lt.rne(c.resid.double() + t.double(), dt))
        for fam in ("small", "wide"):
            a = lt.make_addnorm_case(fam, 3, 32, 512, dt)
            e = a.extra
            hn = (e["h_in"].float() + e["delta"].float()).to(dt)
            assert torch.equal(hn, e["h_out"])
            xn = (hn.float() * torch.rsqrt(hn.float().pow(2).mean(-1, keepdim=True) + e["eps"])).to(dt)  # oracle/ref_cpu.py's RMSNorm
            assert torch.equal(e["norm_w"] * xn, a.x)
            s = lt.make_silumul_case(fam, 3, 32, 512, dt)
            g, u = s.extra["gate_up"][:, :512], s.extra["gate_up"][:, 512:]
            assert torch.equal((torch.nn.functional.silu(g.float()).to(dt).float() * u.float()).to(dt), s.x)  # oracle/ref_cpu.py's MLP activation
            if fam == "small":
                assert a.regime == s.regime == "exact"
                assert bool(lt.representable(a.truth, dt).all()) and bool(lt.representable(s.truth, dt).all())
            else:
                for c in (a, s):  # (iii) for both prologues' wide cases, at the shapes of the GPU table too
                    assert c.regime == "rounding" and float((~lt.representable(c.truth, dt)).float().mean()) >= 0.25
                for B in (1, 3, 8):
                    w = lt.make_silumul_case("wide", B, 40, 512, dt, seed=16 * B)
                    assert float((~lt.representable(w.truth, dt)).float().mean()) >= 0.25
        x, w, y = lt.make_silu_pair_case(4, 32, 256, dt)
        gu = (x.float() @ w.float().T).to(dt)
        assert torch.equal((torch.nn.functional.silu(gu[:, :32].float()).to(dt).float() * gu[:, 32:].float()).to(dt), y)


# mutant -> (family that must catch it, emulate() arguments)
CATCHERS = {
    "truncate_output": ("wide", dict(n_slices=2, lanes=4)),
    "partials_rounded_to_dtype": ("wide", dict(n_slices=2, lanes=4)),
    "running_sum_in_dtype": ("wide", dict(n_slices=3, lanes=2)),
    "last_k_dropped_in_strip": ("small_a", dict(n_slices=2, lanes=4)),
    "weights_8_early": ("small_a", dict(n_slices=1, lanes=4)),
    "scale_of_block_b+1": ("blockscale", dict(n_slices=2, lanes=1)),
    "scale_of_block_b-1": ("blockscale", dict(n_slices=2, lanes=1)),
    "pad_row_reads_next_row": ("small_b", dict(n_slices=1, lanes=1, guard_rows=16)),
    "row_paired_with_m+1": ("small_b", dict(n_slices=1, lanes=1)),
    "row_paired_with_m-1": ("outlier", dict(n_slices=1, lanes=1)),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_every_mutant_is_caught_on_its_family(cases, dtype):
    """The mutant table of docs/linear_exactness.md: differing elements per (mutant, family); the family named in CATCHERS must see >= 1, the unmutated
    emulation 0 everywhere."""
    from dynamic_llava_amd import mxfp8

    assert set(CATCHERS) == set(lt.MUTANTS)
    fams = {f: cases[f, dtype] for f in lt.FAMILIES}
    fams["blockscale"] = lt.blockscale(cases["wide", dtype])
    q, sc = lt.check_blockscale(fams["blockscale"])
    mx = dict(w=mxfp8._e4m3_values(q), scale_e=sc.to(torch.int32) - 127)
    table = {}
    for mutant in (None,) + lt.MUTANTS:
        for fam, c in fams.items():
            kw = dict(CATCHERS[mutant][1]) if mutant else dict(n_slices=2, lanes=4)
            guard = kw.get("guard_rows", 0)
            exp = c.expected()
            if guard:
                exp = torch.cat([exp, torch.full((guard, N), float("nan"), dtype=dtype)], 0)
            w_kw = mx if fam == "blockscale" else dict(w=c.w)
            if fam != "blockscale" and mutant and mutant.startswith("scale_of"):
                continue
            got = lt.emulate(c.x, out_dtype=dtype, mutant=mutant, **w_kw, **kw)
            table[mutant, fam] = lt.count_diff(got, exp)
    print(f"\n{DT_ID[dtype]}: differing elements of {M} x {N}; families " + ", ".join(fams))
    for mutant in (None,) + lt.MUTANTS:
        print(f"  {str(mutant):28s} " + " ".join(f"{table.get((mutant, f), '-'):>6}" for f in fams))
    assert all(table[None, f] == 0 for f in fams)
    for mutant, (fam, _) in CATCHERS.items():
        assert table[mutant, fam] >= 1, (mutant, fam)
    assert table["truncate_output", "small_a"] == 0 and table["partials_rounded_to_dtype", "small_a"] == 0  # nothing rounds there: the two regimes complement each other
    assert table["last_k_dropped_in_strip", "small_a"] == 16  # every element of the strip


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_rounding_mutants_pass_the_older_tolerances_on_gaussian_inputs(dtype):
    """Records the gap: on randn activations and randn / sqrt(K) weights (the only inputs the linear kernels were tested with) at M = 32, N = 512,
    K = 4096, the truncating output and -- in fp16 -- the k-slice partial sums rounded to the dtype stay inside both
    test_linear_packed_vs_fp32_every_layout's bound and _close_ulp(1 ulp, atol 1e-3); in bf16 the rounded partials and the dropped k term stay inside
    the former.  The same mutants on the lattice families differ in thousands of elements (test above; here at the same shape for the table).
    (A mutant passes the max |ref|-scaled bound whenever no output of the top binade sits next to the largest one: about half of the seeds; this is one.)"""
    g = torch.Generator().manual_seed(1)
    m, n, k = 32, 512, 4096
    x = torch.randn(m, k, generator=g).to(dtype)
    w = (torch.randn(n, k, generator=g) / math.sqrt(k)).to(dtype)
    ref64 = x.double() @ w.double().T
    ref = ref64.float().to(dtype)
    res = {}
    for mutant in (None, "truncate_output", "partials_rounded_to_dtype", "last_k_dropped_in_strip", "weights_8_early"):
        y = lt.emulate(x, w, dtype, 2, 4, "forward", mutant=mutant)
        res[mutant] = (lt.old_linear_packed_ratio(y, ref64, dtype, k), lt.old_close_ulp_bad(y, ref, dtype), lt.count_diff(y, ref))
        print(f"{DT_ID[dtype]} gaussian {str(mutant):28s} linear_packed ratio {res[mutant][0]:.2f}, outside _close_ulp {res[mutant][1]}, differing {res[mutant][2]}")
    assert res[None][0] < 1 and res[None][1] == 0
    assert res["truncate_output"][0] < 1 and res["truncate_output"][1] == 0 and res["truncate_output"][2] > 1000, "the truncating store passes both older checks"
    assert res["partials_rounded_to_dtype"][0] < 1 and res["partials_rounded_to_dtype"][2] > 1000
    if dtype == torch.float16:
        assert res["partials_rounded_to_dtype"][1] == 0
    else:
        assert res["last_k_dropped_in_strip"][0] < 1 and res["last_k_dropped_in_strip"][2] >= 1
    assert res["weights_8_early"][0] > 1  # (a gross fault is caught either way)
    # the lattice at the same shape
    wide = lt.make_case("wide", m, n, k, dtype)
    small = lt.make_case("small_a", m, n, k, dtype)
    for mutant in ("truncate_output", "partials_rounded_to_dtype", "last_k_dropped_in_strip", "weights_8_early"):
        dw = lt.count_diff(lt.emulate(wide.x, wide.w, dtype, 2, 4, mutant=mutant), wide.expected())
        ds = lt.count_diff(lt.emulate(small.x, small.w, dtype, 2, 4, mutant=mutant), small.expected())
        print(f"{DT_ID[dtype]} lattice  {mutant:28s} small {ds}, wide {dw}")
        assert dw >= 1 if mutant != "last_k_dropped_in_strip" else ds == 16


def _dry_entries():
    """A few entries of every table of oracle/linear_cases.py: first, last and one in the middle."""
    from oracle import linear_cases as lc

    out = []
    for kernel, (table, _) in lc.TABLES.items():
        for e in (table[0], table[len(table) // 2], table[-1]):
            out.append(pytest.param(kernel, e, id=e["id"]))
    return out


@pytest.mark.parametrize("kernel,entry", _dry_entries())
def test_gpu_table_is_consistent_with_the_specified_arithmetic(kernel, entry):
    """The runners of tests/test_linear_exact_gpu.py on a CPU stand-in for the kernels (fp64 products, the header's k ranges and rounding points): every check
    passes, so a GPU failure is a finding about the kernel and not about the table; and a stand-in that truncates, or writes one element past its
    output, is reported by the same runner."""
    from dynamic_llava_amd import hip_ops
    from oracle import linear_cases as lc

    hip_ops.load_library()  # host queries only (dl_gemm_smallm_slices, dl_gemm_mx8_slices)
    R = lc.Runner(lc.ReferenceOps(hip_ops), device="cpu")
    lc.TABLES[kernel][1](R, entry)
    R.finish()
    assert R.n > 0 and not R.bad, R.bad[:3]


def test_runner_reports_wrong_values_guard_writes_and_unrepeatable_bits():
    from dynamic_llava_amd import hip_ops

    hip_ops.load_library()
    from oracle import linear_cases as lc

    class Truncating(lc.ReferenceOps):
        def linear(self, a, w, bias=None, flags=0, residual=None, out=None):
            out.copy_(lt.truncate(self._mm(a, w) + (0 if bias is None else bias.double()), a.dtype))

    class PastTheRow(lc.ReferenceOps):
        def linear(self, a, w, **kw):
            super().linear(a, w, **kw)
            out = kw["out"]
            out.as_strided((1, 1), (1, 1), out.storage_offset() + out.shape[1]).fill_(0)

    class Unrepeatable(lc.ReferenceOps):
        calls = 0

        def linear(self, a, w, **kw):
            super().linear(a, w, **kw)
            Unrepeatable.calls += 1
            if Unrepeatable.calls % 2 == 0:
                kw["out"][0, 0] += 1

    class PastTheWorkspace(lc.ReferenceOps):
        def gemm_smallm(self, x, w, out=None, workspace=None, **kw):
            super().gemm_smallm(x, w, out=out, workspace=workspace, **kw)
            workspace.as_strided((1,), (1,), workspace.storage_offset() + workspace.numel()).fill_(0)

    R = lc.Runner(PastTheWorkspace(hip_ops), device="cpu")
    lc.run_smallm(R, lc.SMALLM_TABLE[0])
    assert not R.bad
    R.finish()
    assert R.bad and all("workspace guard band" in b["tag"] for b in R.bad)
    entry = lc.LINEAR_TABLE[0]
    for cls, key in ((Truncating, "differing"), (PastTheRow, "guard_intact"), (Unrepeatable, "second_launch_same")):
        R = lc.Runner(cls(hip_ops), device="cpu")
        lc.run_linear(R, entry)
        assert R.bad and any(b[key] not in (0, True) if key == "differing" else b[key] is False for b in R.bad), (cls.__name__, R.bad[:1])


def test_instantiation_list_matches_the_dispatch_sources():
    """oracle/linear_cases.all_instantiations() -- what test_every_reachable_instantiation_is_driven holds the GPU table to -- equals the list parsed out of
    the host dispatch code in csrc/ (template arguments, case lists, thresholds): a new tile shape, unit count or batch case, or a moved threshold, fails here
    until the table follows."""
    import os

    from oracle import linear_cases as lc

    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynamic_llava_amd", "csrc")
    in_src, listed = lc.instantiations_in_sources(csrc), lc.all_instantiations()
    assert in_src == listed, (sorted(in_src - listed)[:8], sorted(listed - in_src)[:8])
    assert lc.driven() | set(lc.omitted()) == in_src  # (the tables of oracle/linear_cases.py and, for what it used to omit, of oracle/rowwise_cases.py)
