"""GPU: every launch that normalises a row or applies an activation, element by element, on hard rows.

tests/test_kernels_gpu.py and test_linear_tiles_gpu.py feed these kernels randn rows with 1 + 0.1 randn weights and allow a whole ulp (plus an atol);
tests/test_rowwise_truth_cpu.py shows a weight applied before the cast, a truncating store, a lost eps and a one-pass variance passing that.  Here the rows
are the lattice and generic rows of oracle/rowwise_truth.py, and every element has to lie in the set of values the specification can produce when its fp32
statistic is within rho of the fp64 truth (decided elements: one value; fp32: an interval) -- inside NaN guard bands, twice with the same bits, the in-place
residual stream compared with == (oracle/rowwise_cases.py: the table, one entry per instantiation and branch, and the runner).  The prologues of the
weight-streaming GEMVs are seen directly through W = I, the activation epilogues of the GEMMs through K = 64 weights that hold every 16-bit value.
docs/rowwise_exactness.md has the construction, the mutant table and the measured results."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rowwise_cases as rc  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from dynamic_llava_amd import hip_ops

    hip_ops.require_gpu()
    return hip_ops


def _run(ops, kernel, entry):
    R = rc.Runner(ops)
    rc.TABLES[kernel][1](R, entry)
    R.finish()
    torch.cuda.synchronize()
    und = [(t, u) for t, u in R.undecided.items() if u > 0 and ("layernorm" in t and " generic " in t and " row " in t or "GELU" in t)]
    print(f"{entry['id']}: {R.n} checks, {len(R.bad)} failed; largest undecided share {max(R.undecided.values(), default=0.0):.4f}")
    for t, u in und:
        print(f"  undecided {u:.4f}  {t}")
    assert R.n > 0
    assert not R.bad, R.bad[:4]


def _params(kernel):
    return [pytest.param(e, id=e["id"]) for e in rc.TABLES[kernel][0]]


@pytest.mark.parametrize("entry", _params("rmsnorm"))
def test_rmsnorm(ops, entry):
    """dl_rmsnorm, dl_add_rmsnorm with and without w: one vector, ragged passes, 257 / 513 vectors, five passes, the largest row; the next H is refused."""
    _run(ops, "rmsnorm", entry)


@pytest.mark.parametrize("entry", _params("add_rmsnorm_parts"))
def test_add_rmsnorm_parts(ops, entry):
    """dl_add_rmsnorm_parts: slice counts 1, 3, 8, 9, 17 (the batch of eight, one past it, two batches and one), vectors in pairs with a one-lane second vector."""
    _run(ops, "add_rmsnorm_parts", entry)


@pytest.mark.parametrize("entry", _params("rmsnorm_packed"))
def test_rmsnorm_packed(ops, entry):
    """The three _packed forms at 1, 17 and 256 rows: the criterion on the unpacked values, which equal the row-major launch's; 257 rows are refused."""
    _run(ops, "rmsnorm_packed", entry)


@pytest.mark.parametrize("entry", _params("layernorm"))
def test_layernorm(ops, entry):
    """dl_layernorm (with a row gather that repeats a row, and without) and dl_add_layernorm."""
    _run(ops, "layernorm", entry)


@pytest.mark.parametrize("entry", _params("layernorm_rows"))
def test_layernorm_rows(ops, entry):
    """dl_layernorm_rows, dl_add_layernorm_rows, dl_add_layernorm_parts: 1, 2, 3, 4, 8 vectors per lane with ragged last passes, slice counts 2 and 4 (the NS
    forms up to two vectors per lane, the generic loop beyond) and 3, the Linear's bias present and absent, fragment-order output where H % 64 == 0."""
    _run(ops, "layernorm_rows", entry)


@pytest.mark.parametrize("entry", _params("compact_tokens"))
def test_compact_tokens_norm(ops, entry):
    _run(ops, "compact_tokens", entry)


@pytest.mark.parametrize("entry", _params("build_x"))
def test_gemv_prologue_through_the_identity(ops, entry):
    """gemv_build_x (ADDNORM with and without delta, SILUMUL) through dl_gemv and dl_gemv_mx8 with W = I: rows in registers and rows in LDS, B = 1..8, h_out."""
    _run(ops, "build_x", entry)


@pytest.mark.parametrize("entry", _params("build_x_pk"))
def test_gemv_pk_prologue_through_the_identity(ops, entry):
    _run(ops, "build_x_pk", entry)


@pytest.mark.parametrize("entry", _params("activations"))
def test_activations_on_every_input(ops, entry):
    """dl_silu_mul, dl_silu_mul_parts, dl_quick_gelu over all 65 536 bit patterns (x eight up values); fp32: a 2^20-point sweep and the powers of two; the default
    and the DL_EXACT_ACT=1 instantiation agree in bits on finite gates."""
    _run(ops, "activations", entry)


@pytest.mark.parametrize("entry", _params("gemv_pair"))
def test_gemv_silu_pair_epilogue(ops, entry):
    _run(ops, "gemv_pair", entry)


@pytest.mark.parametrize("entry", _params("gemv_mx8_pair"))
def test_gemv_mx8_silu_pair_epilogue(ops, entry):
    """A sample: MXFP8 weights cannot hold arbitrary gates."""
    _run(ops, "gemv_mx8_pair", entry)


@pytest.mark.parametrize("entry", _params("linear_packed_pair"))
def test_linear_packed_silu_pair_epilogue(ops, entry):
    _run(ops, "linear_packed_pair", entry)


@pytest.mark.parametrize("entry", _params("linear_tiles_act"))
def test_linear_tiles_activation_epilogues(ops, entry):
    """LT_QGELU (its own copy of the guarded sigmoid) and LT_GELU in every built tile shape, over every 16-bit value."""
    _run(ops, "linear_tiles_act", entry)
