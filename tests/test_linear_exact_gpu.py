"""GPU: every GEMM / GEMV kernel instantiation of the library, bit for bit, on inputs that have exactly one right answer.

tests/test_kernels_gpu.py, test_linear_tiles_gpu.py and test_mxfp8*_gpu.py feed these kernels randn activations and randn / sqrt(K) weights and scale their
tolerance by the largest output; tests/test_linear_truth_cpu.py shows a truncating store, 16-bit partial sums and a dropped k term passing that.  Here the
operands are the integer lattices of oracle/linear_truth.py: products and every fp32 partial sum in any order are exact, so include/dynllava.h's "fp32
accumulation, one rounding" means RNE(truth) and the assertion is equality -- of the output, of every fp32 partial-sum buffer against the truth of its k
range, of dl_quantize_mx8's codes against the host quantiser's -- inside NaN guard bands, on strided rows, twice with the same bits
(oracle/linear_cases.py: the table, one entry per template instantiation the dispatch code can reach, and the runner).  docs/linear_exactness.md has the
construction, the mutant table and the measured results."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import linear_cases as lc  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from dynamic_llava_amd import hip_ops

    hip_ops.require_gpu()
    return hip_ops


def _run(ops, kernel, entry):
    R = lc.Runner(ops)
    lc.TABLES[kernel][1](R, entry)
    R.finish()
    torch.cuda.synchronize()
    print(f"{entry['id']}: {R.n} checks, {len(R.bad)} failed; instantiation {sorted(entry['inst'])}")
    assert R.n > 0
    assert not R.bad, R.bad[:8]


def _params(kernel):
    return [pytest.param(e, id=e["id"]) for e in lc.TABLES[kernel][0]]


@pytest.mark.parametrize("entry", _params("linear"))
def test_linear(ops, entry):
    """dl_linear: MFMA kernel with K >= 1024 and K < 1024 (K no multiple of the k tile), the fp32 kernel; flags 0 / DL_EPI_RESIDUAL x bias; ragged M, N."""
    _run(ops, "linear", entry)


@pytest.mark.parametrize("entry", _params("splitk"))
def test_linear_splitk(ops, entry):
    """dl_linear_splitk: the three tilings x n_slices 1, 3, 8; every part is the truth of its k range, so their sum is exact."""
    _run(ops, "splitk", entry)


@pytest.mark.parametrize("entry", _params("gemv"))
def test_gemv(ops, entry):
    """dl_gemv: B = 1..8, every prologue with and without the SiLU-pair epilogue, the four batch-1 register kernels and the generic one, two grid caps."""
    _run(ops, "gemv", entry)


@pytest.mark.parametrize("entry", _params("gemv_mx8"))
def test_gemv_mx8(ops, entry):
    """dl_gemv_mx8 on weights quantised by dl_quantize_mx8 (codes and scales equal the host's): a different block scale in every neighbouring block and row."""
    _run(ops, "gemv_mx8", entry)


@pytest.mark.parametrize("entry", _params("smallm"))
def test_gemm_smallm(ops, entry):
    """dl_gemm_smallm: variants 1 (4 / 8 waves), 2, 3; one and two row tiles, ragged; n_slices 0, 1, 3 and the slicing LDS forces; the partial-sum form into
    dl_add_rmsnorm_parts and dl_silu_mul_parts."""
    _run(ops, "smallm", entry)


@pytest.mark.parametrize("entry", _params("gemm_mx8"))
def test_gemm_mx8(ops, entry):
    """dl_gemm_mx8: M 4, 16, 17, 32 x slices automatic, 1 and K / 256, stored and as partial sums."""
    _run(ops, "gemm_mx8", entry)


@pytest.mark.parametrize("entry", _params("linear_packed"))
def test_linear_packed(ops, entry):
    """dl_linear_packed: every units-per-workgroup x row-tile count x epilogue, row-major and fragment-order X, k_split 1 and 2 / 3 / 8."""
    _run(ops, "linear_packed", entry)


@pytest.mark.parametrize("entry", _params("linear_tiles"))
def test_linear_tiles(ops, entry):
    """dl_linear_tiles: every built tile shape, bias, partial sums with k_split 1 and 3, row-major and fragment-order X and Y."""
    _run(ops, "linear_tiles", entry)


def test_every_reachable_instantiation_is_driven():
    """The tables name every template instantiation the dispatch code of the eight entry points can reach in a release build: this one, and for the fp32
    prologues, the SiLU-pair epilogues that round and the GELU / QuickGELU epilogues, oracle/rowwise_cases.py (tests/test_rowwise_exact_gpu.py).  Nothing is
    left in linear_cases.omitted()."""
    driven = lc.driven()
    everything, omitted = lc.all_instantiations(), lc.omitted()
    assert set(omitted) <= everything and not (set(omitted) & driven)
    assert all(len(reason) > 10 for reason in omitted.values())
    assert driven | set(omitted) == everything, sorted(everything - driven - set(omitted))[:10] + sorted(driven - everything)[:10]
