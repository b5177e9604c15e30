"""GPU: the keep / evict predictors and the greedy advance, stage by stage and element by element.

tests/test_kernels_gpu.py bounds max|err| of the predictors' logits over the whole tensor at a few contiguous shapes and gives dl_decode_advance one case;
tests/test_predictor_truth_cpu.py shows a dropped 16-byte chunk, a neighbour's bias, a missing rounding and a `>=` in the decision passing that.  Here every
stage is judged from the kernel's own previous intermediate (the caller's workspace) against the set of values its specification can produce
(oracle/predictor_truth.py), on integer-lattice inputs whose every element has one feasible value and on generic rows with planted logit gaps, at the
smallest shapes that reach each branch of csrc/tp_body.h, csrc/predictors.hip and csrc/advance.hip (oracle/predictor_cases.py: the tables and the runner) -- inside guard
bands, every launch twice with the same bits.  dl_decode_advance is compared bit for bit with a plain restatement.  docs/predictor_exactness.md has the
construction, the mutant table and the measured results."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import predictor_cases as pc  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from dynamic_llava_amd import hip_ops

    hip_ops.require_gpu()
    return hip_ops


def _run(ops, kernel, entry):
    R = pc.Runner(pc.HipAdaptor(ops))
    pc.TABLES[kernel][1](R, entry)
    R.finish()
    torch.cuda.synchronize()
    print(f"{entry['id']}: {R.n} checks, {len(R.bad)} failed")
    stages = {}
    for t, u in R.undecided.items():
        key = t[len(entry["id"]) + 1 :]
        stages[key] = max(stages.get(key, 0.0), u)
    for k, u in stages.items():
        print(f"  undecided {u:.4f}  {k}")
    for t, r in R.ratios.items():
        print(f"  {t}: kernel error / tolerance {r['ratio']:.3f} (eager row maximum {r['eager_row_max']:.3e}, kernel maximum {r['kernel_max']:.3e})")
    assert R.n > 0
    assert not R.bad, R.bad[:4]


def _params(kernel):
    return [pytest.param(e, id=e["id"]) for e in pc.TABLES[kernel][0]]


@pytest.mark.parametrize("entry", _params("text_predictor"))
def test_text_predictor_stages(ops, entry):
    """dl_text_predictor_decide: stage 1 (through ln_truth's interval of the LDS row), 2a, the two layers of 2b and the decision; lattice rows (planted ties
    decide 0), generic rows with a non-finite one, row strides H and H + 16, logits_out = NULL; the H past the largest is refused."""
    _run(ops, "text_predictor", entry)


@pytest.mark.parametrize("entry", _params("gemv_gu_tp"))
def test_fused_text_predictor(ops, entry):
    """dl_gemv_gu_tp / dl_gemv_gu_tp_pk: both MAXC instantiations; the predictor's outputs carry the bits of the separate launches and meet the criterion."""
    _run(ops, "gemv_gu_tp", entry)


@pytest.mark.parametrize("entry", _params("vision_predictor"))
def test_vision_predictor_stages(ops, entry):
    """dl_vision_predictor out of its workspace: the gather, x0, down, pool_concat (n_img whose RNE_T differs from n), out0, out2, the head and the score, with
    ragged cu_seqlens and a different img_start per row; the transformer blocks against an fp64 chain started from the kernel's own hs."""
    _run(ops, "vision_predictor", entry)


@pytest.mark.parametrize("entry", _params("decode_advance"))
def test_decode_advance_bit_exact(ops, entry):
    """dl_decode_advance against predictor_truth.advance_ref: maxima and tie pairs on both sides of every vector, wave, block and loop-trip boundary, the tail,
    an unaligned base and an odd stride (the scalar path), one to three banned EOS ids holding the maximum, step at out_cap - 1 and out_cap, finished rows,
    NaN, all-NaN and -inf rows."""
    _run(ops, "decode_advance", entry)
