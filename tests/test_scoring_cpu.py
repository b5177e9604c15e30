"""CPU: the scoring rule (dynamic_llava_amd/scoring.py, the contract of dl_decode_score) -- its exact identities, its distance from
torch.log_softmax in float64, the mutants it must tell apart, label validation and the library's argument checks.

The bound against float64 is score_cases.rule_bound, derived there term by term: one ulp of d = m - x_label; a relative error of the summed weights of
28 * 2^-24 (the fp32 subtraction x - m: only terms with |x - m| < 28 have a non-zero mass) + 2^-23 (exp, one ulp: the HIP math API's bound for expf, and
torch's CPU exp is within the same) + V * 2^-40 (one floor unit per token against M >= 2^40) + 2^-24 (the u64 -> fp32 conversion), carried through the
logarithm (e / (1 - e)); one ulp of lse (log); one ulp of nll (the final addition).  Ulps are taken one binade above the float64 value's."""
import ctypes
import math

import pytest
import torch

import score_cases as cs
from dynamic_llava_amd import scoring as sc


def _bits(t):
    return torch.as_tensor(t, dtype=torch.float32).reshape(-1).view(torch.int32)


@pytest.mark.parametrize("V", cs.VOCABS)
def test_equal_logits_score_log_v_to_the_bit(V):
    for dtype in cs.DTYPES:
        nll, top1, det = sc.reference_step(torch.full((V,), -3.5).to(dtype), V // 2)
        assert det["M"] == V << sc.S_BITS and top1 == 0
        assert torch.equal(_bits(nll), _bits(torch.log(torch.tensor(float(V), dtype=torch.float32))))


@pytest.mark.parametrize("dtype", cs.DTYPES)
def test_a_dominant_logit_scores_zero_and_the_others_their_distance(dtype):
    row = dict(cs.families(32003, dtype))["dominant"]
    top = int(row.float().argmax())
    nll, top1, det = sc.reference_step(row, top)
    assert top1 == top and det["M"] == 1 << sc.S_BITS and float(nll) == 0.0 and not math.copysign(1.0, float(nll)) < 0
    for other in (0 if top else 1, 32002 if top != 32002 else 32001):
        nll, _, _ = sc.reference_step(row, other)
        assert torch.equal(_bits(nll), _bits(row.float()[top] - row.float()[other]))


def test_a_label_at_minus_infinity_scores_plus_infinity():
    row = torch.randn(320)
    row[7] = float("-inf")
    nll, _, det = sc.reference_step(row, 7)
    assert float(nll) == float("inf") and int(det["mass"][7]) == 0
    assert math.isfinite(float(sc.reference_step(row, 8)[0]))


def test_lowest_index_wins_a_tied_maximum():
    row = torch.zeros(320)
    row[[300, 17, 200]] = 5.0
    assert sc.reference_step(row, 0)[1] == 17
    assert sc.reference_rows(torch.stack([row, row]), torch.tensor([3, -100]))[1].tolist() == [17, -1]


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", cs.VOCABS)
def test_rule_against_float64_log_softmax(V, dtype):
    worst = 0.0
    for name, row in cs.families(V, dtype):
        for label in cs.labels_for(row):
            nll, top1, _ = sc.reference_step(row, label)
            ref, lse, d = cs.truth64(row, label)
            assert top1 == int(torch.nonzero(row.float() == row.float().max())[0])
            if math.isinf(ref):
                assert float(nll) == ref, (name, label)
                continue
            bound = cs.rule_bound(V, lse, d)
            err = abs(float(nll) - ref)
            worst = max(worst, err / bound)
            assert err <= bound, (name, label, float(nll), ref, err, bound)
    print(f"V={V} {dtype}: worst |rule - float64| / bound = {worst:.3f}")


# ---- mutants of the rule: each must be caught on at least one family ----
def _mutant_no_max(row, label):
    x = row.float()
    mass = torch.floor(torch.exp(x).double() * float(2**sc.S_BITS))
    M = torch.where(torch.isfinite(mass), mass, torch.zeros_like(mass)).sum()
    return (torch.log((M * 2.0**-sc.S_BITS).float()) - x[label]).item()


def _mutant_bf16_sum(row, label):
    x = row.float()
    m = x.max()
    s = torch.exp(x - m).to(torch.bfloat16).sum(dtype=torch.bfloat16)
    return ((m - x[label]) + torch.log(s.float())).item()


def _mutant_label_term_dropped(row, label):
    m, _, mass = sc.masses(row)
    M = int(mass.sum()) - int(mass[label])
    return float("nan") if M <= 0 else ((m - row.float()[label]) + sc.lse_of(M)).item()


def _caught(mutant, V=32003):
    hits = []
    for dtype in cs.DTYPES:
        for name, row in cs.families(V, dtype):
            for label in cs.labels_for(row):
                ref, lse, d = cs.truth64(row, label)
                if math.isinf(ref):
                    continue
                got = mutant(row, label)
                if not abs(got - ref) <= cs.rule_bound(V, lse, d):  # (NaN is caught)
                    hits.append((str(dtype), name, label))
    return hits


@pytest.mark.parametrize("mutant", [_mutant_no_max, _mutant_bf16_sum, _mutant_label_term_dropped], ids=["no_max_subtraction", "masses_summed_in_bf16", "label_term_dropped"])
def test_the_float64_bound_catches_the_mutant(mutant):
    hits = _caught(mutant)
    assert hits, "the mutant passes every family"
    print(f"caught on {len(hits)} (family, label) pairs, e.g. {hits[0]}")


def test_the_label_of_the_next_step_is_caught():
    """A sequence scored with labels[step + 1] in the place of labels[step]."""
    V, T = 32000, 4
    rows = torch.stack([r for _, r in cs.families(V, torch.float32)[:T]])
    labels = torch.tensor([5, 31999, 17, 1234])
    good = [float(sc.reference_step(rows[j], labels[j])[0]) for j in range(T)]
    shifted = [float(sc.reference_step(rows[j], labels[(j + 1) % T])[0]) for j in range(T)]
    bad = 0
    for j in range(T):
        ref, lse, d = cs.truth64(rows[j], int(labels[j]))
        assert abs(good[j] - ref) <= cs.rule_bound(V, lse, d)
        bad += not abs(shifted[j] - ref) <= cs.rule_bound(V, lse, d)
    assert bad == T


def _thread_order_sum(w):
    """An fp32 sum the way a 1024-thread workgroup would take it: every thread adds its consecutive entries in index order, then a pairwise tree over the
    threads; every addition rounds to fp32 (elementwise tensor adds: no wider accumulator)."""
    ne = -(-w.shape[0] // 1024)
    t = torch.zeros(1024 * ne, dtype=torch.float32)
    t[: w.shape[0]] = w
    t = t.view(1024, ne)
    acc = torch.zeros(1024, dtype=torch.float32)
    for j in range(ne):
        acc = acc + t[:, j]
    while acc.shape[0] > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def test_the_integer_sum_does_not_depend_on_the_order_and_a_float_sum_does():
    """The rule on a reversed row (label moved along) gives the same bits; lse from fp32 sums taken in index order differs somewhere between the two orders --
    that is what the integer sum buys."""
    float_differs = 0
    for dtype in cs.DTYPES:
        for name, row in cs.families(32003, dtype):
            V = row.shape[0]
            for label in cs.labels_for(row)[:2]:
                a, _, da = sc.reference_step(row, label)
                b, _, db = sc.reference_step(row.flip(0), V - 1 - label)
                assert da["M"] == db["M"] and torch.equal(_bits(a), _bits(b)), (name, label)
            w = torch.exp(row.float() - row.float().max())
            float_differs += not torch.equal(_bits(torch.log(_thread_order_sum(w))), _bits(torch.log(_thread_order_sum(w.flip(0)))))
    assert float_differs > 0


def test_label_validation():
    V = 100
    ok = torch.tensor([[3, 99, 0], [5, -100, -100]])
    assert sc.validate_labels(ok, 2, V).tolist() == [3, 1]
    for bad, batch in ((torch.tensor([[3, -100, 4]]), 1),  # a hole
                       (torch.tensor([[3, 100]]), 1),  # >= V
                       (torch.tensor([[3, -1]]), 1),  # negative and not the marker
                       (torch.tensor([[3, 4]]), 2),  # row count
                       (torch.tensor([[-100, 4]]), 1),  # no label in column 0
                       (torch.tensor([[3, 4]], dtype=torch.int32), 1), (torch.zeros((1, 0), dtype=torch.int64), 1), (torch.tensor([3, 4]), 1)):
        with pytest.raises(ValueError):
            sc.validate_labels(bad, batch, V)


def test_score_validates_before_any_launch_and_forward_names_it():
    """On a box without a GPU nothing can be launched: a ValueError (not a HipOpsError) shows the labels were checked first."""
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM
    from oracle import fixtures as fx

    m = DynamicLlavaLlamaForCausalLM(DynamicLlavaConfig.from_namespace(fx.tiny_config()), with_vision_tower=False)
    m._check_ready = lambda *a, **k: None
    V = m.config.vocab_size
    ids = torch.tensor([[1, 5, -200, 9]])
    for bad in (torch.tensor([[3, -100, 4]]), torch.tensor([[3, V]]), torch.tensor([[3, 4], [5, 6]]), torch.tensor([[-100, 4]])):
        with pytest.raises(ValueError):
            m.score(ids, bad)
    with pytest.raises(NotImplementedError, match="score"):
        m.forward(ids, labels=torch.tensor([[1, 2, 3, 4]]))


def test_library_rejects_bad_arguments():
    from dynamic_llava_amd import hip_ops

    lib = hip_ops.load_library()
    p = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    args = lambda V, labels=p, nll=p, cap=4, logits=p, nxt=p: (logits, hip_ops.DL_BF16, V, V, 1, labels, cap, nll, None, nxt, None, 0, None, None, 0, None, None, None, None)
    assert lib.dl_decode_score(*args(65537)) != 0 and b"65536" in lib.dl_last_error()
    assert lib.dl_decode_score(*args(32000, labels=None)) != 0 and b"labels" in lib.dl_last_error()
    assert lib.dl_decode_score(*args(32000, nll=None)) != 0
    assert lib.dl_decode_score(*args(32000, logits=None)) != 0 and lib.dl_decode_score(*args(32000, nxt=None)) != 0
    assert lib.dl_decode_score(*args(0)) != 0 and lib.dl_decode_score(*args(32000, cap=0)) != 0
