"""CPU: the guidance rule (dynamic_llava_amd/guidance.py) against the installed transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor, its place in front of
the other processors, the cutoff, the keywords' validation in request.parse, and the host loop on two tables of logits (no device: nothing is launched).

Truth.  The HF processor with a stubbed get_unconditional_logits, fed float64.  The rule must be no further from it than HF's own fp32 evaluation on the same inputs
(largest error per vocabulary size, lattice and scale), and every element must lie within guidance.error_bound, which DESIGN.md section 4p derives from logprobs.py's two
operations and the three of the rule's step 2."""
import os
import re

import pytest
import torch

import test_request_cpu as rq  # _tiny, _table (not edited: imported)
from dynamic_llava_amd import constraints as C
from dynamic_llava_amd import guidance as G
from dynamic_llava_amd import request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS, SCALES = (5, 257, 32000), (0.0, 0.5, 1.5, 3.0)
LATTICES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _rows(V, lattice, seed, n=2):
    """n pairs of rows on the 16-bit lattice: the conditional row and a negative row that differs from it as a language prior differs (a shifted, re-noised copy)."""
    g = torch.Generator().manual_seed(1000 * seed + V)
    c = torch.randn((n, V), generator=g) * 4.0
    u = 0.7 * c + torch.randn((n, V), generator=g) * 2.0
    return c.to(LATTICES[lattice]).float(), u.to(LATTICES[lattice]).float()


def _hf(c, u, s, dtype):
    """HF's processor on one pair of batches, evaluated in `dtype`; the unconditional forward is stubbed with the negative rows."""
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor

    p = UnbatchedClassifierFreeGuidanceLogitsProcessor(s, model=None)
    p.get_unconditional_logits = lambda input_ids: u.to(dtype)[:, None, :]
    return p(torch.zeros((c.shape[0], 1), dtype=torch.long), c.to(dtype))


_CASES = {}


def _case(V, lattice, s):
    if (V, lattice, s) not in _CASES:
        c, u = _rows(V, lattice, seed=3)
        _CASES[(V, lattice, s)] = (c, u, _hf(c, u, s, torch.float64), _hf(c, u, s, torch.float32), G.apply(c, u, s))
    return _CASES[(V, lattice, s)]


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("lattice", list(LATTICES))
@pytest.mark.parametrize("V", VS)
def test_rule_is_no_further_from_the_truth_than_hf_fp32(V, lattice, s):
    c, u, truth, hf32, rule = _case(V, lattice, s)
    assert rule.dtype == torch.float32 and rule.shape == c.shape
    e_rule, e_hf = float((rule.double() - truth).abs().max()), float((hf32.double() - truth).abs().max())
    print(f"s={s} V={V} {lattice}: rule {e_rule:.3e}  hf fp32 {e_hf:.3e}")
    assert e_rule <= e_hf, (V, lattice, s, e_rule, e_hf)


@pytest.mark.parametrize("lattice", list(LATTICES))
@pytest.mark.parametrize("V", VS)
def test_every_element_within_the_derived_bound(V, lattice):
    for s in SCALES:
        c, u, truth, _, rule = _case(V, lattice, s)
        lc, lu = torch.log_softmax(c.double(), dim=-1), torch.log_softmax(u.double(), dim=-1)
        bound = G.error_bound(s, lc, lu)
        err = (rule.double() - truth).abs()
        assert bool((err <= bound).all()), (V, lattice, s, float((err / bound).max()))
        print(f"V={V} {lattice} s={s}: worst err / bound = {float((err / bound).max()):.3f}")


def test_the_rule_is_logprobs_step_2_and_three_rounded_operations():
    from dynamic_llava_amd import logprobs

    c, u = _rows(257, "bf16", seed=5, n=1)
    toks = list(range(257))
    lc, lu = logprobs.reference_row_tokens(c[0], toks)[0], logprobs.reference_row_tokens(u[0], toks)[0]
    s = torch.tensor(1.5, dtype=torch.float32)
    d = lc - lu
    p = s * d
    assert torch.equal(G.guide_row(c[0], u[0], 1.5), p + lu)  # the same bits output_logprobs reports, then sub, mul, add
    assert torch.equal(G.guide_row(c[0], u[0], 1.5, lse=(G.row_logprobs(c[0])[1], G.row_logprobs(u[0])[1])), p + lu)  # ... also with the two lse handed in
    assert torch.equal(G.guide_row(c[0], u[0], 0.0), (torch.zeros(()) * d) + lu)


def test_minus_inf_in_either_row_is_minus_inf():
    c, u = _rows(257, "bf16", seed=6, n=1)
    c, u = c[0].clone(), u[0].clone()
    c[3], u[9], c[11], u[11] = float("-inf"), float("-inf"), float("-inf"), float("-inf")
    for s in SCALES:
        g = G.guide_row(c, u, s)
        assert torch.isneginf(g[[3, 9, 11]]).all() and not torch.isnan(g).any()
        keep = torch.ones(257, dtype=torch.bool)
        keep[[3, 9, 11]] = False
        assert torch.isfinite(g[keep]).all()


def test_order_guidance_first_then_hf_processor_list():
    """The guided row goes through logits_rules and the constraint in HF's order: equal to HF's own processors run on the rule's output, bit for bit."""
    from transformers.generation.logits_process import (LogitsProcessorList, NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor, PrefixConstrainedLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)

    V, EOS = 257, 2
    _, mcfg = rq._tiny()
    c, u = _rows(V, "bf16", seed=7)
    hist = [[5, 9, 5], [11, 11, 9]]  # (inside the whitelist: a token without an edge would end the walk)
    allowed = [5, 9, 11, 40, EOS]  # (our whitelist takes the request's EOS ids by itself)
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[[40]], allowed_token_ids=allowed[:-1], eos_token_id=EOS, max_new_tokens=8)
    mcfg.vocab_size = V
    req = request.parse(kw, mcfg, batch=2)
    g = G.apply(c, u, 1.5)
    ours = req.rules.apply(g, torch.tensor(hist))
    ours = C.apply_rows(req.constraint, ours, [C.advance(req.constraint, C.advance(req.constraint, C.advance(req.constraint, s0, h[0]), h[1]), h[2])
                                                for s0, h in zip(req.constraint.starts(2), hist)])
    hf = LogitsProcessorList([RepetitionPenaltyLogitsProcessor(penalty=1.3), NoRepeatNGramLogitsProcessor(2), NoBadWordsLogitsProcessor([[40]], eos_token_id=[EOS]),
                              PrefixConstrainedLogitsProcessor(lambda b, ids: allowed, 1)])(torch.tensor(hist), g.clone())
    assert torch.equal(ours.view(torch.int32), hf.view(torch.int32))


@pytest.mark.parametrize("beta", [0.001, 0.1, 0.5, 0.999])
def test_cutoff_keeps_exactly_the_plausible_set(beta):
    import math
    import struct

    c, u = _rows(32000, "bf16", seed=8, n=1)
    c, u = c[0], u[0]
    g, free = G.guide_row(c, u, 2.0, beta), G.guide_row(c, u, 2.0)
    # independently: the conditional log-probabilities through logprobs.py, the threshold from -lse_c and fp32(log beta)
    from dynamic_llava_amd import logprobs

    lc = logprobs.reference_row_tokens(c, list(range(c.shape[0])))[0]
    lb = torch.tensor(struct.unpack("<f", struct.pack("<f", math.log(beta)))[0], dtype=torch.float32)
    thr = lc.max() + lb  # (-lse_c is the maximum's own log-probability)
    kept = lc >= thr
    assert torch.equal(torch.isfinite(g), kept) and torch.equal(g[kept], free[kept])
    assert bool(kept[int(c.argmax())]) and 1 <= int(kept.sum()) < c.shape[0]


def test_cutoff_ties_at_the_threshold_are_both_kept_and_the_argmax_survives_every_beta():
    c = torch.tensor([4.0, 1.0, 1.0, -3.0, 0.5]).bfloat16().float()
    u = torch.tensor([0.0, 2.0, -1.0, 1.0, 0.5]).bfloat16().float()
    lc, lse = G.row_logprobs(c)
    # a beta whose threshold is exactly the tied entries' log-probability: search the fp32 log_beta that lands on it
    import math

    target = float(lc[1] + lse)  # lc(1) - (-lse)
    beta = math.exp(target)
    for b in (beta, math.nextafter(beta, 0.0), math.nextafter(beta, 1.0)):
        g = G.guide_row(c, u, 1.5, b)
        assert bool(torch.isfinite(g[1])) == bool(torch.isfinite(g[2]))  # tied entries share their fate
    thr_hits = [b for b in (beta, math.nextafter(beta, 0.0), math.nextafter(beta, 1.0)) if float((-lse) + torch.tensor(G.log_beta(b))) == float(lc[1])]
    assert thr_hits, "no beta lands the threshold on the tie"
    g = G.guide_row(c, u, 1.5, thr_hits[0])
    assert torch.isfinite(g[1]) and torch.isfinite(g[2]) and torch.isneginf(g[3])
    for b in (1e-30, 1e-6, 0.3, 0.9, 0.999999, 1.0 - 2**-53):
        assert torch.isfinite(G.guide_row(c, u, 3.0, b)[0])


def test_refusals_and_the_neutral_keywords():
    _, mcfg = rq._tiny()
    neg, kw = torch.tensor([[1, 5, 9]]), dict(max_new_tokens=4)
    plain = request.parse(kw, mcfg)
    assert plain.guidance is None
    for neutral in (dict(guidance_scale=None), dict(guidance_scale=1.0), dict(guidance_scale=1), dict(guidance_scale=1.0, negative_prompt_ids=neg), dict(guidance_cutoff=None)):
        assert request.parse(dict(kw, **neutral), mcfg) == plain, neutral
    req = request.parse(dict(kw, guidance_scale=2.0, negative_prompt_ids=neg, guidance_cutoff=0.1), mcfg)
    assert req.guidance == (2.0, 0.1) and req.route == "device"
    assert request.parse(dict(kw, guidance_scale=0, negative_images=torch.zeros(1)), mcfg).guidance == (0.0, None)
    from dynamic_llava_amd.decode import StepMode

    assert StepMode.of(req, 4).guided is True and StepMode.of(plain, 4).guided is False and StepMode().guided is False
    for bad in (-0.5, float("nan"), float("inf"), "2", True):
        with pytest.raises(ValueError, match="guidance_scale"):
            request.parse(dict(kw, guidance_scale=bad, negative_prompt_ids=neg), mcfg)
    with pytest.raises(ValueError, match="negative_prompt_ids= or negative_images="):
        request.parse(dict(kw, guidance_scale=2.0), mcfg)
    for bad in (0.0, 1.0, -1, 2, "0.5", True):
        with pytest.raises(ValueError, match="guidance_cutoff"):
            request.parse(dict(kw, guidance_scale=2.0, negative_prompt_ids=neg, guidance_cutoff=bad), mcfg)
    for off in (dict(), dict(guidance_scale=1.0), dict(guidance_scale=None)):
        with pytest.raises(ValueError, match="guidance_cutoff needs"):
            request.parse(dict(kw, guidance_cutoff=0.5, **off), mcfg)
    with pytest.raises(ValueError, match="negative_prompt_attention_mask"):
        request.parse(dict(kw, guidance_scale=2.0, negative_images=torch.zeros(1), negative_prompt_attention_mask=torch.ones((1, 3))), mcfg)
    with pytest.raises(ValueError, match="int64"):
        request.parse(dict(kw, guidance_scale=2.0, negative_prompt_ids=[[1, 2]]), mcfg)
    with pytest.raises(NotImplementedError, match="guidance_scale with num_return_sequences"):
        request.parse(dict(kw, guidance_scale=2.0, negative_prompt_ids=neg, num_return_sequences=2, do_sample=True, seed=1), mcfg)
    with pytest.raises(NotImplementedError, match="guidance_scale with past_key_values"):
        request.parse(dict(kw, guidance_scale=2.0, negative_prompt_ids=neg, past_key_values=object()), mcfg)
    labels = torch.zeros((1, 2), dtype=torch.int64)
    for k, v in (("guidance_scale", 2.0), ("negative_prompt_ids", neg), ("negative_images", torch.zeros(1)), ("guidance_cutoff", 0.5), ("negative_prompt_attention_mask", torch.ones((1, 3)))):
        with pytest.raises(ValueError, match="score"):
            request.parse(dict(kw, _score_labels=labels, **{k: v}), mcfg)


def test_score_refuses_the_keywords_before_any_launch():
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM

    _, mcfg = rq._tiny()
    m = DynamicLlavaLlamaForCausalLM(mcfg, with_vision_tower=False)
    ids, labels = torch.tensor([[1, 5, -200, 9]]), torch.tensor([[4, 5]])
    for k, v in (("guidance_scale", 2.0), ("negative_prompt_ids", ids), ("negative_images", torch.zeros(1)), ("guidance_cutoff", 0.5)):
        with pytest.raises(ValueError, match="score\\(\\) takes no guidance"):
            m.score(ids, labels, **{k: v})


def test_negative_inputs_defaults_and_broadcast():
    ids = torch.tensor([[1, -200, 7], [1, -200, 8]])
    images, other = torch.zeros((2, 3)), torch.ones((2, 3))
    n, m, im, ft = G.negative_inputs(dict(negative_images=other), ids, images, -200)  # VCD's form: same text, another image
    assert n is ids and m is None and im is other and ft is None
    n, m, im, ft = G.negative_inputs(dict(negative_prompt_ids=torch.tensor([[1, 7, 9, 9]])), ids, images, -200)  # text-only, broadcast
    assert n.shape == (2, 4) and n.tolist() == [[1, 7, 9, 9]] * 2 and im is None and ft is None
    n, m, im, ft = G.negative_inputs(dict(negative_prompt_ids=torch.tensor([[1, -200, 9]])), ids, images, -200)  # a placeholder takes the request's images
    assert n.shape == (2, 3) and im is images
    with pytest.raises(ValueError, match="rows"):
        G.negative_inputs(dict(negative_prompt_ids=torch.zeros((3, 2), dtype=torch.int64)), ids, images, -200)


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
def test_host_loop_feeds_both_streams_the_same_token(greedy):
    _, mcfg = rq._tiny()
    tab_c, tab_u, max_new = rq._table(1), rq._table(2), 5
    kw = dict(guidance_scale=1.5, negative_prompt_ids=torch.tensor([[1, 2]]), guidance_cutoff=0.05, eos_token_id=None, max_new_tokens=max_new, repetition_penalty=1.2)
    if not greedy:
        kw.update(do_sample=True, generator=torch.Generator().manual_seed(4))
    req = request.parse(kw, mcfg, batch=tab_c.shape[1])
    fed_c, fed_u = [], []

    def adv(tab, fed):
        def advance(nxt):
            fed.append(nxt.clone())
            return tab[len(fed)]
        return advance

    toks, scores, _ = request.host_loop(tab_c[0], adv(tab_c, fed_c), req, max_new, greedy, negative=(tab_u[0], adv(tab_u, fed_u)))
    assert len(fed_c) == len(fed_u) == max_new - 1 and all(torch.equal(a, b) and torch.equal(a, t) for a, b, t in zip(fed_c, fed_u, toks))
    for j in range(max_new):  # every step's scores: the rule on the two tables' rows, then the processors
        g = G.apply(tab_c[j], tab_u[j], 1.5, 0.05)
        z = req.rules.apply(g, torch.stack(toks[:j], dim=1) if j else [[]] * 2)
        assert torch.equal(scores[j], z / 1.0)
        if greedy:
            assert torch.equal(toks[j], z.argmax(dim=-1))


def test_header_binding_and_library_agree_on_the_new_entries():
    from ctypes import c_int, c_int64, c_void_p

    from dynamic_llava_amd import hip_ops

    hdr = open(os.path.join(ROOT, "include", "dynllava.h")).read()
    kinds = {"int": c_int, "int64_t": c_int64}
    for name in ("dl_kv_place", "dl_logits_guide", "dl_pair_follow"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, f"include/dynllava.h does not declare {name}"
        want = [c_void_p if "*" in a else kinds[a.split()[0]] for a in (x.strip() for x in m.group(1).split(","))]
        res, args = hip_ops.SIGNATURES[name]
        assert res is c_int and args == want, name
        if os.path.exists(hip_ops.LIB_PATH):
            assert hasattr(hip_ops.load_library(), name)
    words = hip_ops.guide_params_words(1.5, 0.25)
    assert words.dtype == torch.int32 and words.numel() == 8 and words[:3].view(torch.float32)[0] == 1.5 and int(words[1]) == 1
    assert float(words[2:3].view(torch.float32)) == G.log_beta(0.25) and int(hip_ops.guide_params_words(2.0)[1]) == 0
