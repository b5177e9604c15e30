"""generate()'s request handling on the CPU: which route a request takes and what it forwards (a characterisation: the routing test needs nothing but the
model class, so it runs on any revision), the one EOS resolver, and the one host loop against a plain restatement driven from a table of logits."""
import pytest
import torch

from dynamic_llava_amd.config import DynamicLlavaConfig
from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM
from oracle import fixtures as fx


class _Device(Exception):
    pass


def _tiny(**cfg_over):
    cfg = fx.tiny_config()
    mcfg = DynamicLlavaConfig.from_namespace(cfg)
    for k, v in cfg_over.items():
        setattr(mcfg, k, v)
    return cfg, mcfg


def _routed(kw):
    """-> (route, greedy, the forwarded keyword names) of generate(ids, **kw): the three route bodies are sentinels, nothing is launched."""
    cfg, mcfg = _tiny()
    m = DynamicLlavaLlamaForCausalLM(mcfg, with_vision_tower=False)
    m._check_ready = lambda *a, **k: None
    m._generate_sample = lambda inputs, images, greedy=False, **k: ("sample", bool(greedy), sorted(k))
    m._generate_on_cache = lambda inputs, images, **k: ("on_cache", True, sorted(k))

    def device(*a, **k):
        raise _Device()

    m._pooled_cache = device
    try:
        return m.generate(torch.tensor([[1, 5, -200, 9]]), image_features=torch.zeros(1, 4, cfg.hidden_size), **kw)
    except _Device:
        return ("device", None, None)


FOUR = [310, 311, 312, 313]
CACHE = object()
ROUTES = [  # (request besides max_new_tokens / image_features, route, greedy, forwarded names besides those two: None = the device loop, which forwards nothing)
    (dict(), "device", None, None),
    (dict(repetition_penalty=1.2), "device", None, None),
    (dict(do_sample=True, seed=3), "device", None, None),
    (dict(do_sample=True), "sample", False, ["do_sample"]),
    (dict(do_sample=True, seed=3, generator=torch.Generator()), "sample", False, ["do_sample", "generator", "seed"]),
    (dict(eos_token_id=FOUR), "sample", True, ["eos_token_id"]),
    (dict(eos_token_id=FOUR, do_sample=False, sync_every=4), "sample", True, ["eos_token_id"]),
    (dict(eos_token_id=FOUR, do_sample=True, seed=1, sync_every=4), "sample", False, ["do_sample", "eos_token_id", "seed", "sync_every"]),
    (dict(past_key_values=CACHE), "on_cache", True, ["past_key_values"]),
    # known defect, kept: the sampled loop never reads past_key_values -- the dialogue is dropped without a word
    (dict(past_key_values=CACHE, do_sample=True), "sample", False, ["do_sample", "past_key_values"]),
    (dict(past_key_values=CACHE, do_sample=True, seed=1), "sample", False, ["do_sample", "past_key_values", "seed"]),
    (dict(no_repeat_ngram_size=99), "sample", True, ["no_repeat_ngram_size"]),
    (dict(no_repeat_ngram_size=99, do_sample=False, sync_every=2), "sample", True, ["no_repeat_ngram_size"]),
    (dict(no_repeat_ngram_size=99, do_sample=True, seed=1), "sample", False, ["do_sample", "no_repeat_ngram_size", "seed"]),
]


@pytest.mark.parametrize("kw,route,greedy,names", ROUTES, ids=[",".join(sorted(r[0])) or "plain" for r in ROUTES])
def test_routing_table(kw, route, greedy, names):
    want = None if names is None else sorted(names + ["image_features", "max_new_tokens"])
    assert _routed(dict(kw, max_new_tokens=2)) == (route, greedy, want)


def test_routing_rejects_an_empty_generation_on_the_device_route():
    with pytest.raises(ValueError):
        _routed(dict(max_new_tokens=0))
    with pytest.raises(ValueError):
        _routed(dict(max_length=3))  # shorter than the prompt
    with pytest.raises(NotImplementedError):
        _routed(dict(max_new_tokens=2, num_beams=2))


@pytest.mark.parametrize("bad", [dict(temperature=-1.0), dict(temperature=float("nan")), dict(top_p=-0.5), dict(top_p=0.0), dict(top_k=-3)], ids=lambda d: ",".join(d))
def test_seeded_sampling_parameters_are_checked_on_whichever_route(bad):
    """A seeded, sampled request is validated before any launch, also when its logits processors are past the device caps and it ends in the host loop."""
    for kw in (dict(), dict(no_repeat_ngram_size=99), dict(repetition_penalty=1.2)):
        with pytest.raises(ValueError):
            _routed(dict(kw, max_new_tokens=2, do_sample=True, seed=1, **bad))


EOS_ROWS = [  # (kwargs, config default, eos_ids, StepMode.eos)
    (dict(eos_token_id=7), 2, (7,), 7),
    (dict(eos_token_id=[7]), 2, (7,), 7),
    (dict(eos_token_id=[]), 2, (), -1),
    (dict(eos_token_id=None), 2, (), -1),
    (dict(), 2, (2,), 2),
    (dict(), [5, 6], (5, 6), (5, 6)),
    (dict(), None, (), -1),
    (dict(eos_token_id=(9, 8, 9)), 2, (9, 8, 9), (9, 8, 9)),  # as given: order and repeats kept
]


@pytest.mark.parametrize("kw,default,ids,step_eos", EOS_ROWS)
def test_eos_is_resolved_in_one_place(kw, default, ids, step_eos):
    from dynamic_llava_amd import request, sampling
    from dynamic_llava_amd.decode import StepMode

    assert request.eos_ids(kw, default) == ids
    _, mcfg = _tiny(eos_token_id=default)
    req = request.parse(dict(kw, max_new_tokens=4, min_new_tokens=9, pad_token_id=3), mcfg)
    assert req.eos == ids and req.route == "device" and req.max_new([5, 7]) == 4
    assert StepMode.of(req, 4) == StepMode(eos=step_eos, pad=3, min_new=4)  # (min_new_tokens is capped at the steps there are)
    assert request.parse(dict(kw, max_length=10), mcfg).max_new([5, 7]) == 3
    assert sampling.device_route(dict(kw, do_sample=True, seed=1), 320, default)
    assert request.parse(dict(kw, bad_words_ids=[[i] for i in ids] + [[1, 2]]), mcfg).rules.bad_words == ((1, 2),)  # a one-token bad word that is an EOS id is dropped


# ---- the host loop ---------------------------------------------------------------------------------------------------------------------------------
def _table(seed=0, B=2, V=16, steps=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((steps, B, V), generator=g) * 3.0


def _restated(tab, max_new, greedy, eos=(), pad=0, min_new=0, penalty=1.0, temperature=1.0, top_k=0, top_p=None, gen=None):
    """The plain loop the two host routes of generate() have always run, on a table of step logits: HF's order -- processors, temperature, the EOS ban of
    min_new_tokens, top-k, top-p, then the pick; pad behind a row's EOS; stop when every row has finished."""
    B = tab.shape[1]
    finished = torch.zeros(B, dtype=torch.bool)
    toks, scores, raw = [], [], []
    for step in range(max_new):
        z = tab[step].clone()
        raw.append(z.clone())
        if penalty != 1.0:
            pt = torch.tensor(penalty, dtype=torch.float32)  # (a tensor: a true fp32 division, not a multiplication by the reciprocal)
            for b in range(B):
                for t in {int(x[b]) for x in toks}:
                    z[b, t] = z[b, t] * pt if z[b, t] < 0 else z[b, t] / pt
        z = z / temperature
        if step < min_new and eos:
            z[:, list(eos)] = float("-inf")
        if top_k > 0:
            z = z.masked_fill(z < torch.topk(z, top_k, dim=-1).values[:, -1:], float("-inf"))
        if top_p is not None and top_p < 1.0:
            sz, si = torch.sort(z, dim=-1, descending=False)
            remove = sz.softmax(dim=-1).cumsum(dim=-1) <= (1.0 - top_p)
            remove[:, -1] = False
            z = z.masked_fill(remove.scatter(1, si, remove), float("-inf"))
        scores.append(z)
        nxt = z.argmax(dim=-1) if greedy else torch.multinomial(z.softmax(dim=-1), 1, generator=gen)[:, 0]
        nxt = torch.where(finished, torch.full_like(nxt, pad), nxt)
        toks.append(nxt)
        for e in eos:
            finished = finished | (nxt == e)
        if eos and bool(finished.all()):
            break
    return toks, scores, raw


def _driven(tab, max_new, greedy, **kw):
    from dynamic_llava_amd import request

    _, mcfg = _tiny()
    req = request.parse(dict(kw, max_new_tokens=max_new), mcfg)
    fed = []

    def advance(nxt):
        fed.append(nxt.clone())
        return tab[len(fed)]

    toks, scores, raw = request.host_loop(tab[0], advance, req, max_new, greedy)
    assert len(fed) == len(toks) - 1 and all(torch.equal(a, b) for a, b in zip(fed, toks))  # every token but the last is fed, once, in order
    return req, toks, scores, raw


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y)
                                    for x, y in zip(a, b))


def _eos_case():
    """Row 0's greedy token of step 1 is made an EOS id; row 1 ends at step 3: pad afterwards, and the loop stops one step before the table ends."""
    tab = _table(3)
    free, _, _ = _restated(tab, 5, True)
    e0, e1 = int(free[1][0]), int(free[3][1])
    assert e0 != e1 and e0 not in [int(t[0]) for t in free[:1]] and e1 not in [int(t[1]) for t in free[:3]] and e1 not in [int(t[0]) for t in free[:2]] and e0 not in [int(t[1]) for t in free[:4]]
    return tab, (e0, e1)


@pytest.mark.parametrize("lp", [False, True], ids=["plain", "logprobs"])
@pytest.mark.parametrize("case", ["greedy", "min_new", "penalty", "eos", "sampled"])
def test_host_loop_is_the_plain_loop(case, lp):
    from dynamic_llava_amd import logprobs

    tab, greedy, kw, ref = _table(1), True, dict(eos_token_id=None), dict()
    if case == "min_new":
        first = [int(t) for t in tab[0].argmax(dim=-1)]  # both rows' first choice is an EOS id: banned for two steps
        kw, ref = dict(eos_token_id=first, min_new_tokens=2, pad_token_id=1), dict(eos=tuple(first), min_new=2, pad=1)
    elif case == "penalty":
        tab[1:] = tab[0]  # the same logits at every step: without the penalty a row repeats its token
        kw, ref = dict(eos_token_id=None, repetition_penalty=1.7), dict(penalty=1.7)
    elif case == "eos":
        tab, eos = _eos_case()
        kw, ref = dict(eos_token_id=list(eos), pad_token_id=15), dict(eos=eos, pad=15)
    elif case == "sampled":
        greedy = False
        kw = dict(eos_token_id=None, do_sample=True, temperature=0.7, top_k=3, top_p=0.8, generator=torch.Generator().manual_seed(11))
        ref = dict(temperature=0.7, top_k=3, top_p=0.8, gen=torch.Generator().manual_seed(11))
    if lp:
        kw.update(return_dict_in_generate=True, output_logprobs=True, top_logprobs=2)
    req, toks, scores, raw = _driven(tab, 5, greedy, **kw)
    want = _restated(tab, 5, greedy, **ref)
    assert _same(toks, want[0]) and _same(scores, want[1])
    if case == "eos":
        assert len(toks) == 4 and [int(t[0]) for t in toks[2:]] == [15, 15]
    elif case == "penalty":
        assert len(toks) == 5 and len({int(t[1]) for t in toks}) > 1 and len({int(t[1]) for t in _restated(tab, 5, True)[0]}) == 1
    elif case == "min_new":
        assert all(int(t[b]) != kw["eos_token_id"][b] for t in toks[:2] for b in range(2))
    # the raw logits are kept only for the log-probabilities, which are read off them
    assert req.n_lp == (2 if lp else -1) and (_same(raw, want[2]) if lp else raw == [])
    if lp:
        seq = torch.stack(toks, dim=1)
        res = logprobs.host_result(raw, seq, req.eos, req.n_lp)
        assert sorted(res) == ["logprobs", "top_logprob_ids", "top_logprobs"] and res["logprobs"].shape == seq.shape and res["top_logprobs"].shape == (*seq.shape, 2)
        assert sorted(logprobs.host_result(raw, seq, req.eos, 0)) == ["logprobs"]
