"""CPU: constrained decoding's rule (dynamic_llava_amd/constraints.py) -- the automaton and its validation, the compiled table, `apply` against the installed
transformers' PrefixConstrainedLogitsProcessor bit for bit, the routes of the new keywords, and the host loop on a table of logits."""
import os
import re

import pytest
import torch

import test_request_cpu as rq  # the host loop's cases and its plain restatement (not edited: imported)
from dynamic_llava_amd import constraints as C
from dynamic_llava_amd import request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 320  # the tiny config's vocabulary


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- construction and validation ---------------------------------------------------------------------------------------------------------------------------
def test_automaton_validation():
    a = C.TokenAutomaton([0, 2, 2], [9, 4], [1, 0], [False, True])
    assert a.edges(0) == [(4, 0), (9, 1)] and a.edges(1) == [] and (a.n_states, a.n_edges) == (2, 2)  # kept sorted by token
    with pytest.raises(ValueError, match="same token"):
        C.TokenAutomaton([0, 2], [4, 4], [0, 0], [True])
    with pytest.raises(ValueError, match="outside"):
        C.TokenAutomaton([0, 1], [4], [1], [True])  # next_state out of range
    with pytest.raises(ValueError, match="outside"):
        C.TokenAutomaton([0, 1], [4], [-1], [True])
    with pytest.raises(ValueError, match="negative"):
        C.TokenAutomaton([0, 1], [-4], [0], [True])
    with pytest.raises(ValueError, match="outside"):
        C.TokenAutomaton([0, 1], [V], [0], [True], vocab_size=V)
    with pytest.raises(ValueError, match="outside"):
        C.compile(C.TokenAutomaton([0, 1], [V], [0], [True]), (2,), vocab_size=V)
    with pytest.raises(ValueError):
        C.TokenAutomaton([0, 2], [4], [0], [True])  # state_ptr does not end at the number of edges
    with pytest.raises(ValueError):
        C.TokenAutomaton([0, 1], [4], [0], [True, False])
    for bad in ([], [[]], [[1], []], "ab", [[1.5]]):
        with pytest.raises(ValueError):
            C.TokenAutomaton.from_choices(bad)
    with pytest.raises(ValueError):
        C.TokenAutomaton.from_allowed([])


def test_compile_validation():
    trie = C.TokenAutomaton.from_choices([[5, 6], [7]])
    with pytest.raises(ValueError, match="no edge"):
        C.compile(trie, ())  # no EOS id: the terminal accepting states are dead ends
    C.compile(trie, (2,))
    with pytest.raises(ValueError, match="no edge"):
        C.compile(C.TokenAutomaton([0, 1, 1], [4], [1], [False, False]), (2,))  # a reachable state that neither accepts nor continues
    C.compile(C.TokenAutomaton([0, 1, 1], [4], [0], [False, False]), (2,))  # the dead state cannot be reached: allowed
    with pytest.raises(ValueError, match="already an edge"):
        C.compile(C.TokenAutomaton.from_choices([[5, 2, 6], [5]]), (2,))  # EOS collides with an edge of an accepting state
    C.compile(C.TokenAutomaton.from_choices([[2, 6]]), (2,))  # EOS as an edge of a state that does not accept: no collision
    with pytest.raises(ValueError, match="min_new_tokens"):
        C.compile(trie, (2,), min_new=1)
    with pytest.raises(ValueError, match="automata for"):
        C.compile([trie, trie], (2,), B=3)
    with pytest.raises(ValueError):
        C.compile([], (2,))
    with pytest.raises(ValueError):
        C.compile([trie, "x"], (2,))
    # a whitelist without EOS ids never ends by itself and is no dead end: the self-loops remain
    t = C.compile(C.TokenAutomaton.from_allowed([9, 3, 3]), ())
    assert t.allowed(0) == [3, 9] and C.advance(t, 0, 9) == 0


def test_request_validation():
    _, mcfg = rq._tiny()
    kw = dict(max_new_tokens=4)
    trie = C.TokenAutomaton.from_choices([[5, 6], [7]])
    forms = dict(constraint=trie, guided_choice=[[5, 6], [7]], allowed_token_ids=[5, 6], prefix_allowed_tokens_fn=lambda b, ids: [5])
    names = sorted(forms)
    for i, a in enumerate(names):
        assert (request.parse(dict(kw, **{a: forms[a]}), mcfg).constraint is None) == (a == "prefix_allowed_tokens_fn")
        for b in names[i + 1:]:
            with pytest.raises(ValueError, match="at most one"):
                request.parse(dict(kw, **{a: forms[a], b: forms[b]}), mcfg)
        with pytest.raises(ValueError, match="min_new_tokens"):
            request.parse(dict(kw, min_new_tokens=1, **{a: forms[a]}), mcfg)
        with pytest.raises(ValueError, match="score"):
            request.parse(dict(kw, _score_labels=torch.zeros((1, 2), dtype=torch.int64), **{a: forms[a]}), mcfg)
    plain = request.parse(dict(kw, constraint=None, guided_choice=None, allowed_token_ids=None, prefix_allowed_tokens_fn=None), mcfg)
    assert plain == request.parse(kw, mcfg) and plain.constraint is None and plain.allowed_fn is None  # None is the request without the keyword
    with pytest.raises(ValueError):
        request.parse(dict(kw, guided_choice=[[5, V]]), mcfg)
    with pytest.raises(ValueError):
        request.parse(dict(kw, allowed_token_ids=[-1]), mcfg)
    with pytest.raises(ValueError):
        request.parse(dict(kw, prefix_allowed_tokens_fn=3), mcfg)
    with pytest.raises(ValueError, match="no edge"):
        request.parse(dict(kw, guided_choice=[[5]], eos_token_id=None), mcfg)
    with pytest.raises(ValueError, match="automata for"):
        request.parse(dict(kw, constraint=[trie, trie]), mcfg, batch=1)


def test_score_refuses_the_keywords():
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM

    _, mcfg = rq._tiny()
    m = DynamicLlavaLlamaForCausalLM(mcfg, with_vision_tower=False)
    ids, labels = torch.tensor([[1, 5, -200, 9]]), torch.tensor([[4, 5]])
    for k, v in dict(constraint=C.TokenAutomaton.from_allowed([4]), guided_choice=[[4]], allowed_token_ids=[4], prefix_allowed_tokens_fn=lambda b, i: [4]).items():
        with pytest.raises(ValueError, match="constraint"):
            m.score(ids, labels, **{k: v})
    with pytest.raises(TypeError):
        m.score(ids, labels, no_such_keyword=1)


# ---- the trie, the merge, the start states -------------------------------------------------------------------------------------------------------------------
def _language(a, limit=8):
    """Every token sequence that leads from state 0 to an accepting state, found by walking the edges (the tries here are acyclic)."""
    out, todo = set(), [(0, ())]
    while todo:
        s, path = todo.pop()
        assert len(path) <= limit
        if a.accepting[s]:
            out.add(path)
        todo += [(n, path + (t,)) for t, n in a.edges(s)]
    return out


def test_trie_has_exactly_the_edges_of_its_choices():
    choices = [[5, 6, 7], [5, 6], [5, 9], [8], [5, 6, 7], [8, 8, 8]]  # a prefix of another choice, a duplicate
    a = C.TokenAutomaton.from_choices(choices, vocab_size=V)
    prefixes = {tuple(c[:i]) for c in choices for i in range(len(c) + 1)}
    assert a.n_states == len(prefixes) and a.n_edges == len(prefixes) - 1  # one node per distinct prefix, one edge into every node but the root
    assert _language(a) == {tuple(c) for c in choices}
    node = {(): 0}
    for p in sorted(prefixes, key=len):
        if p:
            node[p] = dict(a.edges(node[p[:-1]]))[p[-1]]
    assert a.accepting[node[(5, 6)]] and len(a.edges(node[(5, 6)])) == 1  # accepting and with a child
    assert not a.accepting[node[(5,)]] and [t for t, _ in a.edges(node[(5,)])] == [6, 9]
    assert sum(a.accepting) == 5
    # compiled: every accepting state, and only those, takes the EOS ids -- distinct ones once
    t = C.compile(a, (2, 3, 2))
    for p, s in node.items():
        want = sorted({c[len(p)] for c in map(tuple, choices) if len(c) > len(p) and c[: len(p)] == p} | ({2, 3} if a.accepting[s] else set()))
        assert t.allowed(s) == want, p
        assert (C.advance(t, s, 2) == C.DONE and C.advance(t, s, 3) == C.DONE)
    assert t.n_edges == a.n_edges + 2 * 5 and t.eos == (2, 3, 2)


def test_merge_and_start_states():
    a, b = C.TokenAutomaton.from_choices([[5, 6], [7]]), C.TokenAutomaton.from_allowed([9, 10])
    t = C.compile([a, b, a], (2,), B=3, n_return=2)
    assert t.n_states == a.n_states + b.n_states  # an automaton that occurs twice is stored once
    assert t.prompt_start == (0, a.n_states, 0) and t.starts(3) == [0, 0, a.n_states, a.n_states, 0, 0]  # rows b * n .. b * n + n - 1 share prompt b's start
    assert t.allowed(0) == [5, 7] and t.allowed(a.n_states) == [2, 9, 10]
    assert C.advance(t, a.n_states, 9) == a.n_states and C.advance(t, C.advance(t, 0, 5), 6) != C.DONE  # targets moved with their automaton
    with pytest.raises(ValueError):
        t.starts(2)
    one = C.compile(a, (2,), n_return=3)
    assert one.prompt_start == (0,) and one.starts(2) == [0] * 6
    ptr, edges = t.words()
    assert ptr.dtype == torch.int32 and ptr.tolist() == list(t.state_ptr) and edges.shape == (t.n_edges, 2) and edges[:, 0].tolist() == list(t.edge_tok) and edges[:, 1].tolist() == list(t.edge_next)
    # the rule's corners
    assert C.advance(t, C.DONE, 5) == C.DONE and C.advance(t, 0, 6) == C.DONE and C.advance(t, 0, -3) == C.DONE and C.advance(t, 0, 10 ** 6) == C.DONE
    z = torch.randn(V)
    assert torch.equal(_bits(C.apply(t, z, C.DONE)), _bits(z))
    y = C.apply(t, z.to(torch.bfloat16), 0)
    assert y.dtype == torch.float32 and torch.equal(y[[5, 7]], z.to(torch.bfloat16).float()[[5, 7]]) and int(torch.isinf(y).sum()) == V - 2


def test_complete():
    a, b = C.TokenAutomaton.from_choices([[5, 6], [7]]), C.TokenAutomaton.from_allowed([9, 10])
    t = C.compile([a, b], (2,), B=2, n_return=3)
    seq = torch.tensor([[5, 6, 2, 0], [5, 6, 0, 0], [5, 2, 0, 0], [9, 9, 9, 2], [9, 9, 9, 9], [10, 2, 0, 0]])
    assert C.complete(t, seq).tolist() == [True, False, False, True, False, True]  # cut off, or pad met without an edge: not complete
    assert C.walk(t, 0, [5, 6, 2, 0]) == [0, 1, 2, C.DONE, C.DONE]


def test_caps_match_the_header_and_the_binding():
    from dynamic_llava_amd import hip_ops

    hdr = open(os.path.join(ROOT, "include", "dynllava.h")).read()
    assert int(re.search(r"#define\s+DL_CONSTRAIN_MAX_STATES\s+(\d+)", hdr).group(1)) == C.MAX_STATES == hip_ops.CONSTRAIN_MAX_STATES == 4096
    assert int(re.search(r"#define\s+DL_CONSTRAIN_MAX_EDGES\s+(\d+)", hdr).group(1)) == C.MAX_EDGES == hip_ops.CONSTRAIN_MAX_EDGES == 131072
    assert re.search(r"#define\s+DL_CONSTRAIN_DONE\s+\((-?\d+)\)", hdr).group(1) == str(C.DONE)
    assert hip_ops.CONSTRAIN_TABLE_WORDS == 8 + 4097 + 2 * 131072
    assert C.compile(C.TokenAutomaton.from_allowed(list(range(32000))), ()).device_route  # a 32000-token whitelist fits
    blk = hip_ops.constraint_table_write(torch.zeros(hip_ops.CONSTRAIN_TABLE_WORDS, dtype=torch.int32), *C.compile(C.TokenAutomaton.from_choices([[5, 6], [7]]), (2,)).words())
    assert blk[:2].tolist() == [4, 5] and blk[8:13].tolist() == [0, 2, 3, 4, 5] and blk[8 + 4097 : 8 + 4097 + 10].tolist() == [5, 1, 7, 3, 6, 2, 2, -1, 2, -1]


# ---- against the installed transformers ---------------------------------------------------------------------------------------------------------------------
def test_apply_equals_hf_prefix_constrained_processor_bit_for_bit():
    try:
        from transformers import PrefixConstrainedLogitsProcessor
    except ImportError:
        pytest.skip("the installed transformers has no PrefixConstrainedLogitsProcessor")
    g = torch.Generator().manual_seed(4)
    a, b = C.TokenAutomaton.from_choices([[5, 6, 7], [5, 6], [5, 9], [8], [8, 8, 8], [300, 1]]), C.TokenAutomaton.from_allowed([3, 17, 319, 0])
    t = C.compile([a, b, a], (2, 4), B=3)
    starts = t.starts(3)

    def fn(batch_id, ids):  # HF's callable, derived from the same table: walk the row's tokens, return the state's tokens
        s = starts[batch_id]
        for tok in ids.tolist():
            s = C.advance(t, s, tok)
        return t.allowed(s)

    proc = PrefixConstrainedLogitsProcessor(fn, num_beams=1)
    for trial in range(6):
        states, hist = list(starts), torch.zeros((3, 0), dtype=torch.int64)
        for step in range(5):
            if C.DONE in states:  # (HF raises on an empty list: a finished row is not asked -- the host loop does not ask either)
                break
            z = torch.randn((3, V), generator=g) * 4.0
            got = C.apply_rows(t, z, states)
            want = proc(hist, z.clone())
            assert torch.equal(_bits(got), _bits(want)), (trial, step)
            nxt = torch.tensor([t.allowed(s)[int(torch.randint(len(t.allowed(s)), (1,), generator=g))] for s in states])  # a random walk along the edges
            hist = torch.cat([hist, nxt[:, None]], dim=1)
            states = [C.advance(t, s, int(k)) for s, k in zip(states, nxt)]


# ---- the routes -------------------------------------------------------------------------------------------------------------------------------------------------
def _big_trie():
    """More states than the device table holds: a chain."""
    n = C.MAX_STATES + 1
    return C.TokenAutomaton(list(range(n)) + [n - 1], [5] * (n - 1), list(range(1, n)), [False] * (n - 1) + [True])


_FN = lambda b, ids: [5]  # noqa: E731
ROUTES = [  # (request besides max_new_tokens / image_features, route, greedy, forwarded names besides those two: None = the device loop)
    (dict(guided_choice=[[5, 6], [7]]), "device", None, None),
    (dict(allowed_token_ids=[5, 6]), "device", None, None),
    (dict(allowed_token_ids=[t for t in range(V) if t != 2]), "device", None, None),  # (2 is the config's EOS id: an explicit edge with it would collide)
    (dict(constraint=C.TokenAutomaton.from_choices([[5]])), "device", None, None),
    (dict(guided_choice=[[5]], repetition_penalty=1.2), "device", None, None),
    (dict(guided_choice=[[5]], do_sample=True, seed=3), "device", None, None),
    (dict(guided_choice=[[5]], do_sample=True), "sample", False, ["do_sample", "guided_choice"]),
    (dict(constraint=_big_trie()), "sample", True, ["constraint"]),
    (dict(constraint=_big_trie(), do_sample=False, sync_every=4), "sample", True, ["constraint"]),
    (dict(constraint=_big_trie(), do_sample=True, seed=1), "sample", False, ["constraint", "do_sample", "seed"]),
    (dict(prefix_allowed_tokens_fn=_FN), "sample", True, ["prefix_allowed_tokens_fn"]),
    (dict(prefix_allowed_tokens_fn=_FN, do_sample=True, seed=1), "sample", False, ["do_sample", "prefix_allowed_tokens_fn", "seed"]),
    (dict(guided_choice=[[5]], past_key_values=rq.CACHE), "on_cache", True, ["guided_choice", "past_key_values"]),
    (dict(prefix_allowed_tokens_fn=_FN, past_key_values=rq.CACHE), "on_cache", True, ["past_key_values", "prefix_allowed_tokens_fn"]),
    (dict(guided_choice=[[5]], no_repeat_ngram_size=99), "sample", True, ["guided_choice", "no_repeat_ngram_size"]),
]


@pytest.mark.parametrize("kw,route,greedy,names", ROUTES + rq.ROUTES, ids=[",".join(sorted(r[0])) or "plain" for r in ROUTES + rq.ROUTES])
def test_extended_routing_table(kw, route, greedy, names):
    want = None if names is None else sorted(names + ["image_features", "max_new_tokens"])
    assert rq._routed(dict(kw, max_new_tokens=2)) == (route, greedy, want)
    _, mcfg = rq._tiny()
    if "past_key_values" not in kw:
        req = request.parse(dict(kw, max_new_tokens=2), mcfg)
        assert req.route == {"device": "device", "sample": "host_greedy" if greedy else "host_sample"}[route]
        from dynamic_llava_amd.decode import StepMode

        assert StepMode.of(req, 2).constrained == (req.constraint is not None)


def test_past_the_edge_cap_takes_the_host_route():
    _, mcfg = rq._tiny()
    # 420 states of 319 edges: within MAX_STATES, past MAX_EDGES
    n, toks = 420, [t for t in range(V) if t != 2]
    a = C.TokenAutomaton([i * len(toks) for i in range(n + 1)], toks * n, [min(i + 1, n - 1) for i in range(n) for _ in toks], [True] * n)
    req = request.parse(dict(constraint=a, max_new_tokens=2), mcfg)
    assert req.constraint.n_states <= C.MAX_STATES and req.constraint.n_edges > C.MAX_EDGES and req.route == "host_greedy"


# ---- the host loop ------------------------------------------------------------------------------------------------------------------------------------------------
def _driven(tab, max_new, greedy, **kw):
    _, mcfg = rq._tiny()
    req = request.parse(dict(kw, max_new_tokens=max_new), mcfg, batch=tab.shape[1])
    fed = []

    def advance(nxt):
        fed.append(nxt.clone())
        return tab[len(fed)]

    toks, scores, raw = request.host_loop(tab[0], advance, req, max_new, greedy)
    return req, toks, scores


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
def test_host_loop_emits_only_walks_of_the_automaton(greedy):
    EOS, PAD = 15, 1
    choices = [[3, 4, 5], [3, 4], [6], [7, 8, 9, 10, 11, 12, 13]]  # V = 16 in the table of logits
    a = C.TokenAutomaton.from_choices(choices)
    for seed in range(4):
        tab = rq._table(seed, B=3, V=16, steps=6)
        more = {} if greedy else dict(do_sample=True, temperature=1.5, generator=torch.Generator().manual_seed(seed))
        req, toks, scores = _driven(tab, 6, greedy, guided_choice=choices, eos_token_id=EOS, pad_token_id=PAD, **more)
        seq = torch.stack(toks, dim=1)
        t = req.constraint
        for b, row in enumerate(seq.tolist()):
            states = C.walk(t, 0, row)
            end = row.index(EOS) if EOS in row else len(row)
            assert row[end + 1:] == [PAD] * (len(row) - end - 1), row  # pad behind EOS
            said = row[:end]
            assert all(s != C.DONE for s in states[: end + 1]), (row, states)  # every token up to EOS follows an edge
            if end < len(row):  # EOS exactly from an accepting state: what was said is one of the choices
                assert said in choices, row
            else:  # cut off by max_new_tokens inside the long choice
                assert said == choices[3][: len(row)], row
            for j in range(min(end + 1, len(row))):  # the scores: -inf exactly off the state's edges
                assert (scores[j][b] > float("-inf")).nonzero().flatten().tolist() == t.allowed(states[j]), (b, j)
        assert C.complete(t, seq).tolist() == [EOS in r for r in seq.tolist()]


def test_host_loop_callable_form_equals_the_automaton_form():
    EOS, PAD = 15, 1
    choices = [[3, 4, 5], [3, 4], [6], [7, 8, 9]]
    for seed in range(3):
        tab = rq._table(seed + 10, B=3, V=16, steps=6)
        kw = dict(eos_token_id=EOS, pad_token_id=PAD, repetition_penalty=1.3)
        req, toks, scores = _driven(tab, 6, True, guided_choice=choices, **kw)
        t, calls = req.constraint, []

        def fn(b, ids):
            calls.append((b, tuple(ids.shape), ids.dtype))
            s = 0
            for tok in ids.tolist():
                s = C.advance(t, s, tok)
            return t.allowed(s)

        req2, toks2, scores2 = _driven(tab, 6, True, prefix_allowed_tokens_fn=fn, **kw)
        assert req2.constraint is None and req2.allowed_fn is fn and req2.route == "host_greedy"
        assert rq._same(toks, toks2) and rq._same(scores, scores2)
        assert all(0 <= b < 3 and len(shape) == 1 and shape[0] < len(toks2) and dt == torch.int64 for b, shape, dt in calls)
        assert calls[:3] == [(0, (0,), torch.int64), (1, (0,), torch.int64), (2, (0,), torch.int64)]  # called with the tokens emitted in this call: none at step 0


@pytest.mark.parametrize("lp", [False, True], ids=["plain", "logprobs"])
@pytest.mark.parametrize("case", ["greedy", "min_new", "penalty", "eos", "sampled"])
def test_host_loop_without_the_keywords_is_unchanged(case, lp):
    """tests/test_request_cpu.py's cases, run through its own driver and restatement, with the keywords absent and with all four None."""
    rq.test_host_loop_is_the_plain_loop(case, lp)
    tab, greedy, kw, ref = rq._table(1), True, dict(eos_token_id=None), dict()
    if case == "min_new":
        first = [int(t) for t in tab[0].argmax(dim=-1)]
        kw, ref = dict(eos_token_id=first, min_new_tokens=2, pad_token_id=1), dict(eos=tuple(first), min_new=2, pad=1)
    elif case == "penalty":
        tab[1:] = tab[0]
        kw, ref = dict(eos_token_id=None, repetition_penalty=1.7), dict(penalty=1.7)
    elif case == "eos":
        tab, eos = rq._eos_case()
        kw, ref = dict(eos_token_id=list(eos), pad_token_id=15), dict(eos=eos, pad=15)
    elif case == "sampled":
        greedy = False
        kw = dict(eos_token_id=None, do_sample=True, temperature=0.7, top_k=3, top_p=0.8, generator=torch.Generator().manual_seed(11))
        ref = dict(temperature=0.7, top_k=3, top_p=0.8, gen=torch.Generator().manual_seed(11))
    if lp:
        kw.update(return_dict_in_generate=True, output_logprobs=True, top_logprobs=2)
    req, toks, scores, raw = rq._driven(tab, 5, greedy, constraint=None, guided_choice=None, allowed_token_ids=None, prefix_allowed_tokens_fn=None, **kw)
    want = rq._restated(tab, 5, greedy, **ref)
    assert req.constraint is None and req.allowed_fn is None and rq._same(toks, want[0]) and rq._same(scores, want[1])
