"""GPU, model level: generate(constraint= / guided_choice= / allowed_token_ids= / prefix_allowed_tokens_fn=) on the tiny config of oracle/fixtures.py.

The replay tests are exact and compare no routes: every generated token must be the lowest-index argmax of constraints.apply(the step's RAW logits, as
output_logits reports them, the state replayed on the host).  The choices are made of the tokens the unconstrained first step ranks lowest, so the
unconstrained run never says one of them: a build that ignores the keyword fails."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import constraints as C  # noqa: E402
from dynamic_llava_amd import logits_rules  # noqa: E402
from dynamic_llava_amd.decode import StepMode  # noqa: E402

T, PAD, EOS = 8, 1, 2
_MODELS, _FREE = {}, {}


@pytest.fixture(autouse=True, scope="module")
def _release_models():
    yield
    _MODELS.clear()
    _FREE.clear()
    gc.collect()
    torch.cuda.synchronize()


def _model(dtype):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from oracle import fixtures as fx
    from oracle.make_golden import SD_SEED

    if dtype not in _MODELS:
        cfg = fx.tiny_config()  # text predictor on: rows evict
        sd = fx.make_state_dict(cfg, seed=SD_SEED, predictor_gain=50.0)
        clip = fx.build_clip(cfg, seed=1, dtype=dtype)
        _MODELS[dtype] = (cfg, build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg), sd, clip.state_dict(), dtype=dtype, device="cuda"))
    return _MODELS[dtype]


def _inputs(cfg, B, dtype):
    from oracle import fixtures as fx

    return dict(inputs=torch.stack([fx.make_prompt(cfg, 5, 7, seed=10 + b) for b in range(B)]).cuda(), images=fx.make_images(cfg, B, seed=3).to(dtype).cuda())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_logits(a, b):
    return len(a) == len(b) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _base(dtype, B):
    """-> (cfg, model, the request without the keywords, its result (computed once and left unchanged), six tokens the unconstrained first step ranks lowest in every row)."""
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=T, eos_token_id=EOS, pad_token_id=PAD, return_dict_in_generate=True, output_logits=True)
    if (dtype, B) not in _FREE:
        free = model.generate(**kw)
        best = free["logits"][0].float().max(dim=0).values.cpu()  # a token's best rank over the rows
        best[[0, PAD, EOS]] = float("inf")
        low = torch.argsort(best)[:6].tolist()
        _FREE[(dtype, B)] = ({k: (v.cpu() if torch.is_tensor(v) else tuple(x.cpu() for x in v)) for k, v in free.items() if k in ("sequences", "logits")}, low)
    free, low = _FREE[(dtype, B)]
    return cfg, model, kw, free, low


def _choices(low):
    a, b, c, d, e, f = low
    return [[a, b], [a], [c, d, e], [f, a]]  # one choice is a prefix of another


def _argmax(z):
    return int((z == z.max()).nonzero()[0])


def _replay(table, res, B, rules=None):
    """Every token of the result is the lowest-index argmax of the rule on the step's raw logits; -> the rows' tokens up to and including their EOS."""
    seq, raw = res["sequences"].cpu(), [z.cpu() for z in res["logits"]]
    assert len(raw) == seq.shape[1]
    starts, said = table.starts(B // table.n_return), []
    for b in range(seq.shape[0]):
        s, row, done = starts[b], seq[b].tolist(), False
        for j, tok in enumerate(row):
            if done:
                assert tok == PAD, (b, row)
                continue
            z = raw[j][b]
            if rules is not None:
                z = rules.apply(z[None], [row[:j]])[0]
            z = C.apply(table, z, s)
            assert tok == _argmax(z), (b, j, row, tok, _argmax(z))
            if "scores" in res:
                assert torch.equal(_bits(res["scores"][j][b].cpu()), _bits(z)), (b, j)
            s, done = C.advance(table, s, tok), tok == EOS
        said.append(row[: row.index(EOS) + 1] if EOS in row else row)
    return said


@pytest.mark.parametrize("B", [1, 4], ids=["b1_gemv", "b4_gemm"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_replay_and_the_ignored_keyword(dtype, B):
    cfg, model, kw, free, low = _base(dtype, B)
    choices = _choices(low)
    # the unconstrained request says none of the choices: no row even starts like one
    assert all(int(free["sequences"][b, 0]) not in (low[0], low[2], low[5]) for b in range(B)), (free["sequences"].tolist(), low)
    res = model.generate(**kw, guided_choice=choices, output_scores=True)
    torch.cuda.synchronize()
    model.check_device_errors()
    assert model._mode.constrained is True and model._mode.processed is False
    table = C.compile(C.TokenAutomaton.from_choices(choices), (EOS,), B)
    said = _replay(table, res, B)
    assert all(r[-1] == EOS and r[:-1] in choices for r in said), said  # one of the choices, EOS, then pad
    assert res["sequences"].shape[1] == max(len(r) for r in said)  # trimmed where the last row finishes
    assert res["constraint_complete"].dtype == torch.bool and res["constraint_complete"].tolist() == [True] * B
    assert _same_logits([z.cpu() for z in res["logits"][:1]], free["logits"][:1])  # `logits` stay the model's own: the first step's are the unconstrained run's
    plain = model.generate(**{k: v for k, v in kw.items() if k not in ("return_dict_in_generate", "output_logits")}, guided_choice=choices)
    assert torch.equal(plain.cpu(), res["sequences"].cpu())  # chunks of captured steps: the same tokens as step by step


def test_routes_agree():
    """fp32: graph and eager runs, constraint= with the same trie, the host route through prefix_allowed_tokens_fn built from the same automaton, and the host route
    past MAX_STATES all return the device route's tokens."""
    dtype, B = torch.float32, 4
    cfg, model, kw, free, low = _base(dtype, B)
    choices = _choices(low)
    dev = model.generate(**kw, guided_choice=choices)
    try:
        model.use_hip_graph = False
        eager = model.generate(**kw, guided_choice=choices)
    finally:
        model.use_hip_graph = True
    assert torch.equal(eager["sequences"], dev["sequences"]) and _same_logits(eager["logits"], dev["logits"])
    trie = C.TokenAutomaton.from_choices(choices)
    same = model.generate(**kw, constraint=trie)
    assert torch.equal(same["sequences"], dev["sequences"]) and _same_logits(same["logits"], dev["logits"])
    table, calls = C.compile(trie, (EOS,), B), []

    def fn(b, ids):
        calls.append((b, ids.shape[0]))
        s = 0
        for tok in ids.tolist():
            s = C.advance(table, s, tok)
        return table.allowed(s)

    hk = {k: v for k, v in kw.items() if k != "output_logits"}
    host = model.generate(**hk, prefix_allowed_tokens_fn=fn)
    assert torch.equal(host["sequences"].cpu(), dev["sequences"].cpu()) and "constraint_complete" not in host
    assert calls[:B] == [(b, 0) for b in range(B)] and all(0 <= b < B for b, _ in calls)
    # past MAX_STATES: the same trie followed by states no row can reach -- the host route, the same rule
    n = trie.n_states
    big = C.TokenAutomaton(trie.state_ptr + [trie.n_edges + i + 1 for i in range(C.MAX_STATES)], trie.edge_tok + [5] * C.MAX_STATES,
                           trie.edge_next + [n + i for i in range(C.MAX_STATES)], trie.accepting + [False] * C.MAX_STATES)
    from dynamic_llava_amd import request

    assert request.parse(dict(constraint=big, max_new_tokens=T, eos_token_id=EOS), model.config).route == "host_greedy"
    past = model.generate(**hk, constraint=big)
    assert torch.equal(past["sequences"].cpu(), dev["sequences"].cpu()) and past["constraint_complete"].tolist() == [True] * B


def test_max_new_tokens_cuts_a_row_off():
    dtype, B = torch.bfloat16, 4
    cfg, model, kw, free, low = _base(dtype, B)
    choices = [low[:3], low[2:5]]  # three tokens each
    for n in (1, 2):
        res = model.generate(**dict(kw, max_new_tokens=n), guided_choice=choices)
        assert res["sequences"].shape == (B, n) and res["constraint_complete"].tolist() == [False] * B
        assert all(r in [c[:n] for c in choices] for r in res["sequences"].tolist())
    res = model.generate(**dict(kw, max_new_tokens=4), guided_choice=choices)
    assert res["constraint_complete"].tolist() == [True] * B and all(r[:3] in choices and r[3] == EOS for r in res["sequences"].tolist())


def test_processors_run_first_the_constraint_second():
    """allowed_token_ids with repetition_penalty and bad_words_ids: `scores` are constraints.apply(logits_rules(raw logits, the row's tokens), state), bit for bit,
    and the banned id of the whitelist is never said."""
    dtype, B = torch.bfloat16, 4
    cfg, model, kw, free, low = _base(dtype, B)
    allowed, banned = low[:4], low[3]
    kw = dict(kw, eos_token_id=None, output_scores=True)
    res = model.generate(**kw, allowed_token_ids=allowed, repetition_penalty=1.5, bad_words_ids=[[banned]])
    assert model._mode.constrained and model._mode.processed
    table = C.compile(C.TokenAutomaton.from_allowed(allowed), (), B)
    rules = logits_rules.normalize(dict(repetition_penalty=1.5, bad_words_ids=[[banned]]), cfg.vocab_size)
    said = _replay(table, res, B, rules)
    assert res["sequences"].shape == (B, T) and all(set(r) <= set(allowed) - {banned} for r in said), said
    assert res["constraint_complete"].tolist() == [False] * B  # a whitelist without an EOS id never ends by itself
    assert any(len(set(r)) > 1 for r in said), said  # the penalty moves a row off its first token
    only = model.generate(**kw, allowed_token_ids=allowed)
    assert not torch.equal(only["sequences"], res["sequences"])  # (without the processors the rows differ: they did act)
    _replay(table, only, B)


def test_sampled_rows_stay_inside_the_automaton():
    dtype, B = torch.bfloat16, 2
    cfg, model, kw, free, low = _base(dtype, B)
    choices = _choices(low)
    A, Bt = C.TokenAutomaton.from_choices(choices[:2]), C.TokenAutomaton.from_choices(choices[2:])
    sk = dict({k: v for k, v in kw.items() if k != "output_logits"}, do_sample=True, temperature=2.0, max_new_tokens=T)
    for seed in (3, 4):
        res = model.generate(**sk, seed=seed, guided_choice=choices)
        again = model.generate(**sk, seed=seed, guided_choice=choices)
        assert model._mode.sampled and model._mode.constrained and torch.equal(res["sequences"], again["sequences"])
        for r in res["sequences"].tolist():
            assert EOS in r and r[: r.index(EOS)] in choices and set(r[r.index(EOS) + 1 :]) <= {PAD}, r
        assert res["constraint_complete"].tolist() == [True] * B
    # num_return_sequences = 3 with one automaton per prompt: rows b * 3 .. b * 3 + 2 share prompt b's start state
    res = model.generate(**sk, seed=5, num_return_sequences=3, constraint=[A, Bt])
    rows = res["sequences"].tolist()
    assert len(rows) == 6 and res["constraint_complete"].tolist() == [True] * 6
    for i, r in enumerate(rows):
        assert r[: r.index(EOS)] in (choices[:2] if i < 3 else choices[2:]), (i, r)


def test_per_row_automata_greedy():
    dtype, B = torch.float32, 4
    cfg, model, kw, free, low = _base(dtype, B)
    autos = [C.TokenAutomaton.from_choices([[low[b], low[b + 1]]]) for b in range(B)]
    autos[3] = autos[0]  # the same object twice: stored once
    res = model.generate(**kw, constraint=autos)
    want = [[low[0], low[1], EOS], [low[1], low[2], EOS], [low[2], low[3], EOS], [low[0], low[1], EOS]]
    assert res["sequences"].tolist() == want and res["constraint_complete"].tolist() == [True] * B
    _replay(C.compile(autos, (EOS,), B), res, B)
    with pytest.raises(ValueError, match="automata for"):
        model.generate(**kw, constraint=autos[:3])


def test_stop_sequences_and_logprobs():
    dtype, B = torch.bfloat16, 4
    cfg, model, kw, free, low = _base(dtype, B)
    c = low[:3]
    res = model.generate(**kw, guided_choice=[c], stop_sequences=[c[:2]])
    assert model._mode.stop and model._mode.constrained
    assert res["sequences"].tolist() == [c[:2]] * B and res["constraint_complete"].tolist() == [False] * B  # the stop sequence ends the rows inside the choice
    # log-probabilities stay those of the model's own distribution: step 0's equal, bit for bit, the negative of score()'s nll of the same token on the same prompt
    lk = {k: v for k, v in kw.items() if k != "output_logits"}
    res = model.generate(**lk, guided_choice=[c], output_logprobs=True, top_logprobs=2)
    assert res["sequences"].tolist() == [c + [EOS]] * B
    sc = model.score(kw["inputs"], torch.tensor([[c[0]]] * B), images=kw["images"])
    assert torch.equal(_bits(res["logprobs"][:, 0].cpu()), _bits(-sc["nll"][:, 0].cpu()))
    assert bool((res["logprobs"][:, 0] < -1.0).all())  # a low-ranked token: not the constrained distribution's (near 0)
    assert torch.equal(res["top_logprob_ids"][:, 0, 0].cpu(), free["logits"][0].float().argmax(dim=1))  # the alternatives are the unconstrained ones


def _spy(model, run):
    """run() with eager launches -> the C entries every _bookkeep call made (hip_ops' wrappers report their entry's name to ops._check)."""
    from dynamic_llava_amd import hip_ops as ops

    calls, sink, check, cls = [], [None], ops._check, type(model)

    def spy_check(rc, what):
        if sink[0] is not None:
            sink[0].append(what)
        return check(rc, what)

    def bookkeep(*a, **k):
        sink[0] = []
        try:
            return cls._bookkeep(model, *a, **k)
        finally:
            calls.append(tuple(sink[0]))
            sink[0] = None

    graph = model.use_hip_graph
    ops._check, model._bookkeep, model.use_hip_graph = spy_check, bookkeep, False
    try:
        out = run()
        torch.cuda.synchronize()
    finally:
        ops._check, model.use_hip_graph = check, graph
        del model._bookkeep
    return out, calls


def test_one_graph_per_shape_and_no_change_without_the_keywords():
    dtype, B = torch.bfloat16, 4
    cfg, model, kw, free, low = _base(dtype, B)
    pk = {k: v for k, v in kw.items() if k not in ("return_dict_in_generate", "output_logits")}
    choices = _choices(low)
    before_plain = model.generate(**pk).cpu()
    assert torch.equal(before_plain, free["sequences"][:, : before_plain.shape[1]])
    plain_mode = model._mode
    assert plain_mode == StepMode(eos=EOS, pad=PAD, min_new=0) and plain_mode.constrained is False
    first = None
    for _ in range(3):  # (a prompt shape's prefill is captured at its second sighting)
        got = model.generate(**pk, guided_choice=choices).cpu()
        assert first is None or torch.equal(got, first)
        first = got
    count = lambda: (len(model._dstate.graphs), sum(e["graph"] is not None for e in model._prefill_graphs.values()), len(model._prefill_graphs))
    before = count()
    other = [[low[4], low[3]], [low[5]]]
    got = model.generate(**pk, guided_choice=other).cpu()  # another automaton
    assert all(r[: r.index(EOS)] in other for r in got.tolist()) and not torch.equal(got, first)
    got = model.generate(**pk, allowed_token_ids=low[:2]).cpu()  # a whitelist: one accepting state, EOS among its edges
    assert set(got.reshape(-1).tolist()) <= set(low[:2]) | {EOS, PAD}
    got = model.generate(**pk, constraint=[C.TokenAutomaton.from_choices([[low[b]]]) for b in range(B)]).cpu()  # one automaton per row
    assert got.tolist() == [[low[b], EOS] for b in range(B)]
    assert count() == before, (count(), before)
    # an unconstrained request after constrained ones: the mode, the tokens and the logits of before
    assert torch.equal(model.generate(**pk).cpu(), before_plain) and model._mode == plain_mode
    for v in (None,):
        res = model.generate(**kw, constraint=v, guided_choice=v, allowed_token_ids=v, prefix_allowed_tokens_fn=v)
        assert model._mode == plain_mode and torch.equal(res["sequences"].cpu(), free["sequences"]) and _same_logits([z.cpu() for z in res["logits"]], free["logits"])
        assert "constraint_complete" not in res
    # the launches that close a step: without the keywords dl_logits_constrain is absent, with them it sits behind dl_logits_process and in front of the step-closing kernel
    _, calls = _spy(model, lambda: model.generate(**pk))
    assert calls and all(c == ("dl_decode_advance",) for c in calls), calls
    _, calls = _spy(model, lambda: model.generate(**pk, guided_choice=choices))
    assert calls and all(c == ("dl_logits_constrain", "dl_decode_advance") for c in calls), calls
    _, calls = _spy(model, lambda: model.generate(**pk, guided_choice=choices, repetition_penalty=1.2, do_sample=True, seed=1, output_logprobs=True, return_dict_in_generate=True))
    assert calls and all(c == ("dl_logits_process", "dl_logits_constrain", "dl_decode_sample", "dl_decode_logprobs") for c in calls), calls


def test_score_refuses_a_constraint_before_any_launch():
    dtype, B = torch.bfloat16, 1
    cfg, model, kw, free, low = _base(dtype, B)
    with pytest.raises(ValueError, match="constraint"):
        model.score(kw["inputs"], torch.tensor([[low[0]]]), images=kw["images"], guided_choice=[[low[0]]])
    with pytest.raises(ValueError, match="at most one"):
        model.generate(**kw, guided_choice=[[low[0]]], allowed_token_ids=low)
    with pytest.raises(ValueError, match="min_new_tokens"):
        model.generate(**kw, guided_choice=[[low[0]]], min_new_tokens=2)
