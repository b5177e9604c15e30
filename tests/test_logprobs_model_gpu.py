"""GPU, model level: generate(output_logprobs=True, top_logprobs=n) on the tiny config of oracle/fixtures.py -- the log-probabilities dl_decode_logprobs reads off
inside the decode graphs against the rule (dynamic_llava_amd/logprobs.py) on the step logits the model itself reports, against score() on the same tokens, over
graph states and schedules, early EOS, sampled and processed requests, every host route; the launch sequence and the decode loop's chunks.

Tolerance.  Where the kernel is compared with the host rule on the same logits the bound is score_cases.device_tol (derived there):
    tol = (2 * 2^-23 + V * 2^-40 + 2^-23) + 2 * ulp32(lse_ref) + ulp32(logprob_ref);
ids, tokens, and every comparison between two runs of the device route, with score(), and of a host route with the host rule are exact."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

import score_cases as cs  # noqa: E402
from dynamic_llava_amd import hip_ops as ops  # noqa: E402
from dynamic_llava_amd import logits_rules as lr  # noqa: E402
from dynamic_llava_amd import logprobs as lpr  # noqa: E402

LP = dict(return_dict_in_generate=True, output_logprobs=True)
KEYS = ("logprobs", "top_logprobs", "top_logprob_ids")
_MODELS = {}


@pytest.fixture(autouse=True, scope="module")
def _release_models():
    """The models this module shares live exactly as long as the module's tests (a model that served requests is an object cycle: collected here, between tests,
    and not whenever the collector next runs inside somebody's stream capture)."""
    yield
    _MODELS.clear()
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


def _same(a, b, keys=KEYS + ("sequences",)):
    return all((k in a) == (k in b) and (k not in a or (a[k].shape == b[k].shape and torch.equal(_bits(a[k]) if a[k].dtype == torch.float32 else a[k], _bits(b[k]) if b[k].dtype == torch.float32 else b[k])))
               for k in keys)


def _check_shapes(res, n):
    B, T = res["sequences"].shape
    assert res["logprobs"].shape == (B, T) and res["logprobs"].dtype == torch.float32
    if n == 0:
        assert "top_logprobs" not in res and "top_logprob_ids" not in res
    else:
        assert res["top_logprobs"].shape == (B, T, n) and res["top_logprobs"].dtype == torch.float32
        assert res["top_logprob_ids"].shape == (B, T, n) and res["top_logprob_ids"].dtype == torch.int64


def _check_against_rule(res, step_logits, n, what, live=None):
    """The result keys against the rule on step_logits (one fp32 [B, V] per column of `sequences`): ids exact, values within tol.  live [B, T] bool: the columns
    that are not behind a row's first EOS (default: all)."""
    _check_shapes(res, n)
    seq = res["sequences"].cpu()
    B, T = seq.shape
    V = step_logits[0].shape[-1]
    assert len(step_logits) == T
    lp, top_lp, top_ids = res["logprobs"].cpu(), (res["top_logprobs"].cpu() if n else None), (res["top_logprob_ids"].cpu() if n else None)
    worst = 0.0
    for t in range(T):
        for b in range(B):
            if live is not None and not bool(live[b, t]):
                continue
            r_lp, r_top, r_ids = lpr.reference_row(step_logits[t][b].cpu(), int(seq[b, t]), max(n, 1))
            lse = -float(r_top[0])
            assert n == 0 or top_ids[b, t].tolist() == r_ids[:n].tolist(), (what, b, t)
            for k, (got, ref) in enumerate([(lp[b, t], r_lp)] + [(top_lp[b, t, k], r_top[k]) for k in range(n)]):
                if torch.isinf(ref):
                    assert float(got) == float(ref), (what, b, t, k)
                    continue
                tol = cs.device_tol(V, lse, float(ref))
                err = abs(float(got) - float(ref))
                worst = max(worst, err / tol)
                assert err <= tol, (what, b, t, k, float(got), float(ref), tol)
    print(f"{what}: worst |value - rule| / tol = {worst:.3f}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_greedy(dtype, B):
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=7, eos_token_id=None)
    plain = model.generate(**kw)
    rec = model.generate(**kw, return_dict_in_generate=True, output_logits=True)
    res = model.generate(**kw, **LP, top_logprobs=5)
    none = model.generate(**kw, **LP)
    torch.cuda.synchronize()
    model.check_device_errors()
    assert torch.equal(res["sequences"], plain) and torch.equal(rec["sequences"], plain) and torch.equal(none["sequences"], plain)
    assert "logprobs" not in rec and "scores" not in res and "logits" not in res
    _check_against_rule(res, rec["logits"], 5, f"greedy {dtype} B={B}")
    _check_shapes(none, 0)
    assert torch.equal(_bits(none["logprobs"]), _bits(res["logprobs"]))
    assert torch.equal(res["top_logprob_ids"][:, :, 0], plain)  # greedy: the token is entry 0 of its step's list ...
    assert torch.equal(_bits(res["top_logprobs"][:, :, 0]), _bits(res["logprobs"]))  # ... and reports the same bits there
    eight = model.generate(**kw, **LP, top_logprobs=8)
    assert torch.equal(eight["top_logprob_ids"][:, :, :5], res["top_logprob_ids"]) and torch.equal(_bits(eight["top_logprobs"][:, :, :5]), _bits(res["top_logprobs"]))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_generate_then_score_the_same_tokens(dtype, B):
    """The scorer's nll of the tokens generate() picked, on bit-equal logits: the same bits, negated."""
    cfg, model = _model(dtype)
    inp = _inputs(cfg, B, dtype)
    gen = model.generate(**inp, max_new_tokens=8, eos_token_id=None, **LP, top_logprobs=2, output_logits=True)
    sc = model.score(inp["inputs"], gen["sequences"].clone(), images=inp["images"], output_logits=True)
    torch.cuda.synchronize()
    model.check_device_errors()
    assert torch.equal(_bits(torch.stack(gen["logits"])), _bits(torch.stack(sc["logits"])))
    assert torch.equal(_bits(gen["logprobs"]), _bits(-sc["nll"])), (gen["logprobs"], sc["nll"])
    assert torch.equal(sc["top1"], gen["top_logprob_ids"][:, :, 0])


@pytest.mark.parametrize("B", [1, 3])
def test_graph_against_eager_and_across_schedules(B):
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=8, eos_token_id=None, **LP, top_logprobs=8)
    runs = [model.generate(**kw) for _ in range(3)]  # the decode steps are captured and replayed inside every call; the third call has seen the shape twice
    runs += [model.generate(**kw, sync_every=se) for se in (1, 3)]
    runs.append(model.generate(**kw, output_logits=True))  # the step-by-step route
    model.use_hip_graph = False
    try:
        runs.append(model.generate(**kw))
    finally:
        model.use_hip_graph = True
    runs.append(model.generate(**kw))
    torch.cuda.synchronize()
    model.check_device_errors()
    for i, r in enumerate(runs[1:]):
        assert _same(r, runs[0]), i + 1
    _check_shapes(runs[0], 8)


def _early_eos_id(seq):
    """From a greedy run [3, T] without EOS: (row, column, token) with 1 <= column <= T - 3 whose token occurs nowhere else before that column in its own row and
    nowhere at all in the other rows."""
    rows = seq.cpu().tolist()
    for r, row in enumerate(rows):
        for c in range(1, len(row) - 2):
            others = {t for q, other in enumerate(rows) if q != r for t in other}
            if row[c] not in others and row[c] not in row[:c]:
                return r, c, row[c]
    raise AssertionError(f"no token ends exactly one row early in {rows}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_early_eos(dtype):
    cfg, model = _model(dtype)
    PAD, n = 1, 3
    kw = dict(_inputs(cfg, 3, dtype), max_new_tokens=8, pad_token_id=PAD, **LP, top_logprobs=n)
    base = model.generate(**kw, eos_token_id=None)
    r, c, eos = _early_eos_id(base["sequences"])
    res = model.generate(**kw, eos_token_id=eos)
    rec = model.generate(**{k: v for k, v in kw.items() if k not in ("output_logprobs", "top_logprobs")}, eos_token_id=eos, output_logits=True)
    torch.cuda.synchronize()
    model.check_device_errors()
    seq = res["sequences"].cpu()
    assert seq.shape == (3, 8) and torch.equal(seq, rec["sequences"].cpu())  # one row of three ends: nothing is trimmed
    assert int(seq[r, c]) == eos and seq[r, c + 1 :].tolist() == [PAD] * (7 - c)
    live = torch.ones((3, 8), dtype=torch.bool)
    live[r, c + 1 :] = False
    assert torch.equal(torch.where(live, seq, torch.full_like(seq, PAD)), torch.where(live, base["sequences"].cpu(), torch.full_like(seq, PAD)))
    dead = ~live
    assert bool((res["logprobs"].cpu()[dead] == 0.0).all()) and bool((res["top_logprobs"].cpu()[dead] == 0.0).all()) and bool((res["top_logprob_ids"].cpu()[dead] == -1).all())
    _check_against_rule(res, rec["logits"], n, f"early EOS {dtype}", live=live)
    assert float(res["logprobs"][r, c]) < 0.0 and int(res["top_logprob_ids"][r, c, 0]) == eos  # the EOS token's own entry is real
    assert bool((res["top_logprob_ids"].cpu()[live] >= 0).all())
    # every row ends: the columns after the last EOS are trimmed from all keys
    one = dict(_inputs(cfg, 1, dtype), max_new_tokens=8, pad_token_id=PAD, **LP, top_logprobs=n)
    b1 = model.generate(**one, eos_token_id=None)
    row = b1["sequences"][0].cpu().tolist()
    c1 = next(i for i in range(1, 8) if row[i] not in row[:i])
    cut = model.generate(**one, eos_token_id=row[c1])
    assert cut["sequences"].shape == (1, c1 + 1) and c1 + 1 < 8
    _check_shapes(cut, n)
    assert _same(cut, {k: b1[k][:, : c1 + 1] for k in KEYS + ("sequences",)})


def test_sampled_with_processors_reports_the_raw_distribution():
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    inp = _inputs(cfg, 3, dtype)
    first = model.generate(**inp, max_new_tokens=7, eos_token_id=None)
    kw = dict(inp, max_new_tokens=7, eos_token_id=None, do_sample=True, seed=5, temperature=0.8, top_k=20, repetition_penalty=1.3, bad_words_ids=[[int(t)] for t in first[:, 0]])
    toks = model.generate(**kw)
    res = model.generate(**kw, **LP, top_logprobs=4)
    rec = model.generate(**kw, **LP, top_logprobs=4, output_logits=True, output_scores=True)
    torch.cuda.synchronize()
    model.check_device_errors()
    assert torch.equal(res["sequences"], toks) and torch.equal(rec["sequences"], toks)  # the keywords change no token
    assert _same(res, rec)
    _check_against_rule(res, rec["logits"], 4, "sampled + processors")
    raw0, proc0 = rec["logits"][0].cpu(), rec["scores"][0].cpu()
    assert not torch.equal(raw0.argmax(dim=-1), proc0.argmax(dim=-1)), "the greedy token of step 0 is a bad word: the processed maximum is another token"
    assert torch.equal(res["top_logprob_ids"][:, 0, 0].cpu(), raw0.argmax(dim=-1))  # the list is the raw row's, bad word included
    on_processed = torch.log_softmax(proc0.double(), dim=-1)[torch.arange(3), toks[:, 0].cpu()]
    assert bool(((res["logprobs"][:, 0].cpu().double() - on_processed).abs() > 1e-3).any()), "values refer to the raw logits, not to the processed ones"


def _forward_loop(model, seq, first_logits, cache):
    """What every host route does: take the logits, feed the token, one forward() per step -> fp32 [B, V] per column of seq."""
    logits = [first_logits.float().clone()]
    for j in range(seq.shape[1] - 1):
        out = model(seq[:, j : j + 1], past_key_values=cache)
        cache = out.past_key_values
        logits.append(out.logits[:, -1].float().clone())
    torch.cuda.synchronize()
    model.check_device_errors()
    return logits


def _prompt_logits(model, inp):
    out = model(inp["inputs"], images=inp["images"])
    cache = out.past_key_values
    last = cache[1][-1].to(out.logits.device).long() - 1
    return out.logits[torch.arange(out.logits.shape[0], device=out.logits.device), last], cache


def _check_host_route(model, res, logits, eos_ids, n, what):
    want = lpr.host_result(logits, res["sequences"], eos_ids, n)
    _check_shapes(res, n)
    assert _same(res, dict(want, sequences=res["sequences"])), what
    assert res["logprobs"].device == res["sequences"].device


def test_every_host_route():
    dtype = torch.float32
    cfg, model = _model(dtype)
    inp = _inputs(cfg, 3, dtype)
    kw = dict(inp, max_new_tokens=6, **LP, top_logprobs=3)
    base = model.generate(**inp, max_new_tokens=6, eos_token_id=None).cpu()
    unseen = [t for t in range(cfg.vocab_size - 1, 0, -1) if t not in set(base.flatten().tolist())]
    r, c, eos = _early_eos_id(torch.cat([base, base[:, -1:]], dim=1))  # (a column in 1 .. 4 of the six)

    def run(what, eos_ids, **route):
        res = model.generate(**kw, **route)
        logits = _forward_loop(model, res["sequences"], *_prompt_logits(model, inp))
        _check_host_route(model, res, logits, eos_ids, 3, what)
        return res

    torch.manual_seed(3)
    run("torch RNG", [], do_sample=True, temperature=0.9, top_k=30, eos_token_id=None)
    run("generator=", [], do_sample=True, seed=4, generator=torch.Generator(device="cuda").manual_seed(8), eos_token_id=None)
    four = run("four EOS ids", unseen[:3] + [eos], eos_token_id=unseen[:3] + [eos], pad_token_id=1)
    assert torch.equal(four["sequences"][:, : c + 1].cpu(), base[:, : c + 1]) and four["sequences"][r, c + 1 :].tolist() == [1] * (5 - c)
    assert bool((four["logprobs"][r, c + 1 :] == 0.0).all()) and bool((four["top_logprob_ids"][r, c + 1 :] == -1).all()) and float(four["logprobs"][r, c]) < 0.0
    over = run("processors past the device caps", [], eos_token_id=None, no_repeat_ngram_size=lr.MAX_NGRAM + 1, repetition_penalty=1.3)
    assert torch.equal(over["top_logprob_ids"][:, 0, 0].cpu(), base[:, 0])  # the raw row's list
    # the continuation of a dialogue: the same first turn twice, one cache for the route and one for the loop
    one = _inputs(cfg, 1, dtype)
    turn2 = torch.randint(3, cfg.vocab_size, (1, 7), generator=torch.Generator().manual_seed(12)).cuda()
    c_route = model.generate(**one, max_new_tokens=4, eos_token_id=None, return_dict_in_generate=True)["past_key_values"]
    c_loop = model.generate(**one, max_new_tokens=4, eos_token_id=None, return_dict_in_generate=True)["past_key_values"]
    res = model.generate(turn2, past_key_values=c_route, max_new_tokens=6, eos_token_id=None, **LP, top_logprobs=3)
    out = model(turn2, past_key_values=c_loop)
    _check_host_route(model, res, _forward_loop(model, res["sequences"], out.logits[:, -1], out.past_key_values), [], 3, "continued dialogue")
    assert "logprobs" not in model.generate(turn2, past_key_values=res["past_key_values"], max_new_tokens=2, eos_token_id=None, return_dict_in_generate=True)


def _record(model, run):
    """run() with eager launches -> (the C entries _first_token called, the C entries the SECOND _decode_step_kernels call made): every wrapper of hip_ops
    reports its entry's name to ops._check."""
    first, step, sink, n_steps = [], [], [None], [0]
    check, cls = ops._check, type(model)

    def spy_check(rc, what):
        if sink[0] is not None:
            sink[0].append(what)
        return check(rc, what)

    def first_token(*a, **k):
        sink[0] = first
        try:
            return cls._first_token(model, *a, **k)
        finally:
            sink[0] = None

    def step_kernels(*a, **k):
        n_steps[0] += 1
        sink[0] = step if n_steps[0] == 2 else None
        try:
            return cls._decode_step_kernels(model, *a, **k)
        finally:
            sink[0] = None

    graph = model.use_hip_graph
    ops._check, model._first_token, model._decode_step_kernels, model.use_hip_graph = spy_check, first_token, step_kernels, False
    try:
        run()
        torch.cuda.synchronize()
        model.check_device_errors()
    finally:
        ops._check, model.use_hip_graph = check, graph
        del model._first_token, model._decode_step_kernels
    assert n_steps[0] >= 2
    return first, step


@pytest.mark.parametrize("B", [1, 3])
def test_launch_sequence_gains_one_trailing_launch(B):
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=4, eos_token_id=None, return_dict_in_generate=True)
    for route in (dict(), dict(do_sample=True, seed=3, temperature=0.8), dict(repetition_penalty=1.2, no_repeat_ngram_size=2)):
        first0, step0 = _record(model, lambda: model.generate(**kw, **route))
        assert "dl_decode_logprobs" not in first0 + step0 and len(step0) > 3
        for n in (0, 8):
            first, step = _record(model, lambda: model.generate(**kw, **route, output_logprobs=True, top_logprobs=n))
            assert first == first0 + ["dl_decode_logprobs"], (route, n, first)
            assert step == step0 + ["dl_decode_logprobs"], (route, n, step)


def test_the_decode_loop_keeps_its_chunks():
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, 1, dtype), max_new_tokens=14, eos_token_id=None, return_dict_in_generate=True)

    def chunks(**more):
        seen, cls = [], type(model)
        model._run_decode_steps = lambda st, cache, n_steps: (seen.append(n_steps), cls._run_decode_steps(model, st, cache, n_steps))[1]
        try:
            model.generate(**kw, **more)
        finally:
            del model._run_decode_steps
        return seen

    plain = chunks()
    assert sum(plain) == 13 and max(plain) > 1
    assert chunks(output_logprobs=True) == plain and chunks(output_logprobs=True, top_logprobs=8) == plain
    assert chunks(output_scores=True) == [1] * 13  # (the route the keyword replaces steps one graph at a time)
