"""GPU: generate(repetition_penalty= / no_repeat_ngram_size= / bad_words_ids=) on the tiny config of oracle/fixtures.py -- every step replayed from the
record (`scores` are what dl_logits_process left, `logits` the raw step logits, `sequences` the history), on every route, schedule and graph state.

The comparisons are bit for bit: the rule (logits_rules.py) edits an entry with one fp32 operation on the raw logit, which the record holds exactly
(the step buffer's model-dtype values, copied to fp32)."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import logits_rules as lr  # noqa: E402
from dynamic_llava_amd import sampling as sp  # noqa: E402

NEG = float("-inf")
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
_MODELS = {}


@pytest.fixture(autouse=True, scope="module")
def _release_models():
    """The models this module shares live exactly as long as the module's tests; a model that served requests is an object cycle (a prefill entry's closure holds
    it), so it is collected here, between tests, and not whenever the collector next runs inside somebody's stream capture."""
    yield
    _MODELS.clear()
    gc.collect()
    torch.cuda.synchronize()


def _model(dtype, kv=None, fresh=False):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from oracle import fixtures as fx
    from oracle.make_golden import SD_SEED

    if fresh or (dtype, kv) not in _MODELS:
        cfg = fx.tiny_config()  # text predictor on: rows evict
        sd = fx.make_state_dict(cfg, seed=SD_SEED, predictor_gain=50.0)
        clip = fx.build_clip(cfg, seed=1, dtype=dtype)
        model = build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg), sd, clip.state_dict(), dtype=dtype, device="cuda")
        if kv is not None:
            model.set_kv_cache_format(kv)
        if fresh:  # (a test that counts captured graphs wants a model nobody has used)
            return cfg, model
        _MODELS[(dtype, kv)] = (cfg, model)
    return _MODELS[(dtype, kv)]


def _inputs(cfg, B, dtype):
    from oracle import fixtures as fx

    if B == 1:
        return dict(inputs=fx.make_prompt(cfg, 5, 9, seed=2)[None].cuda(), images=fx.make_images(cfg, 1, seed=3).to(dtype).cuda())
    prompts = [fx.make_prompt(cfg, 5, 7, seed=0), fx.make_prompt(cfg, 2, 15, seed=1)]  # ragged
    n = max(p.shape[0] for p in prompts)
    ids, am = torch.zeros(B, n, dtype=torch.long), torch.zeros(B, n, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]] = p
        am[b, : p.shape[0]] = 1
    return dict(inputs=ids.cuda(), attention_mask=am.cuda(), images=fx.make_images(cfg, B, seed=3).to(dtype).cuda())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lowest_argmax(z):
    return torch.tensor([int((z[b] == z[b].max()).nonzero()[0]) for b in range(z.shape[0])])


def _bad_words(base):
    """From an unprocessed run [B, T]: every row's first token as a one-token word, its tokens 2..3 as a two-token word."""
    base = base.cpu().tolist()
    return [[r[0]] for r in base] + [[r[1], r[2]] for r in base]


def _replay(res, rules, B, sampled=None):
    """Every step of a recorded request against the rule; -> the sequences (CPU)."""
    seq = res["sequences"].cpu()
    assert len(res["scores"]) == len(res["logits"]) == seq.shape[1]
    for j in range(seq.shape[1]):
        raw = res["logits"][j].cpu()
        want = rules.apply(raw, seq[:, :j])
        if sampled is None:
            assert torch.equal(_bits(res["scores"][j].cpu()), _bits(want)), f"step {j}: scores are the processed logits"
            assert torch.equal(seq[:, j], _lowest_argmax(want)), f"step {j}: the token is their argmax"
        else:
            T, k, p, seed = sampled
            for b in range(B):
                tok, kept, _ = sp.reference_step(want[b], T, k, p, (), seed, b, j)
                assert int(seq[b, j]) == tok, (j, b)
                assert torch.equal(res["scores"][j][b].cpu() > NEG, kept), "sampled scores: -inf exactly outside the kept set of the processed row"
    return seq


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_replay_from_the_record(dtype, B):
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=12, eos_token_id=None)
    base = model.generate(**kw)
    words = _bad_words(base)
    res = model.generate(**kw, **PROC, bad_words_ids=words, return_dict_in_generate=True, output_scores=True, output_logits=True)
    rules = lr.normalize(dict(PROC, bad_words_ids=words), cfg.vocab_size)
    seq = _replay(res, rules, B)
    assert seq.shape == (B, 12)
    assert bool((seq[:, 0] != base[:, 0].cpu()).all()), "the unprocessed first token is a bad word"
    assert not torch.equal(_bits(res["scores"][0].cpu()), _bits(res["logits"][0].cpu())), "scores are not the raw logits"
    for b in range(B):  # no 2-gram occurs twice
        grams = [tuple(seq[b, i : i + 2].tolist()) for i in range(11)]
        assert len(set(grams)) == len(grams)
    # the same request without the step-by-step outputs emits the same tokens
    assert torch.equal(model.generate(**kw, **PROC, bad_words_ids=words).cpu(), seq)


@pytest.mark.parametrize("B", [1, 2])
def test_no_repeat_ngram_size_1_gives_pairwise_distinct_tokens(B):
    cfg, model = _model(torch.bfloat16)
    out = model.generate(**_inputs(cfg, B, torch.bfloat16), max_new_tokens=24, eos_token_id=None, no_repeat_ngram_size=1).cpu()
    for b in range(B):
        assert len(set(out[b].tolist())) == 24


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_device_sampling_on_the_processed_rows(dtype, B):
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=12, eos_token_id=None)
    words = _bad_words(model.generate(**kw))
    T, k, p, seed = 0.8, 20, 0.9, 7
    res = model.generate(**kw, **PROC, bad_words_ids=words, do_sample=True, seed=seed, temperature=T, top_k=k, top_p=p,
                         return_dict_in_generate=True, output_scores=True, output_logits=True)
    rules = lr.normalize(dict(PROC, bad_words_ids=words), cfg.vocab_size)
    seq = _replay(res, rules, B, sampled=(T, k, p, seed))
    banned_first = {w[0] for w in words if len(w) == 1}
    assert not set(seq[:, 0].tolist()) & banned_first


@pytest.mark.parametrize("B", [1, 2])
def test_schedule_independence(B):
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=24, eos_token_id=None)
    words = _bad_words(model.generate(**kw))
    pk = dict(PROC, bad_words_ids=words)
    base = model.generate(**kw, **pk)
    for se in (1, 3, 64):
        assert torch.equal(model.generate(**kw, **pk, sync_every=se), base), se
    model.use_hip_graph = False
    try:
        assert torch.equal(model.generate(**kw, **pk), base)
    finally:
        model.use_hip_graph = True
    assert torch.equal(model.generate(**kw, **pk), base)


@pytest.mark.parametrize("B", [1, 2])
def test_host_routes_agree_with_the_device_route(B):
    dtype = torch.float32
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=10)
    words = _bad_words(model.generate(**kw, eos_token_id=None))
    pk = dict(repetition_penalty=1.3, bad_words_ids=words)
    dev = model.generate(**kw, eos_token_id=None, **pk, no_repeat_ngram_size=2)
    # four EOS ids, which never occur, force the plain loop over forward(): _generate_sample(greedy=True) applies the same rule
    seen = set(dev.cpu().flatten().tolist()) | {t for w in words for t in w}  # (a one-token word equal to an EOS id would be dropped)
    four = [t for t in range(cfg.vocab_size - 1, 0, -1) if t not in seen][:4]
    host4 = model.generate(**kw, eos_token_id=four, **pk, no_repeat_ngram_size=2)
    assert torch.equal(host4, dev)
    assert not torch.equal(dev, model.generate(**kw, eos_token_id=None)), "the settings change the tokens"
    # an n-gram size over the device cap forces the same loop; at 10 tokens n = 17 bans nothing, so the tokens are those of penalty + words alone
    over = model.generate(**kw, eos_token_id=None, **pk, no_repeat_ngram_size=lr.MAX_NGRAM + 1)
    assert torch.equal(over, model.generate(**kw, eos_token_id=None, **pk))
    assert not torch.equal(over, model.generate(**kw, eos_token_id=None)), "the host loop does not drop the keywords"
    over_s = model.generate(**kw, eos_token_id=None, **pk, no_repeat_ngram_size=lr.MAX_NGRAM + 1, return_dict_in_generate=True, output_scores=True)
    rules = lr.normalize(dict(pk, no_repeat_ngram_size=lr.MAX_NGRAM + 1), cfg.vocab_size)
    seq = over_s["sequences"].cpu()
    assert torch.equal(seq, over.cpu())
    for j in range(seq.shape[1]):
        assert bool((over_s["scores"][j].cpu()[:, [w[0] for w in words if len(w) == 1]] == NEG).all())


def test_a_continued_dialogue_never_emits_a_bad_word():
    dtype = torch.float32
    cfg, model = _model(dtype)
    inp = _inputs(cfg, 1, dtype)
    turn2 = torch.randint(3, cfg.vocab_size, (1, 7), generator=torch.Generator().manual_seed(12)).cuda()
    r0 = model.generate(**inp, max_new_tokens=4, eos_token_id=None, return_dict_in_generate=True)
    free = model.generate(turn2, past_key_values=r0["past_key_values"], max_new_tokens=8, eos_token_id=None).cpu()
    r1 = model.generate(**inp, max_new_tokens=4, eos_token_id=None, return_dict_in_generate=True)  # (the first turn again: a continuation advances the cache it is given)
    bad = sorted(set(free[0].tolist()))[:2]
    out = model.generate(turn2, past_key_values=r1["past_key_values"], max_new_tokens=8, eos_token_id=None, bad_words_ids=[[t] for t in bad], no_repeat_ngram_size=1).cpu()
    assert not set(out[0].tolist()) & set(bad) and len(set(out[0].tolist())) == 8


def test_one_graph_serves_every_setting_and_off_stays_off():
    dtype = torch.bfloat16
    cfg, model = _model(dtype, fresh=True)
    kw = dict(_inputs(cfg, 1, dtype), max_new_tokens=12, eos_token_id=None)
    for _ in range(3):  # first sighting runs eagerly, the second captures, the third replays
        plain = model.generate(**kw)
    st = model._dstate
    n_dec, n_pre = len(st.graphs), len(model._prefill_graphs)
    assert n_dec >= 1 and n_pre >= 1
    # an all-neutral request is the request without the keywords: same graphs, same tokens
    assert torch.equal(model.generate(**kw, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=[]), plain)
    assert torch.equal(model.generate(**kw, repetition_penalty=None, no_repeat_ngram_size=None, bad_words_ids=None), plain)
    assert len(st.graphs) == n_dec and len(model._prefill_graphs) == n_pre and model._dstate is st and model._mode.processed is False
    words = _bad_words(plain)
    for _ in range(3):
        first = model.generate(**kw, **PROC, bad_words_ids=words)
    n_dec2, n_pre2 = len(st.graphs), len(model._prefill_graphs)
    assert n_dec2 > n_dec and n_pre2 == n_pre + 1 and model._mode.processed is True
    outs = [first]
    for pk in (dict(repetition_penalty=0.7), dict(no_repeat_ngram_size=1), dict(repetition_penalty=2.0, no_repeat_ngram_size=3, bad_words_ids=[[5], [6, 7, 8]]),
               dict(bad_words_ids=[[int(plain[0, 0])]])):
        outs.append(model.generate(**kw, **pk))
        assert len(st.graphs) == n_dec2 and len(model._prefill_graphs) == n_pre2 and model._dstate is st, pk
    assert len({tuple(o.cpu().tolist()[0]) for o in outs}) > 1
    assert torch.equal(model.generate(**kw), plain), "a plain call after processed ones is what it was before them"
    assert len(st.graphs) == n_dec2 and len(model._prefill_graphs) == n_pre2
    del model, st  # (this test's own model: collected now, see _release_models)
    gc.collect()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_min_new_tokens_and_the_eos_word(dtype):
    cfg, model = _model(dtype)
    inp = _inputs(cfg, 2, dtype)
    kw = dict(inp, max_new_tokens=12)
    # the EOS id: the token the processed run would emit first in row 0
    words0 = _bad_words(model.generate(**kw, eos_token_id=None))
    first = model.generate(**kw, eos_token_id=None, **PROC, bad_words_ids=words0).cpu()
    eos = int(first[0, 0])
    res = model.generate(**kw, eos_token_id=eos, pad_token_id=1, min_new_tokens=4, **PROC, bad_words_ids=words0, return_dict_in_generate=True, output_scores=True, output_logits=True)
    seq = res["sequences"].cpu()
    assert eos not in seq[:, :4].flatten().tolist(), "the EOS ban of min_new_tokens holds under processing"
    rules = lr.normalize(dict(PROC, bad_words_ids=words0), cfg.vocab_size, [eos])
    for j in range(min(4, seq.shape[1])):
        want = rules.apply(res["logits"][j].cpu(), seq[:, :j])
        want[:, eos] = NEG
        assert torch.equal(_bits(res["scores"][j].cpu()), _bits(want)), j
    # a bad word equal to [eos] is dropped: the row still ends with it
    out = model.generate(**kw, eos_token_id=eos, pad_token_id=1, **PROC, bad_words_ids=words0 + [[eos]]).cpu()
    assert int(out[0, 0]) == eos and (out.shape[1] == 1 or out[0, 1:].tolist() == [1] * (out.shape[1] - 1))
    assert lr.normalize(dict(bad_words_ids=[[eos]]), cfg.vocab_size, [eos]).bad_words == ()


@pytest.mark.parametrize("B", [1, 2])
def test_mxfp8_kv_cache_with_processors(B):
    dtype = torch.bfloat16
    cfg, model = _model(dtype, kv="mxfp8")
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=12, eos_token_id=None)
    base = model.generate(**kw)
    words = _bad_words(base)
    res = model.generate(**kw, **PROC, bad_words_ids=words, return_dict_in_generate=True, output_scores=True, output_logits=True)
    seq = _replay(res, lr.normalize(dict(PROC, bad_words_ids=words), cfg.vocab_size), B)
    assert bool((seq[:, 0] != base[:, 0].cpu()).all())
    assert torch.equal(model.generate(**kw, **PROC, bad_words_ids=words).cpu(), seq)


def test_score_is_unaffected_and_takes_no_processors():
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    inp = _inputs(cfg, 2, dtype)
    labels = torch.randint(3, cfg.vocab_size, (2, 6), generator=torch.Generator().manual_seed(5))
    skw = dict(images=inp["images"], attention_mask=inp["attention_mask"])
    before = model.score(inp["inputs"], labels, **skw)
    model.generate(**inp, max_new_tokens=6, eos_token_id=None, **PROC, bad_words_ids=[[int(labels[0, 0])]])
    after = model.score(inp["inputs"], labels, **skw)
    assert torch.equal(_bits(before["nll"]), _bits(after["nll"])) and torch.equal(before["top1"], after["top1"])
    with pytest.raises(ValueError):
        model.generate(**inp, max_new_tokens=6, eos_token_id=None, repetition_penalty=1.3, _score_labels=labels)
    with pytest.raises(TypeError):
        model.score(inp["inputs"], labels, repetition_penalty=1.3, **skw)
