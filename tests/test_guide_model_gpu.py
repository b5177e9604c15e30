"""GPU, model level: generate(guidance_scale=, negative_prompt_ids= / negative_images=, guidance_cutoff=) on the tiny config of oracle/fixtures.py, at B = 1 (device
prompt layout, captured prefills) and at a ragged B = 2 (attention mask, host layout).

The replay tests are exact and compare no routes: every step's `scores` must be the rule of guidance.py on the step's raw `logits` / `negative_logits`, then the
processors, then the EOS ban, bit for bit, and every token its lowest-index argmax.  As in tests/test_guide_gpu.py the rule takes the two lse values from
dl_decode_logprobs on the same rows (the device's expf / logf cannot be reproduced on the CPU); everything else is the CPU rule."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_sampling_gpu as tsg  # noqa: E402  (the model builder and the B = 1 / ragged B = 2 inputs of the sampler's own tests)
from dynamic_llava_amd import constraints as C  # noqa: E402
from dynamic_llava_amd import guidance as G  # noqa: E402
from dynamic_llava_amd import request  # noqa: E402
from test_guide_gpu import _device_lse  # noqa: E402

T, PAD, EOS = 8, 1, 2
DT = torch.bfloat16
NEG_TEXT = torch.tensor([[1, 17, 45, 99, 120, 7]])  # a text-only negative prompt (no placeholder): the "language prior" contrast, broadcast over the prompts
_M = {}


@pytest.fixture(autouse=True, scope="module")
def _release():
    yield
    _M.clear()
    gc.collect()
    torch.cuda.synchronize()


def _model():
    if "m" not in _M:
        _M["m"] = tsg._model(DT)
    return _M["m"]


def _kw(B, **more):
    cfg, model = _model()
    return cfg, model, dict(tsg._inputs(cfg, B, DT), max_new_tokens=T, eos_token_id=EOS, pad_token_id=PAD, **more)


def _plain(B):
    """The request without the keywords, once per batch: its tokens (left unchanged)."""
    if ("plain", B) not in _M:
        cfg, model, kw = _kw(B)
        _M[("plain", B)] = model.generate(**kw).cpu()
    return _M[("plain", B)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _rule(c, u, scale, cutoff=None):
    """guidance.py on the reported raw logits [B, V] (fp32 images of model-dtype values), with the device's lse of either row."""
    lse_c, lse_u = _device_lse(c.to(DT).cuda()), _device_lse(u.to(DT).cuda())
    return torch.stack([G.guide_row(c[b].cpu(), u[b].cpu(), scale, cutoff, lse=(lse_c[b], lse_u[b])) for b in range(c.shape[0])])


def _argmax(z):
    return int((z == z.max()).nonzero()[0])


def _replay(res, B, scale, cutoff=None, rules=None, table=None):
    seq = res["sequences"].cpu()
    assert seq.shape[0] == B and len(res["logits"]) == len(res["negative_logits"]) == len(res["scores"]) == seq.shape[1]
    states = None if table is None else table.starts(B)
    done, cpu_diff = [False] * B, 0
    for t in range(seq.shape[1]):
        c, u = res["logits"][t].cpu(), res["negative_logits"][t].cpu()
        assert c.shape == u.shape == (B, 320) and c.dtype == torch.float32
        z = _rule(c, u, scale, cutoff)
        cpu_diff += int((_bits(z) != _bits(G.apply(c, u, scale, cutoff))).sum())
        if rules is not None:
            z = rules.apply(z, seq[:, :t] if t else [[]] * B)
        if states is not None:
            z = C.apply_rows(table, z, states)
        assert torch.equal(_bits(res["scores"][t].cpu()), _bits(z)), (t, int((_bits(res["scores"][t].cpu()) != _bits(z)).sum()))
        for b in range(B):
            tok = int(seq[b, t])
            assert tok == (PAD if done[b] else _argmax(z[b])), (b, t, seq.tolist())
            done[b] = done[b] or tok == EOS
        if states is not None:
            states = [C.advance(table, s, int(k)) for s, k in zip(states, seq[:, t])]
    print(f"elements of the replayed scores whose bits differ under the all-CPU rule: {cpu_diff}")


@pytest.mark.parametrize("B", [1, 2])
def test_neutral_keywords_take_the_plain_path(B):
    cfg, model, kw = _kw(B)
    plain = _plain(B)
    for _ in range(2):  # (a shape's second sighting captures its prefill: after two more plain calls everything the plain path captures is captured)
        assert torch.equal(model.generate(**kw).cpu(), plain)
    n_graphs = (len(model._dstate.graphs), len(model._prefill_graphs))
    for neutral in (dict(guidance_scale=None), dict(guidance_scale=1.0), dict(guidance_scale=1.0, negative_prompt_ids=NEG_TEXT)):
        assert torch.equal(model.generate(**kw, **neutral).cpu(), plain), neutral
        assert model._mode.guided is False and (len(model._dstate.graphs), len(model._prefill_graphs)) == n_graphs, neutral


@pytest.mark.parametrize("B", [1, 2])
def test_exact_replay_with_a_text_only_negative(B):
    cfg, model, kw = _kw(B, return_dict_in_generate=True, output_logits=True, output_scores=True)
    res = model.generate(**kw, guidance_scale=3.0, negative_prompt_ids=NEG_TEXT)
    torch.cuda.synchronize()
    model.check_device_errors()
    assert model._mode.guided is True
    _replay(res, B, 3.0)
    # ... and in front of repetition penalty, a constraint and under the cutoff, together
    first = [int(t) for t in res["sequences"][:, 0]]
    choices = [[first[0], 200, 201], [first[-1], 202], [203]]
    more = dict(repetition_penalty=1.3, guided_choice=choices, guidance_cutoff=0.001)
    res2 = model.generate(**kw, guidance_scale=3.0, negative_prompt_ids=NEG_TEXT, **more)
    req = request.parse(dict(kw, guidance_scale=3.0, negative_prompt_ids=NEG_TEXT, **more), model.config, batch=B)
    _replay(res2, B, 3.0, 0.001, rules=req.rules, table=req.constraint)
    assert res2["constraint_complete"].shape == (B,)
    # the feature does something: greedy tokens under guidance_scale = 3 against a text-only negative differ from the plain call's (prompts: fixtures seeds 2 / 0, 1)
    plain = _plain(B)
    w = min(plain.shape[1], res["sequences"].shape[1])
    assert plain.shape != res["sequences"].shape or not torch.equal(plain[:, :w], res["sequences"].cpu()[:, :w]), (plain.tolist(), res["sequences"].tolist())


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("B", [1, 2])
def test_the_pair_shares_one_history(B, sampled):
    """The negative rows ARE the prompts (same ids, same images): both rows of a pair must then compute the same bits at every step -- which they only do while the
    negative row is fed its prompt's token (dl_pair_follow; a sampled pair draws from two random streams) -- and g = lu."""
    cfg, model, kw = _kw(B, return_dict_in_generate=True, output_logits=True)
    neg = dict(negative_prompt_ids=kw["inputs"], negative_images=kw["images"])
    if "attention_mask" in kw:
        neg["negative_prompt_attention_mask"] = kw["attention_mask"]
    draw = dict(do_sample=True, seed=11, temperature=1.3) if sampled else {}
    res = model.generate(**kw, guidance_scale=3.0, **neg, **draw)
    assert len(res["logits"]) == res["sequences"].shape[1] > 1
    for t, (c, u) in enumerate(zip(res["logits"], res["negative_logits"])):
        assert torch.equal(_bits(c), _bits(u)), (t, "the two rows of a pair left their common history")
    if not sampled:
        # g = lu = lc, monotone in the raw logits: every token is the lowest-index argmax of the step's raw logits (no route is compared) ...
        seq = res["sequences"].cpu()
        assert seq.tolist() == [[_argmax(z[b].cpu()) for z in res["logits"]] for b in range(B)]
        # ... which makes them the tokens of the plain call of the B prompts: the same prefill batch, and a decode step whose rows do not depend on their batch
        assert torch.equal(seq, _plain(B))
        # (The plain call of the same 2 B rows is NOT a reference for them: it prefills at batch 2 B, and the plain prefill is not batch-invariant for every row --
        # the ragged pair's second prompt gives other tokens in the plain call of 4 rows than in the plain call of 2.  What is checked of it is only a sanity check of
        # the plain path itself: a prompt's two copies in one batch say the same, and at least one prompt says what it says in the smaller batch.)
        twice = {k: torch.cat([kw[k], kw[k]]) for k in ("inputs", "images", "attention_mask") if k in kw}
        plain2 = model.generate(**dict(kw, **twice, return_dict_in_generate=False, output_logits=False)).cpu()
        assert torch.equal(plain2[:B], plain2[B:]) and bool((plain2[:B] == _plain(B)).all(dim=1).any())


@pytest.mark.parametrize("B", [1, 2])
def test_lengths_and_the_returned_cache(B):
    cfg, model, kw = _kw(B, return_dict_in_generate=True)
    res = model.generate(**kw, guidance_scale=2.0, negative_prompt_ids=NEG_TEXT)
    produced = res["sequences"].shape[1]
    pairs, out = model._cache_pool, res["past_key_values"]
    assert pairs is not None and pairs.batch == 2 * B and out.batch == B and out is not pairs and out.slab.data_ptr() != pairs.slab.data_ptr()
    steps = int(model._dstate.step[0])  # (the loop may have enqueued steps past the column at which every row had finished)
    lens = pairs.lens.cpu()
    assert steps >= produced
    for b in range(B):
        assert int(lens[0, B + b]) == NEG_TEXT.shape[1] + steps - 1 and pairs.full_len_host[B + b] == NEG_TEXT.shape[1] + steps - 1
        assert int(lens[1, B + b]) <= int(lens[0, B + b])
    assert torch.equal(out.lens.cpu(), lens[:, :B]) and out.full_len_host == pairs.full_len_host[:B]
    SL = pairs.sparse_layer
    for b in range(B):  # the live slots of either length group, bit for bit
        n_full, n_sparse = int(lens[0, b]), int(lens[1, b])
        assert torch.equal(_bits(out.slab[:SL, :, b, :, :n_full].float()), _bits(pairs.slab[:SL, :, b, :, :n_full].float()))
        assert torch.equal(_bits(out.slab[SL:, :, b, :, :n_sparse].float()), _bits(pairs.slab[SL:, :, b, :, :n_sparse].float()))


class Sink:
    def __init__(self):
        self.cols, self.ended = [], 0

    def put(self, t):
        self.cols.append(t.clone())

    def end(self):
        self.ended += 1


@pytest.mark.parametrize("B", [1, 2])
def test_the_streamer_sees_the_prompts_rows_only(B):
    """put() gets [B, 0] first, then one [B] column per column of `sequences` -- never a negative row -- at sync_every = 1 (every step a chunk of its own) and 3."""
    cfg, model, kw = _kw(B)
    want = model.generate(**kw, guidance_scale=3.0, negative_prompt_ids=NEG_TEXT).cpu()
    for sync_every in (1, 3):
        sink = Sink()
        got = model.generate(**kw, guidance_scale=3.0, negative_prompt_ids=NEG_TEXT, streamer=sink, sync_every=sync_every).cpu()
        assert torch.equal(got, want)
        assert sink.ended == 1 and tuple(sink.cols[0].shape) == (B, 0) and all(tuple(c.shape) == (B,) and c.dtype == torch.int64 for c in sink.cols[1:])
        assert torch.equal(torch.stack(sink.cols[1:], dim=1), got)


@pytest.mark.parametrize("B", [1, 2])
def test_the_returned_cache_continues_under_forward(B):
    """A guided call of T - 1 tokens returns the prompts' cache; forward() of its last token on that cache gives the logits the guided call of T tokens reports for
    the conditional rows at step T - 1 -- the same keys and values attended by a B-row step instead of a 2 B-row one, so equal up to the model dtype's rounding (a
    few bf16 ulps of the row's largest logit), not bit for bit -- and advances the cache's lengths by one."""
    cfg, model, kw = _kw(B, return_dict_in_generate=True, output_logits=True)
    kw.update(eos_token_id=None)
    g = dict(guidance_scale=2.0, negative_prompt_ids=NEG_TEXT)
    long = model.generate(**kw, **g)
    short = model.generate(**dict(kw, max_new_tokens=T - 1), **g)
    assert torch.equal(short["sequences"], long["sequences"][:, : T - 1])
    cache = short["past_key_values"]
    before = list(cache.full_len_host)
    out = model.forward(short["sequences"][:, -1:], past_key_values=cache)
    torch.cuda.synchronize()
    model.check_device_errors()
    got, ref = out.logits[:, -1].float().cpu(), long["logits"][T - 1].float().cpu()
    assert got.shape == ref.shape == (B, 320)
    tol = 4 * 2.0**-8 * ref.abs().max(dim=1, keepdim=True).values  # four bf16 ulps of the largest logit
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() / tol).max())
    assert cache.full_len_host == [n + 1 for n in before] and cache.lens[0].cpu().tolist() == cache.full_len_host


@pytest.mark.parametrize("B", [1, 2])
def test_one_graph_serves_every_setting(B):
    cfg, model, kw = _kw(B)
    a = model.generate(**kw, guidance_scale=3.0, negative_prompt_ids=NEG_TEXT).cpu()
    a2 = model.generate(**kw, guidance_scale=3.0, negative_prompt_ids=NEG_TEXT).cpu()  # the second sighting captures the prefills
    assert torch.equal(a, a2)
    n_graphs = (len(model._dstate.graphs), len(model._prefill_graphs))
    placed = [e for k, e in model._prefill_graphs.items() if "place" in k]
    assert sum(e["graph"] is not None for e in placed) >= 2  # both prefills, the prompts' and the negatives', are captured
    b = model.generate(**kw, guidance_scale=1.5, guidance_cutoff=0.2, negative_prompt_ids=NEG_TEXT).cpu()
    assert (len(model._dstate.graphs), len(model._prefill_graphs)) == n_graphs and b.shape == a.shape  # another scale, a cutoff: device data
    c = model.generate(**kw, guidance_scale=3.0, negative_prompt_ids=NEG_TEXT).cpu()
    assert torch.equal(a, c)


@pytest.mark.parametrize("B", [1, 2])
def test_host_route_agrees_up_to_a_near_tie(B):
    """The same request on the plain loop over forward() (two streams, two caches): the same tokens, up to the first step at which the two largest guided scores
    lie closer than the rule's error bound (guidance.error_bound) allows two evaluations to differ."""
    cfg, model, kw = _kw(B, return_dict_in_generate=True, output_scores=True, output_logits=True)
    g = dict(guidance_scale=3.0, negative_prompt_ids=NEG_TEXT)
    dev = model.generate(**kw, **g)
    host = model.generate(**{k: v for k, v in kw.items() if k != "output_logits"}, **g, stopping_criteria=[lambda ids, scores: False])  # a callable criterion that never fires
    d, h = dev["sequences"].cpu(), host["sequences"].cpu()
    assert h.shape[0] == B and len(host["scores"]) == h.shape[1]
    for b in range(B):
        for t in range(min(d.shape[1], h.shape[1])):
            if int(d[b, t]) == int(h[b, t]):
                continue
            z = dev["scores"][t][b].float().cpu()
            top = torch.topk(z, 2)
            lc = torch.log_softmax(dev["logits"][t][b].double().cpu(), dim=-1)[top.indices]
            lu = torch.log_softmax(dev["negative_logits"][t][b].double().cpu(), dim=-1)[top.indices]
            bound = 2 * float(G.error_bound(3.0, lc, lu).sum())  # either score, in either evaluation
            print(f"row {b} diverges at step {t}: gap {float(top.values[0] - top.values[1]):.3e}, bound {bound:.3e}")
            assert float(top.values[0] - top.values[1]) <= bound, (b, t, float(top.values[0] - top.values[1]), bound)
            break  # (the histories differ from here on)


@pytest.mark.parametrize("B", [1, 2])
def test_refusals_come_before_any_launch(monkeypatch, B):
    from dynamic_llava_amd import hip_ops as ops

    cfg, model, kw = _kw(B)
    calls = []
    real = ops._check
    monkeypatch.setattr(ops, "_check", lambda rc, what: (calls.append(what), real(rc, what))[1])
    for bad, err in ((dict(guidance_scale=2.0), ValueError), (dict(guidance_scale=-1.0, negative_prompt_ids=NEG_TEXT), ValueError),
                     (dict(guidance_scale=2.0, negative_prompt_ids=NEG_TEXT, guidance_cutoff=1.5), ValueError), (dict(guidance_cutoff=0.5), ValueError),
                     (dict(guidance_scale=2.0, negative_prompt_ids=NEG_TEXT, num_return_sequences=2, do_sample=True, seed=1), NotImplementedError),
                     (dict(guidance_scale=2.0, negative_prompt_ids=NEG_TEXT, past_key_values=object()), NotImplementedError)):
        with pytest.raises(err):
            model.generate(**kw, **bad)
    with pytest.raises(ValueError, match="score"):
        model.score(kw["inputs"], torch.tensor([[5, 6]] * B), images=kw["images"], guidance_scale=2.0)
    assert calls == []
