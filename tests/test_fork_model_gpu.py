"""GPU, model level: generate(do_sample=True, seed=s, num_return_sequences=n) on the tiny config of oracle/fixtures.py (text predictor on: rows evict) -- one prefill of
the B prompts, dl_kv_fork into B * n decode rows, n different first draws from one logits row.

What is compared exactly (torch.equal): the forked K/V, lengths and first-step logits against a plain call of the same prompts -- a fork is a copy, and the prefill is
the plain call's prefill; tokens across graph states, schedules and repeated calls; the host route against the prompts repeated by hand.  The draws are replayed with
sampling.reference_step under the two-sided acceptance of tests/test_sampling_gpu.py (derived in that module's docstring), with the counter row base + b * n + r."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_sampling_gpu as tsg  # noqa: E402  (the model builder, the B = 1 / ragged B = 2 inputs and the draw check of the sampler's own tests)

N = 3
_MODELS = {}


@pytest.fixture(autouse=True, scope="module")
def _release_models():
    """The shared models live as long as this module's tests (a model that served requests is an object cycle: collected here, not inside somebody's stream capture)."""
    yield
    _MODELS.clear()
    gc.collect()
    torch.cuda.synchronize()


def _model(dtype, kv=None):
    if (dtype, kv) not in _MODELS:
        cfg, model = tsg._model(dtype)
        if kv is not None:
            model.set_kv_cache_format(kv)
        _MODELS[(dtype, kv)] = (cfg, model)
    return _MODELS[(dtype, kv)]


def _arrays(cache):
    """The storage arrays of a cache, [L, 2, B, nKV, T, w]: the slab, and with MXFP8 the scale bytes."""
    return [cache.slab] + ([cache.scales] if cache.kv_format == "mxfp8" else [])


def _check_forked_kv(model, inp, B, n):
    """(a): lengths, live K/V slots of every layer and the first-step logits of every replica row against a plain call of the B prompts."""
    plain = model.generate(**inp, max_new_tokens=1, eos_token_id=None, return_dict_in_generate=True)
    pc, p_logits = plain["past_key_values"], model.last_prefill_logits.clone()
    res = model.generate(**inp, max_new_tokens=1, eos_token_id=None, do_sample=True, seed=4, temperature=5.0, num_return_sequences=n, return_dict_in_generate=True)
    fc, f_logits = res["past_key_values"], model.last_prefill_logits.clone()
    assert res["sequences"].shape == (B * n, 1) and fc.batch == B * n and pc.batch == B and fc.kv_format == pc.kv_format == model.kv_cache_format
    assert p_logits.shape[0] == B and f_logits.shape[0] == B * n
    assert torch.equal(fc.lens, pc.lens.repeat_interleave(n, dim=1)) and fc.full_len_host == [v for v in pc.full_len_host for _ in range(n)]
    lens = pc.lens.cpu().tolist()
    assert min(lens[1]) > 0 and max(lens[0]) > max(lens[1]), "the prompts hold live rows in both groups, fewer where the image tokens were dropped"
    for fa, pa in zip(_arrays(fc), _arrays(pc)):
        for l in range(pc.n_layers):
            for b in range(B):
                m = lens[pc.group(l)][b]
                for r in range(n):
                    assert torch.equal(fa[l, :, b * n + r, :, :m], pa[l, :, b, :, :m]), (l, b, r)
    for b in range(B):
        for r in range(n):
            assert torch.equal(f_logits[b * n + r], p_logits[b]), (b, r)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_forked_kv_and_logits_are_the_plain_prefills(dtype, B):
    cfg, model = _model(dtype)
    _check_forked_kv(model, tsg._inputs(cfg, B, dtype), B, N)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_draw_of_every_replica_replays_from_the_scores(dtype, B):
    """(b): row b * n + r draws with counter row base + b * n + r at every step, on that step's reported logits."""
    cfg, model = _model(dtype)
    T, k, p, seed, base_row, steps = 1.5, 200, 0.8, 31, 3, 8
    kw = dict(tsg._inputs(cfg, B, dtype), max_new_tokens=steps, eos_token_id=None, do_sample=True, temperature=T, top_k=k, top_p=p, seed=seed, sample_row_base=base_row, num_return_sequences=N)
    res = model.generate(**kw, return_dict_in_generate=True, output_scores=True, output_logits=True)
    seq = res["sequences"].cpu()
    assert seq.shape == (B * N, steps) and len(res["scores"]) == len(res["logits"]) == steps and res["scores"][0].shape[0] == res["logits"][0].shape[0] == B * N
    stats = dict(band_max=0, draws=0, margin=0)
    for i in range(steps):
        raw, sc = res["logits"][i].cpu().to(dtype), res["scores"][i].cpu()
        for row in range(B * N):
            tsg._check_row(raw[row], T, k, p, (), seed, row, seq[row, i : i + 1], sc[row] > float("-inf"), stats, row_base=base_row, step0=i)
        for b in range(B):  # step 0: the n rows of a prompt draw from ONE logits row
            assert i > 0 or all(torch.equal(raw[b * N + r], raw[b * N]) for r in range(N))
    assert stats["margin"] == 0 or stats["draws"] >= 1000 * stats["margin"]
    assert torch.equal(model.generate(**kw).cpu(), seq), "the same request without the step-by-step outputs draws the same tokens"


def _top1_rows(model, kw, B, n):
    """top_k = 1 -> the tokens [B * n, T]: every row emits a member of its step's top tie class, and the n rows of a prompt, which carry one history, emit the same
    token.  top-k keeps the WHOLE tie class at its threshold (sampling.py, rule 2: HF's `z < kth`), so where a row's largest logit is tied -- 16-bit logits do tie --
    the rows may draw different members of the class, and that prompt's histories are compared no further."""
    res = model.generate(**kw, do_sample=True, seed=5, temperature=0.7, top_k=1, num_return_sequences=n, return_dict_in_generate=True, output_logits=True)
    seq = res["sequences"]
    assert seq.shape == (B * n, kw["max_new_tokens"]) and len(res["logits"]) == seq.shape[1]
    for b in range(B):
        rows = range(b * n, b * n + n)
        for i, z in enumerate(res["logits"]):
            tops = [z[r] == z[r].max() for r in rows]
            assert all(bool(t[seq[r, i]]) for r, t in zip(rows, tops)), (b, i)
            if any(int(t.sum()) > 1 for t in tops):
                print(f"prompt {b}, step {i}: the largest logit is tied")
                break
            assert all(int(seq[r, i]) == int(seq[b * n, i]) for r in rows), (b, i)
    return seq


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_degenerate_rows_agree_and_hot_rows_differ(dtype, B):
    """(c)"""
    cfg, model = _model(dtype)
    kw = dict(tsg._inputs(cfg, B, dtype), max_new_tokens=10, eos_token_id=None)
    one = _top1_rows(model, kw, B, N)
    if dtype == torch.float32:
        for b in range(B):
            assert all(torch.equal(one[b * N + r], one[b * N]) for r in range(N)), b
        assert torch.equal(one[::N], model.generate(**kw))  # (16-bit: a decode batch of B * n rows and one of B rows run different GEMM kernels -- equal rounding class, not equal bits)
    hot = model.generate(**kw, do_sample=True, seed=5, temperature=5.0, num_return_sequences=N)
    for b in range(B):
        assert len({tuple(hot[b * N + r].tolist()) for r in range(N)}) >= 2, b


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graph_states_and_schedules_give_the_same_tokens(dtype, B):
    """(d)"""
    cfg, model = _model(dtype)
    kw = dict(tsg._inputs(cfg, B, dtype), max_new_tokens=20, eos_token_id=None, do_sample=True, temperature=5.0, top_p=0.95, seed=11, num_return_sequences=N)
    base = model.generate(**kw)  # eager (or a replay, when an earlier test left the graphs)
    assert base.shape == (B * N, 20)
    assert torch.equal(model.generate(**kw), base) and torch.equal(model.generate(**kw), base)  # capture, replay
    st = model._dstate
    n_dec, n_pre, n_cap = len(st.graphs), len(model._prefill_graphs), sum(e["graph"] is not None for e in model._prefill_graphs.values())
    assert st.B == B * N and n_dec >= 1 and n_cap >= 1
    other = model.generate(**dict(kw, seed=12, temperature=0.7))
    assert not torch.equal(other, base)
    assert (len(st.graphs), len(model._prefill_graphs), sum(e["graph"] is not None for e in model._prefill_graphs.values())) == (n_dec, n_pre, n_cap) and model._dstate is st
    for se in (1, 64):
        assert torch.equal(model.generate(**kw, sync_every=se), base), se
    model.use_hip_graph = False
    try:
        assert torch.equal(model.generate(**kw), base)
    finally:
        model.use_hip_graph = True


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_plain_calls_are_what_they_were(dtype):
    """(e): a plain sampled and a greedy call before and after forked ones; the entries they leave behind are no more than before."""
    cfg, model = _model(dtype)
    kw = dict(tsg._inputs(cfg, 2, dtype), max_new_tokens=10, eos_token_id=None)
    counts = lambda: (len(model._dstate.graphs), len(model._prefill_graphs), sum(e["graph"] is not None for e in model._prefill_graphs.values()))
    model._dstate = None
    model._prefill_graphs = {}
    for _ in range(3):
        greedy, sampled = model.generate(**kw), model.generate(**kw, do_sample=True, seed=3, temperature=5.0)
    before = counts()
    for n in (2, 3):
        assert model.generate(**kw, do_sample=True, seed=3, temperature=5.0, num_return_sequences=n).shape == (2 * n, 10)
    for _ in range(3):
        assert torch.equal(model.generate(**kw), greedy) and torch.equal(model.generate(**kw, do_sample=True, seed=3, temperature=5.0), sampled)
    after = counts()
    assert all(a <= b for a, b in zip(after, before)), (before, after)
    assert model._dstate.B == 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_logprobs_have_a_row_per_replica_and_an_eos_pads_only_its_row(dtype):
    """(f)"""
    cfg, model = _model(dtype)
    B, T, pad = 2, 12, 7
    kw = dict(tsg._inputs(cfg, B, dtype), max_new_tokens=T, do_sample=True, seed=21, temperature=5.0, num_return_sequences=N, pad_token_id=pad, return_dict_in_generate=True, output_logprobs=True, top_logprobs=2)
    free = model.generate(**kw, eos_token_id=None)
    seq = free["sequences"].cpu()
    assert seq.shape == (B * N, T) and free["logprobs"].shape == (B * N, T) and free["top_logprobs"].shape == free["top_logprob_ids"].shape == (B * N, T, 2)
    assert free["past_key_values"].batch == B * N
    assert bool((free["logprobs"] < 0).all())
    # an EOS id that exactly one replica emits, once, and not as its last token
    hit = [(r, j) for r in range(B * N) for j in range(1, T - 1) if int((seq == seq[r, j]).sum()) == 1 and int(seq[r, j]) != pad]
    assert hit, "no token of this run is unique to one row"
    r0, j0 = hit[0]
    res = model.generate(**kw, eos_token_id=int(seq[r0, j0]))
    out = res["sequences"].cpu()
    assert out.shape == (B * N, T), "the other rows never finish: nothing is trimmed"
    others = [r for r in range(B * N) if r != r0]
    assert torch.equal(out[others], seq[others]) and torch.equal(out[r0, : j0 + 1], seq[r0, : j0 + 1]) and out[r0, j0 + 1 :].tolist() == [pad] * (T - j0 - 1)
    lp = res["logprobs"].cpu()
    assert bool((lp[r0, j0 + 1 :] == 0).all()) and float(lp[r0, j0]) < 0 and bool((lp[others] < 0).all())
    assert bool((res["top_logprob_ids"][r0, j0 + 1 :] == -1).all())


@pytest.mark.parametrize("B", [1, 2])
def test_mxfp8_kv_cache_forks_codes_and_scales(B):
    """(g): set_kv_cache_format("mxfp8") -- (a) on the codes and on the scale bytes, and (c)."""
    dtype = torch.bfloat16
    cfg, model = _model(dtype, "mxfp8")
    inp = tsg._inputs(cfg, B, dtype)
    _check_forked_kv(model, inp, B, N)
    kw = dict(inp, max_new_tokens=10, eos_token_id=None)
    _top1_rows(model, kw, B, N)
    hot = model.generate(**kw, do_sample=True, seed=5, temperature=5.0, num_return_sequences=N)
    assert hot.shape == (B * N, 10)
    for b in range(B):
        assert len({tuple(hot[b * N + r].tolist()) for r in range(N)}) >= 2, b
    assert torch.equal(model.generate(**kw, do_sample=True, seed=5, temperature=5.0, num_return_sequences=N), hot)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_host_route_repeats_the_prompts(dtype):
    """(h): generator= -- the plain loop over forward() on every prompt n times in the batch, no fork."""
    cfg, model = _model(dtype)
    inp = tsg._inputs(cfg, 2, dtype)
    kw = dict(max_new_tokens=8, eos_token_id=None, do_sample=True, temperature=5.0, top_p=0.95)
    got = model.generate(**inp, **kw, generator=torch.Generator(device="cuda").manual_seed(7), num_return_sequences=2)
    by_hand = model.generate(**{k: v.repeat_interleave(2, dim=0) for k, v in inp.items()}, **kw, generator=torch.Generator(device="cuda").manual_seed(7))
    assert got.shape == (4, 8) and torch.equal(got, by_hand)
    assert len({tuple(r.tolist()) for r in got[:2]}) == 2, "the two answers of prompt 0 are drawn separately"
