"""GPU, model level: generate(stop_sequences= / stopping_criteria= / streamer=) on the tiny config of oracle/fixtures.py.  A stopped run is the unstopped run cut at
the rule's finish columns (dynamic_llava_amd/stopping.py): every comparison here is exact -- tokens equal, logits and log-probabilities bit for bit."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import stopping  # noqa: E402
from dynamic_llava_amd.decode import StepMode  # noqa: E402

T, PAD = 12, 1
_MODELS = {}


@pytest.fixture(autouse=True, scope="module")
def _release_models():
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


def _same_logits(a, b):
    return len(a) == len(b) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


class Keywords:
    """What generate() reads of the reference's KeywordsStoppingCriteria."""

    def __init__(self, seqs):
        self.keyword_ids = [torch.tensor(s) for s in seqs]


class Recorder:
    def __init__(self):
        self.puts, self.ends = [], 0

    def put(self, t):
        assert self.ends == 0 and t.device.type == "cpu" and t.dtype == torch.int64
        self.puts.append(t.clone())

    def end(self):
        self.ends += 1


def _check_stream(rec, sequences):
    seq = sequences.cpu()
    B, W = seq.shape
    assert rec.ends == 1 and len(rec.puts) == W + 1, (rec.ends, len(rec.puts), W)
    assert rec.puts[0].shape == (B, 0)
    for j in range(W):
        assert rec.puts[j + 1].shape == (B,) and torch.equal(rec.puts[j + 1], seq[:, j]), j


def _fresh_pair(row, start=2):
    """The first position p >= start of a row of tokens whose pair (row[p - 1], row[p]) does not occur earlier in it -> (p, the pair)."""
    row = [int(t) for t in row]
    for p in range(start, len(row)):
        if all((row[q - 1], row[q]) != (row[p - 1], row[p]) for q in range(1, p)):
            return p, [row[p - 1], row[p]]
    return None


def _ragged_stops(S, starts):
    """One fresh pair per row of the unstopped run S, row b's looked for from starts[b] on -> (stops, the rule's finish columns on S): ragged, all inside the run."""
    picks = [_fresh_pair(S[b], starts[b]) for b in range(S.shape[0])]
    assert all(p is not None for p in picks), S.tolist()
    stops = [p[1] for p in picks]
    finish = stopping.finish_columns(S.cpu(), (), [tuple(s) for s in stops])
    assert int(finish.max()) < S.shape[1] - 1 and len(set(finish.tolist())) > 1, (finish.tolist(), S.tolist())
    return stops, finish


def _cut(S, finish, pad=PAD):
    """The unstopped run cut at the finish columns: pad behind a row's finish, trimmed where the last row finishes."""
    want = S.cpu().clone()[:, : int(finish.max()) + 1]
    for b in range(want.shape[0]):
        want[b, int(finish[b]) + 1 :] = pad
    return want


def _never(S, k):
    """k one-token sequences that no row of S contains."""
    used = set(S.reshape(-1).tolist())
    return [[v] for v in range(2, 300) if v not in used][:k]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_b1_greedy_stops_at_the_sequence(dtype):
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, 1, dtype), max_new_tokens=T, eos_token_id=None, pad_token_id=PAD, return_dict_in_generate=True, output_logits=True)
    free = model.generate(**kw)
    S = free["sequences"].cpu()
    assert S.shape == (1, T)
    pick = _fresh_pair(S[0])
    assert pick is not None, S.tolist()
    p, pair = pick
    res = model.generate(**kw, stop_sequences=[pair])
    torch.cuda.synchronize()
    model.check_device_errors()
    assert model._mode.stop is True
    assert torch.equal(res["sequences"].cpu(), S[:, : p + 1]), (res["sequences"].tolist(), S.tolist(), p)
    assert _same_logits(res["logits"], free["logits"][: p + 1])
    plain = model.generate(**{k: v for k, v in kw.items() if k not in ("return_dict_in_generate", "output_logits")}, stop_sequences=[torch.tensor(pair)])
    assert torch.equal(plain.cpu(), S[:, : p + 1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_b3_rows_stop_at_their_own_columns(dtype):
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, 3, dtype), max_new_tokens=T, eos_token_id=None, pad_token_id=PAD)
    S = model.generate(**kw).cpu()
    stops, finish = _ragged_stops(S, (2, 4, 7))
    for sync in (None, 1, 3):
        got = model.generate(**kw, stop_sequences=stops, **({} if sync is None else {"sync_every": sync})).cpu()
        assert torch.equal(got, _cut(S, finish)), (sync, got.tolist(), S.tolist(), finish.tolist())
    for b in range(3):
        assert torch.equal(got[b, : int(finish[b]) + 1], S[b, : int(finish[b]) + 1])


def test_equivalent_forms_and_routes():
    """fp32: graph and eager runs, the host route (the list padded past the cap with sequences that never match), a keyword criterion and a callable criterion that
    states the same rule all return the device route's result."""
    dtype = torch.float32
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, 3, dtype), max_new_tokens=T, eos_token_id=None, pad_token_id=PAD, return_dict_in_generate=True, output_logits=True)
    S = model.generate(**kw)["sequences"].cpu()
    stops, finish = _ragged_stops(S, (2, 4, 7))
    want = _cut(S, finish)
    dev = model.generate(**kw, stop_sequences=stops)
    assert torch.equal(dev["sequences"].cpu(), want)
    try:
        model.use_hip_graph = False
        eager = model.generate(**kw, stop_sequences=stops)
    finally:
        model.use_hip_graph = True
    assert torch.equal(eager["sequences"], dev["sequences"]) and _same_logits(eager["logits"], dev["logits"])
    crit = model.generate(**kw, stopping_criteria=[Keywords(stops)])
    assert torch.equal(crit["sequences"], dev["sequences"]) and _same_logits(crit["logits"], dev["logits"])
    both = model.generate(**kw, stop_sequences=stops[:1], stopping_criteria=[Keywords(stops[1:])])
    assert torch.equal(both["sequences"], dev["sequences"])
    # the host route: nine sequences
    hk = {k: v for k, v in kw.items() if k != "output_logits"}
    long_list = stops + _never(S, 9 - len(stops))
    assert len(long_list) == 9 and not stopping.device_route(stopping.normalize(dict(stop_sequences=long_list), cfg.vocab_size))
    host = model.generate(**hk, stop_sequences=long_list)
    assert torch.equal(host["sequences"].cpu(), want)
    # a callable: the host route, called once per step on the tokens generated in this call
    calls = []

    def rule(ids, scores):
        calls.append(tuple(ids.shape))
        return torch.tensor([stopping.tail_matches(r, [tuple(s) for s in stops]) for r in ids.tolist()])

    rec = Recorder()
    called = model.generate(**hk, stopping_criteria=[rule], streamer=rec)
    assert torch.equal(called["sequences"].cpu(), want) and calls == [(3, t + 1) for t in range(want.shape[1])]
    _check_stream(rec, called["sequences"])


@pytest.mark.parametrize("case", ["sampled", "return_sequences", "penalty", "eos_too"])
def test_combinations(case):
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    B = 2
    more = {"sampled": dict(do_sample=True, seed=5, temperature=0.9, top_k=40), "return_sequences": dict(do_sample=True, seed=7, temperature=0.9, num_return_sequences=2),
            "penalty": dict(repetition_penalty=1.3), "eos_too": dict()}[case]
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=T, eos_token_id=None, pad_token_id=PAD, **more)
    S = model.generate(**kw).cpu()
    rows = S.shape[0]
    assert rows == (4 if case == "return_sequences" else 2)
    stops, finish = _ragged_stops(S, (6, 3) if case == "eos_too" else (3, 6, 2, 8)[:rows])
    if case == "eos_too":  # row 0 ends on an EOS id in front of its stop sequence; row 1 never emits that id
        c = next((c for c in range(1, 5) if int(S[0, c]) not in S[0, :c].tolist() and int(S[0, c]) not in S[1].tolist()), None)
        assert c is not None, S.tolist()
        kw["eos_token_id"] = int(S[0, c])
        without = finish.tolist()
        finish = stopping.finish_columns(S, (int(S[0, c]),), [tuple(s) for s in stops])
        assert int(finish[0]) == min(c, without[0]) and int(finish[1]) == without[1] and finish.tolist() != without
    got = model.generate(**kw, stop_sequences=stops).cpu()
    assert torch.equal(got, _cut(S, finish)), (case, got.tolist(), S.tolist(), finish.tolist())


def test_logprobs_behind_a_stop_finished_row():
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, 3, dtype), max_new_tokens=T, eos_token_id=None, pad_token_id=PAD, return_dict_in_generate=True, output_logprobs=True, top_logprobs=3)
    free = model.generate(**kw)
    S = free["sequences"].cpu()
    stops, finish = _ragged_stops(S, (2, 4, 7))
    res = model.generate(**kw, stop_sequences=stops)
    W = int(finish.max()) + 1
    assert torch.equal(res["sequences"].cpu(), _cut(S, finish)) and res["logprobs"].shape == (3, W) and res["top_logprobs"].shape == (3, W, 3)
    for b in range(3):
        c = int(finish[b]) + 1
        for k in ("logprobs", "top_logprobs"):
            assert torch.equal(_bits(res[k][b, :c]), _bits(free[k][b, :c])), (k, b)
            assert bool((res[k][b, c:] == 0.0).all()), (k, b)
        assert torch.equal(res["top_logprob_ids"][b, :c], free["top_logprob_ids"][b, :c]) and bool((res["top_logprob_ids"][b, c:] == -1).all())


def test_one_graph_serves_every_list_and_no_op_values_are_the_plain_request():
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, 3, dtype), max_new_tokens=T, eos_token_id=None, pad_token_id=PAD)
    S = model.generate(**kw).cpu()
    plain_mode = model._mode
    assert plain_mode == StepMode(eos=-1, pad=PAD, min_new=0)
    stops, finish = _ragged_stops(S, (2, 4, 7))
    for _ in range(3):  # (a prompt shape's prefill is captured at its second sighting)
        assert torch.equal(model.generate(**kw, stop_sequences=stops).cpu(), _cut(S, finish))
    count = lambda: (len(model._dstate.graphs), sum(e["graph"] is not None for e in model._prefill_graphs.values()), len(model._prefill_graphs))
    before = count()
    other, finish2 = _ragged_stops(S, (5, 2, 3))
    assert other != stops
    assert torch.equal(model.generate(**kw, stop_sequences=other).cpu(), _cut(S, finish2))
    one = [[int(S[1, 0])]]  # a one-token sequence: row 1 stops at column 0
    f1 = stopping.finish_columns(S, (), [tuple(one[0])])
    assert int(f1[1]) == 0
    assert torch.equal(model.generate(**kw, stop_sequences=one).cpu(), _cut(S, f1))
    assert count() == before, (count(), before)
    # None and [] are the request without the keyword: the same mode (so the same graphs) and the same bits
    dk = dict(kw, return_dict_in_generate=True, output_logits=True)
    ref = model.generate(**dk)
    for v in (None, []):
        res = model.generate(**dk, stop_sequences=v, stopping_criteria=v)
        assert model._mode == plain_mode and torch.equal(res["sequences"], ref["sequences"]) and _same_logits(res["logits"], ref["logits"])


@pytest.mark.parametrize("sync", [1, 3, 8])
def test_streamer_receives_the_columns_of_sequences(sync):
    dtype = torch.bfloat16
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, 3, dtype), max_new_tokens=T, eos_token_id=None, pad_token_id=PAD, sync_every=sync)
    S = model.generate(**kw).cpu()
    n_graphs = len(model._dstate.graphs)
    rec = Recorder()
    got = model.generate(**kw, streamer=rec)
    assert torch.equal(got.cpu(), S) and len(model._dstate.graphs) == n_graphs
    _check_stream(rec, got)
    # every row ends on an EOS id inside a chunk: the columns the device ran past that step are never put
    col = 5
    eos = sorted({int(t) for t in S[:, col]})
    first = stopping.finish_columns(S, eos, ())
    assert len(eos) <= 3 and int(first.max()) < T - 1
    ek = dict(kw, eos_token_id=eos, return_dict_in_generate=True, output_logits=True)
    ref = model.generate(**ek)
    rec = Recorder()
    res = model.generate(**ek, streamer=rec)
    assert res["sequences"].shape[1] == int(first.max()) + 1 and torch.equal(res["sequences"], ref["sequences"]) and _same_logits(res["logits"], ref["logits"])
    _check_stream(rec, res["sequences"])
    # with stop sequences, ragged
    stops, finish = _ragged_stops(S, (2, 4, 7))
    rec = Recorder()
    cut = model.generate(**kw, stop_sequences=stops, streamer=rec)
    assert torch.equal(cut.cpu(), _cut(S, finish))
    _check_stream(rec, cut)
