"""CPU: the stopping rule (dynamic_llava_amd/stopping.py, the contract of dl_decode_stop) -- normalize and its caps, finish_columns on hand-made tables, the host
loop with stop sequences, host criteria and a streamer against a plain restatement, the routes such requests take, the step mode of a request without the
keywords, the installed transformers' EosTokenCriteria on a one-token stop sequence, and the C entry's argument checks (no device: nothing is launched)."""
import ctypes
import os
import re

import pytest
import torch

from dynamic_llava_amd import request, stopping
from dynamic_llava_amd.config import DynamicLlavaConfig
from dynamic_llava_amd.decode import StepMode
from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM
from oracle import fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 320


class Keywords:
    """A stand-in for the reference's KeywordsStoppingCriteria: what generate() reads of it is `keyword_ids`, a list of 1-D tensors."""

    def __init__(self, *seqs):
        self.keyword_ids = [torch.tensor(s) for s in seqs]

    def __call__(self, ids, scores, **kw):
        raise AssertionError("a keyword criterion is matched by its ids, never called")


class Recorder:
    def __init__(self):
        self.puts, self.ends = [], 0

    def put(self, t):
        assert self.ends == 0 and t.device.type == "cpu" and t.dtype == torch.int64
        self.puts.append(t.clone())

    def end(self):
        self.ends += 1


def check_stream(rec, sequences):
    """The streamer contract: an empty [B, 0] tensor, then every column of `sequences` in order and once each, then one end()."""
    seq = sequences.cpu()
    B, W = seq.shape
    assert rec.ends == 1 and len(rec.puts) == W + 1
    assert rec.puts[0].shape == (B, 0)
    for j in range(W):
        assert rec.puts[j + 1].shape == (B,) and torch.equal(rec.puts[j + 1], seq[:, j]), j


def _tiny():
    cfg = fx.tiny_config()
    return cfg, DynamicLlavaConfig.from_namespace(cfg)


# ---- normalize ------------------------------------------------------------------------------------------------------------------------------------
def test_caps_and_no_op_values():
    assert (stopping.MAX_STOPS, stopping.MAX_STOP_LEN) == (8, 8)
    for kw in (dict(), dict(stop_sequences=None), dict(stop_sequences=[]), dict(stop_sequences=()), dict(stopping_criteria=None), dict(stopping_criteria=[])):
        assert stopping.normalize(kw, V) == () and stopping.host_criteria(kw) == ()


@pytest.mark.parametrize("bad", [[[]], [[1], []], [[V]], [[-1]], [[1, 2.0]], [[True]], [["a"]], [5], "ab", [torch.tensor([1.0])], [torch.tensor([[1]])], [torch.tensor([V])],
                                 [torch.tensor([], dtype=torch.long)], [torch.tensor([True])], 7], ids=repr)
def test_normalize_refuses(bad):
    with pytest.raises(ValueError):
        stopping.normalize(dict(stop_sequences=bad), V)
    if isinstance(bad, list) and bad and not isinstance(bad[0], int):
        with pytest.raises(ValueError):
            stopping.normalize(dict(stopping_criteria=[type("K", (), {"keyword_ids": bad})()]), V)


def test_normalize_sources_and_order():
    kw = dict(stop_sequences=[[3, 4], torch.tensor([5]), (6, 7, 8), torch.tensor([9, 9], dtype=torch.int32)], stopping_criteria=[Keywords([3, 4], [V - 1]), len, Keywords([0])])
    assert stopping.normalize(kw, V) == ((3, 4), (5,), (6, 7, 8), (9, 9), (3, 4), (V - 1,), (0,))  # concatenated in order, duplicates kept
    assert stopping.host_criteria(kw) == (len,)
    assert stopping.normalize(dict(stopping_criteria=[Keywords([3, 4], [5])]), V) == stopping.normalize(dict(stop_sequences=[[3, 4], [5]]), V)
    with pytest.raises(ValueError):
        stopping.host_criteria(dict(stopping_criteria=[3]))
    with pytest.raises(ValueError):
        stopping.normalize(dict(stopping_criteria=Keywords([1])), V)  # not a list


def test_cap_boundaries():
    eight, nine = [[i + 1] for i in range(8)], [[i + 1] for i in range(9)]
    assert stopping.device_route(stopping.normalize(dict(stop_sequences=eight), V)) and not stopping.device_route(stopping.normalize(dict(stop_sequences=nine), V))
    assert stopping.device_route(((1,) * 8,)) and not stopping.device_route(((1,) * 9,))
    assert stopping.device_route(()) and stopping.device_route(tuple((i,) * 8 for i in range(8)))
    assert not stopping.device_route(stopping.normalize(dict(stop_sequences=eight[:4], stopping_criteria=[Keywords(*nine[:5])]), V))  # the caps count both sources


# ---- finish_columns ---------------------------------------------------------------------------------------------------------------------------------
def _restated_finish(out, eos, stops):
    B, T = out.shape
    res = []
    for b in range(B):
        row, col = out[b].tolist(), T
        for c in range(T):
            if row[c] in eos or any(len(s) <= c + 1 and row[c + 1 - len(s) : c + 1] == list(s) for s in stops):
                col = c
                break
        res.append(col)
    return torch.tensor(res, dtype=torch.int64)


def test_finish_columns_hand_made():
    fc = stopping.finish_columns
    out = torch.tensor([[7, 1, 2, 3, 0, 0],   # a one-token stop at column 0
                        [1, 2, 9, 9, 9, 9],   # the sequence (3, 1, 2) is longer than what precedes column 1: no match across column 0
                        [5, 1, 2, 4, 4, 4],   # (1, 2) in the middle only
                        [4, 6, 1, 2, 4, 4],   # EOS (6) before the stop
                        [4, 1, 2, 6, 4, 4],   # the stop before EOS
                        [4, 4, 4, 4, 4, 4]])  # nothing
    stops = ((7,), (3, 1, 2), (1, 2))
    assert fc(out, (6,), stops).tolist() == [0, 1, 2, 1, 2, 6]
    assert fc(out, (), stops).tolist() == [0, 1, 2, 3, 2, 6]
    assert fc(out, (6,), ()).tolist() == [6, 6, 6, 1, 3, 6]
    assert fc(out, (), ()).tolist() == [6] * 6 and fc(out, None, None).tolist() == [6] * 6
    assert fc(out[:, :1], (), ((7,), (1, 2))).tolist() == [0, 1, 1, 1, 1, 1]  # a sequence longer than the row
    assert fc(torch.tensor([[1, 2, 3, 4, 5, 6, 7, 8, 9]]), (), (tuple(range(2, 10)),)).tolist() == [8] and fc(torch.tensor([[2, 3]]), (), ((1, 2, 3),)).tolist() == [2]
    assert fc(out[:, :0], (6,), stops).tolist() == [0] * 6
    g = torch.Generator().manual_seed(5)
    for _ in range(20):
        rnd = torch.randint(0, 3, (16, 12), generator=g)
        st = tuple(tuple(torch.randint(0, 3, (int(n),), generator=g).tolist()) for n in torch.randint(1, 9, (3,), generator=g))
        assert torch.equal(fc(rnd, (), st), _restated_finish(rnd, (), st)) and torch.equal(fc(rnd, (2,), st[:1]), _restated_finish(rnd, (2,), st[:1]))


def test_reference_flags_is_the_tail_rule():
    from dynamic_llava_amd import hip_ops

    out = torch.tensor([[1, 2, 1, 2], [2, 1, 2, 1], [1, 2, 0, 0], [1, 2, 1, 2]])
    step, fin = torch.tensor([4, 4, 2, 9], dtype=torch.int32), torch.tensor([0, 0, 0, 1], dtype=torch.int32)
    tab = hip_ops.stop_table_words(((1, 2), (2, 2, 1, 2)))
    assert tab.shape == (hip_ops.STOP_TABLE_WORDS,) and tab[0] == 2 and tab[8:11].tolist() == [2, 1, 2] and tab[17:22].tolist() == [4, 2, 2, 1, 2]
    assert stopping.reference_flags(out, step, fin, tab).tolist() == [1, 0, 1, 1]
    assert stopping.reference_flags(out, torch.zeros(4, dtype=torch.int32), fin, tab).tolist() == [0, 0, 0, 1]
    assert stopping.reference_flags(out, step, fin, hip_ops.stop_table_words(())).tolist() == [0, 0, 0, 1]
    with pytest.raises(hip_ops.HipOpsError):
        hip_ops.stop_table_words(((1,),) * 9)
    with pytest.raises(hip_ops.HipOpsError):
        hip_ops.stop_table_words(((1,) * 9,))


# ---- the host loop ------------------------------------------------------------------------------------------------------------------------------------
def _table(seed=0, B=3, Vt=16, steps=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((steps, B, Vt), generator=g) * 3.0


def _restated_loop(tab, max_new, eos=(), pad=0, stops=(), criteria=()):
    """The plain greedy loop with the stopping rule restated: per row, finished once its tokens end in a stop sequence / hold an EOS id / a criterion says so."""
    B = tab.shape[1]
    done, toks = [False] * B, []
    for step in range(max_new):
        pick = tab[step].argmax(dim=-1).tolist()
        toks.append([pad if done[b] else pick[b] for b in range(B)])
        ids = torch.tensor(toks).t()
        verdicts = [c(ids, tab[step]) for c in criteria]
        for b in range(B):
            hist = [t[b] for t in toks]
            done[b] = done[b] or hist[-1] in eos or any(len(s) <= len(hist) and hist[-len(s):] == list(s) for s in stops) or any(
                bool(v[b]) if torch.is_tensor(v) else bool(v) for v in verdicts)
        if all(done):
            break
    return torch.tensor(toks).t()


def _drive(tab, max_new, **kw):
    _, mcfg = _tiny()
    req = request.parse(dict(kw, max_new_tokens=max_new), mcfg)
    fed, finish = [], []

    def advance(nxt):
        fed.append(nxt.clone())
        return tab[len(fed)]

    toks, scores, raw = request.host_loop(tab[0], advance, req, max_new, True, finish)
    assert len(fed) == len(toks) - 1 and len(finish) == 1
    return req, torch.stack(toks, dim=1), finish[0]


def _free_run(tab, n):
    return torch.stack([tab[s].argmax(dim=-1) for s in range(n)], dim=1)


def test_host_loop_stops_rows_on_their_sequences():
    tab = _table(2)
    free = _free_run(tab, 8)
    stops = [free[0, 1:3].tolist(), free[1, 4:5].tolist(), free[2, 0:3].tolist()]  # row 0 ends at column 2, row 1 at 4 (unless sooner), row 2 at 2
    want = _restated_loop(tab, 8, pad=15, stops=stops)
    rec = Recorder()
    req, seq, finish = _drive(tab, 8, eos_token_id=None, pad_token_id=15, stop_sequences=stops, min_new_tokens=6, streamer=rec)  # (min_new_tokens holds nothing back)
    assert req.stops == tuple(map(tuple, stops)) and torch.equal(seq, want) and seq.shape[1] < 8
    assert torch.equal(finish, stopping.finish_columns(seq, (), req.stops)) and int(finish.max()) == seq.shape[1] - 1
    for b in range(3):
        c = int(finish[b])
        assert torch.equal(seq[b, : c + 1], free[b, : c + 1]) and bool((seq[b, c + 1 :] == 15).all())
    check_stream(rec, seq)
    # the same list through a keyword criterion; EOS and a stop together
    _, seq2, _ = _drive(tab, 8, eos_token_id=None, pad_token_id=15, stopping_criteria=[Keywords(*stops)])
    assert torch.equal(seq2, seq)
    eos = int(free[1, 1])
    _, seq3, fin3 = _drive(tab, 8, eos_token_id=eos, pad_token_id=15, stop_sequences=stops)
    assert torch.equal(seq3, _restated_loop(tab, 8, eos=(eos,), pad=15, stops=stops)) and torch.equal(fin3, stopping.finish_columns(seq3, (eos,), req.stops))


@pytest.mark.parametrize("kind", ["bool", "tensor"])
def test_host_loop_calls_host_criteria_once_per_step(kind):
    tab = _table(4)
    calls = []

    def make(log):
        def crit(ids, scores):
            if log is not None:
                log.append((tuple(ids.shape), tuple(scores.shape)))
            if kind == "bool":
                return ids.shape[1] >= 3  # every row, after three tokens
            return torch.tensor([ids.shape[1] >= 2, False, ids.shape[1] >= 5])  # per row

        return crit

    rec = Recorder()
    req, seq, finish = _drive(tab, 8, eos_token_id=None, pad_token_id=15, stopping_criteria=[make(calls)], streamer=rec)
    assert req.route == "host_greedy" and req.stops == () and len(req.criteria) == 1
    want = _restated_loop(tab, 8, pad=15, criteria=[make(None)])
    assert torch.equal(seq, want)
    assert calls == [((3, t + 1), (3, 16)) for t in range(seq.shape[1])]  # once per step, on the tokens generated in this call
    assert seq.shape[1] == (3 if kind == "bool" else 8) and finish.tolist() == ([2, 2, 2] if kind == "bool" else [1, 8, 4])
    if kind == "tensor":
        assert bool((seq[0, 2:] == 15).all()) and bool((seq[2, 5:] == 15).all())
    check_stream(rec, seq)


def test_host_loop_without_the_keywords_is_unchanged_and_streams():
    tab = _table(1)
    rec = Recorder()
    _, seq, finish = _drive(tab, 5, eos_token_id=None, streamer=rec)
    assert torch.equal(seq, _free_run(tab, 5)) and finish.tolist() == [5, 5, 5]
    check_stream(rec, seq)
    _, mcfg = _tiny()
    with pytest.raises(ValueError):
        request.parse(dict(streamer=object()), mcfg)


# ---- routes and modes -------------------------------------------------------------------------------------------------------------------------------
class _Device(Exception):
    pass


def _routed(kw):
    """(route, greedy, the forwarded keyword names) of generate(ids, **kw), as tests/test_request_cpu.py takes them: the route bodies are sentinels."""
    cfg, mcfg = _tiny()
    m = DynamicLlavaLlamaForCausalLM(mcfg, with_vision_tower=False)
    m._check_ready = lambda *a, **k: None
    m._generate_sample = lambda inputs, images, greedy=False, **k: ("sample", bool(greedy), sorted(k))
    m._generate_on_cache = lambda inputs, images, **k: ("on_cache", True, sorted(k))

    def device(*a, **k):
        raise _Device()

    m._pooled_cache = device
    try:
        return m.generate(torch.tensor([[1, 5, -200, 9]]), image_features=torch.zeros(1, 4, cfg.hidden_size), max_new_tokens=2, **kw)
    except _Device:
        return ("device", None, None)


NINE = [[i + 1] for i in range(9)]
ROUTES = [
    (dict(stop_sequences=[[3, 4]]), "device", None, None),
    (dict(stop_sequences=[[1] * 8] * 8, streamer=Recorder()), "device", None, None),
    (dict(stopping_criteria=[Keywords([3, 4])], do_sample=True, seed=3), "device", None, None),
    (dict(stop_sequences=None, stopping_criteria=[]), "device", None, None),
    (dict(streamer=Recorder()), "device", None, None),
    (dict(stop_sequences=NINE), "sample", True, ["stop_sequences"]),
    (dict(stop_sequences=[[1] * 9], sync_every=2), "sample", True, ["stop_sequences"]),
    (dict(stop_sequences=NINE, do_sample=True, seed=1), "sample", False, ["do_sample", "seed", "stop_sequences"]),
    (dict(stopping_criteria=[len]), "sample", True, ["stopping_criteria"]),
    (dict(stopping_criteria=[len], do_sample=True, seed=1, streamer=Recorder()), "sample", False, ["do_sample", "seed", "stopping_criteria", "streamer"]),
    (dict(stop_sequences=[[3]], past_key_values=object()), "on_cache", True, ["past_key_values", "stop_sequences"]),
    (dict(stop_sequences=[[3]], do_sample=True), "sample", False, ["do_sample", "stop_sequences"]),
]


@pytest.mark.parametrize("kw,route,greedy,names", ROUTES, ids=[",".join(sorted(r[0])) + f"-{i}" for i, r in enumerate(ROUTES)])
def test_routing_table_rows(kw, route, greedy, names):
    want = None if names is None else sorted(names + ["image_features", "max_new_tokens"])
    assert _routed(kw) == (route, greedy, want)


def test_bad_values_raise_before_any_launch_and_score_refuses():
    for kw in (dict(stop_sequences=[[V]]), dict(stop_sequences=[[]]), dict(stop_sequences=[[1.5]]), dict(stopping_criteria=[3]), dict(streamer=3)):
        for more in (dict(), dict(do_sample=True, seed=1), dict(do_sample=True), dict(eos_token_id=[2, 3, 4, 5])):
            with pytest.raises(ValueError):
                _routed(dict(kw, **more))
    _, mcfg = _tiny()
    labels = torch.zeros((1, 2), dtype=torch.long)
    for kw in (dict(stop_sequences=[[3]]), dict(stopping_criteria=[Keywords([3])]), dict(stopping_criteria=[len])):
        with pytest.raises(ValueError):
            request.parse(dict(kw, _score_labels=labels, max_new_tokens=2, eos_token_id=None), mcfg)
    assert request.parse(dict(_score_labels=labels, stop_sequences=[], max_new_tokens=2, eos_token_id=None), mcfg).forced is labels


def test_step_mode_of_a_request_without_the_keywords():
    _, mcfg = _tiny()
    base = dict(max_new_tokens=4, min_new_tokens=9, pad_token_id=3, eos_token_id=7)
    plain = request.parse(dict(base), mcfg)
    assert StepMode.of(plain, 4) == StepMode(eos=7, pad=3, min_new=4) and StepMode().stop is False
    for kw in (dict(stop_sequences=None), dict(stop_sequences=[]), dict(stopping_criteria=[]), dict(streamer=Recorder())):
        req = request.parse(dict(base, **kw), mcfg)
        assert StepMode.of(req, 4) == StepMode.of(plain, 4) and req.route == "device" and req.stops == () and req.criteria == ()
    on = request.parse(dict(base, stop_sequences=[[5, 6]]), mcfg)
    assert StepMode.of(on, 4) == StepMode(eos=7, pad=3, min_new=4, stop=True) != StepMode.of(plain, 4)
    assert StepMode.of(on, 4) == StepMode.of(request.parse(dict(base, stop_sequences=[[1], [2, 3]]), mcfg), 4)  # the list is device data: one mode, one graph
    assert on.can_finish and request.parse(dict(max_new_tokens=2, eos_token_id=None), mcfg).can_finish is False
    cfg = fx.tiny_config()
    m = DynamicLlavaLlamaForCausalLM(DynamicLlavaConfig.from_namespace(cfg), with_vision_tower=False)
    assert m.knobs()["device_stop_sequences"] is True


def test_one_token_stop_finishes_where_transformers_eos_criterion_does():
    from transformers.generation.stopping_criteria import EosTokenCriteria

    g = torch.Generator().manual_seed(9)
    out = torch.randint(0, 6, (32, 10), generator=g)
    crit = EosTokenCriteria(eos_token_id=4)
    want = torch.full((32,), 10, dtype=torch.int64)
    for t in range(10):  # HF: a row is done at the first step whose newest token makes the criterion true
        done = crit(out[:, : t + 1], None)
        want = torch.where(done & (want == 10), torch.full_like(want, t), want)
    assert torch.equal(stopping.finish_columns(out, (), ((4,),)), want) and torch.equal(stopping.finish_columns(out, (4,), ()), want)
    assert 0 < int((want < 10).sum()) and int(want.min()) == 0


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_entry():
    """include/dynllava.h declares dl_decode_stop with the caps and the table, hip_ops binds it, the library exports it and refuses bad arguments before any launch
    (the pointers are never dereferenced)."""
    from ctypes import c_int, c_void_p

    from dynamic_llava_amd import hip_ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dynllava.h")).read(), flags=re.S)
    want = (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p])
    m = re.search(r"\bdl_decode_stop\s*\(([^)]*)\)", hdr)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(want[1]) and hip_ops.SIGNATURES["dl_decode_stop"] == want
    assert int(re.search(r"#define\s+DL_STOP_MAX_SEQS\s+(\d+)", hdr).group(1)) == stopping.MAX_STOPS
    assert int(re.search(r"#define\s+DL_STOP_MAX_LEN\s+(\d+)", hdr).group(1)) == stopping.MAX_STOP_LEN
    assert hip_ops.STOP_TABLE_WORDS == 8 + stopping.MAX_STOPS * (1 + stopping.MAX_STOP_LEN)
    lib = hip_ops.load_library()
    assert lib.dl_version() == 4 and hip_ops.ABI_VERSION == 4
    p = ctypes.c_void_p(16)

    def call(out=p, cap=4, B=1, step=p, fin=p, tab=p):
        return lib.dl_decode_stop(out, cap, B, step, fin, tab, None)

    for kw in (dict(out=None), dict(step=None), dict(fin=None), dict(tab=None), dict(B=0), dict(B=-3), dict(cap=0)):
        assert call(**kw) == -1 and b"dl_decode_stop" in lib.dl_last_error(), kw
