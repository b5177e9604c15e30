"""CPU: the logits-processor rule (dynamic_llava_amd/logits_rules.py) against the installed transformers processors, chained in HF's order, on a
table of rows, histories and settings; mutants of the rule that the table must tell apart; validation and routing; the C ABI entry."""
import ctypes
import os
import re

import pytest
import torch

from dynamic_llava_amd import logits_rules as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")
EOS = 2
PENALTIES = (0.5, 0.7, 1.0, 1.3, 2.0)
NGRAMS = (0, 1, 2, 3, 5)
ALPHA = (5, 17, 40, 41, 99)  # the histories' alphabet: a handful of ids, so tokens and n-grams repeat


def _rows(V):
    """name -> fp32 [V]: bf16-representable random logits, and the same with -inf, both zeros, huge and tiny magnitudes at ids the histories use."""
    g = torch.Generator().manual_seed(20261019 + V)
    x = (torch.randn(V, generator=g) * 8).bfloat16().float()
    hard = x.clone()
    hard[5], hard[17], hard[40], hard[41], hard[99] = NEG, -0.0, 0.0, 3.0e38, -3.0e38
    hard[3], hard[7], hard[21], hard[23] = 1.0e-38, -1.0e-38, NEG, 2.5
    return {"randn": x, "hard": hard}


def _histories(n, V):
    """Histories of length 0, 1, n - 2, n - 1, n and 40 over ALPHA, with planted repeats; the 40-token one ends in the first tokens of an n-gram it holds."""
    g = torch.Generator().manual_seed(7 + n)
    out = []
    for s in sorted({0, 1, max(n - 2, 0), max(n - 1, 0), n, 40}):
        h = [ALPHA[i] for i in torch.randint(0, len(ALPHA), (s,), generator=g).tolist()]
        if s == 40 and n >= 2:
            block = [ALPHA[(i * 2) % 5] for i in range(n - 1)] + [V - 1]  # an n-gram ending in the vocabulary's last id ...
            h[3 : 3 + n] = block
            h[20 : 20 + n] = block[:-1] + [7]  # ... the same prefix with another ending ...
            h[40 - (n - 1) :] = block[:-1]  # ... and the prefix again as the tail: both endings are banned
        if s >= 3:
            h[0] = h[2]  # a token that occurs more than once
        out.append(h)
    return out


def _words(h):
    """One-, two- and three-token words; some match the tail of `h`, some do not; [EOS] is dropped by the parser."""
    w = [[3], [EOS], [ALPHA[0], 11], [ALPHA[1], ALPHA[0], 13], [9, 9, 15]]
    if len(h) >= 1:
        w += [[h[-1], 21], [h[-1] + 1, 22]]
    if len(h) >= 2:
        w += [[h[-2], h[-1], 23], [h[-1], h[-2] + 1, 24]]
    return w


def _table():
    for V in (320, 1003):
        for name, x in _rows(V).items():
            for n in NGRAMS:
                for h in _histories(n, V):
                    for p in PENALTIES:
                        yield V, name, x, h, p, n, _words(h)


def _hf(x, h, p, n, words):
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    ids = torch.tensor([h], dtype=torch.long)
    z = x[None].clone()
    z = RepetitionPenaltyLogitsProcessor(penalty=float(p))(ids, z)
    if n > 0:
        z = NoRepeatNGramLogitsProcessor(n)(ids, z)
    if words:
        z = NoBadWordsLogitsProcessor(words, eos_token_id=[EOS])(ids, z)
    return z[0]


def _restated(x, g, p, n, words, mutant=None):
    """The rule once more, with switches for the mutants below (mutant None: the rule itself, which the test holds to logits_rules first)."""
    y, V, s = x.clone(), x.shape[0], len(g)
    pt = torch.tensor(p, dtype=torch.float32)
    pen = lambda v: v * pt if (v < 0 and mutant != "always_divide") else v / pt
    bans = set()
    if n >= 1 and s + 1 >= n:
        k = n if mutant == "match_n_tokens" else n - 1
        pre = g[s - k :] if k else []
        last = s - n - (1 if mutant == "scan_stops_early" else 0)
        bans |= {g[i + k] for i in range(0, last + 1) if g[i : i + k] == pre and i + k < s}
    for w in words:
        if len(w) == 1 or mutant == "word_without_prefix" or (len(w) <= s and g[s - (len(w) - 1) :] == w[:-1]):
            bans.add(w[-1])
    if mutant == "penalty_after_bans":
        for t in bans:
            y[t] = NEG
    if p != 1.0:
        for t in (g if mutant == "per_occurrence" else sorted(set(g))):
            src = y[t] if mutant == "per_occurrence" else x[t]
            y[t] = pen(src.bfloat16().float()).bfloat16().float() if mutant == "bf16_arithmetic" else pen(src)
    if mutant != "penalty_after_bans":
        for t in bans:
            y[t] = NEG
    return y


def test_rule_equals_the_transformers_processors():
    n_cases = 0
    for V, name, x, h, p, n, words in _table():
        rules = lr.normalize(dict(repetition_penalty=p, no_repeat_ngram_size=n, bad_words_ids=words), V, [EOS])
        assert [EOS] not in [list(w) for w in rules.bad_words] and len(rules.bad_words) == len(words) - 1
        got = lr.process_row(x, h, rules.repetition_penalty, rules.no_repeat_ngram_size, rules.bad_words)
        assert got.dtype == torch.float32 and torch.equal(got, _hf(x, h, p, n, words)), (V, name, h, p, n)
        n_cases += 1
    assert n_cases >= 2 * 2 * 5 * 5 * 4


def test_special_values_keep_their_bits():
    """-0.0 and +0.0 are divided (and keep their sign), -inf stays -inf, a token that occurs three times is penalised once, bans win."""
    x = torch.tensor([-0.0, 0.0, NEG, -3.0, 3.0, 1.5, -1.5, 8.0])
    y = lr.process_row(x, [0, 1, 2, 3, 3, 3, 4, 5], 2.0, 0, [[5], [4, 5, 6], [0, 7]])
    assert y.view(torch.int32).tolist() == torch.tensor([-0.0, 0.0, NEG, -6.0, 1.5, NEG, NEG, 8.0]).view(torch.int32).tolist()
    # an id outside [0, V) in the history is never an index: the row is otherwise what it would be
    assert torch.equal(lr.process_row(x, [3, 99, -4, 4], 2.0, 1, ()), torch.tensor([-0.0, 0.0, NEG, NEG, NEG, 1.5, -1.5, 8.0]))
    assert torch.equal(lr.process_row(x.bfloat16(), [], 1.3, 3, ()), x), "an empty history edits nothing"


@pytest.mark.parametrize("mutant", ["per_occurrence", "always_divide", "bf16_arithmetic", "match_n_tokens", "scan_stops_early", "word_without_prefix", "penalty_after_bans"])
def test_the_table_tells_each_mutant_from_the_rule(mutant):
    differs = 0
    for V, name, x, h, p, n, words in _table():
        words = [w for w in words if w != [EOS]]
        want = lr.process_row(x, h, p, n, words)
        assert torch.equal(_restated(x, h, p, n, words).view(torch.int32), want.view(torch.int32)), "the restatement is the rule"
        differs += int(not torch.equal(_restated(x, h, p, n, words, mutant), want))
    assert differs > 0, mutant


def test_validation():
    V = 100
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.3), dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
                dict(repetition_penalty="1.3"), dict(repetition_penalty=True),
                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size="3"), dict(no_repeat_ngram_size=True),
                dict(bad_words_ids=[[]]), dict(bad_words_ids=[5]), dict(bad_words_ids=[[V]]), dict(bad_words_ids=[[-1]]), dict(bad_words_ids=[[1, 2.5]]),
                dict(bad_words_ids="ab"), dict(bad_words_ids=[[1], [2, V + 3]])):
        with pytest.raises(ValueError):
            lr.normalize(bad, V)


def test_neutral_values_are_off_and_over_cap_requests_take_the_host_route():
    V = 1000
    for off in ({}, dict(repetition_penalty=None, no_repeat_ngram_size=None, bad_words_ids=None), dict(repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=[]),
                dict(repetition_penalty=1, bad_words_ids=[[EOS]])):
        r = lr.normalize(off, V, [EOS])
        assert not r.on and r.device_route and r == lr.Rules()
    for on in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=lr.MAX_NGRAM), dict(bad_words_ids=[[1]] * lr.MAX_BAD_WORDS), dict(bad_words_ids=[list(range(lr.MAX_BAD_WORD_LEN))]),
               dict(bad_words_ids=[[EOS, 3]])):
        r = lr.normalize(on, V, [EOS])
        assert r.on and r.device_route, on
    for over in (dict(no_repeat_ngram_size=lr.MAX_NGRAM + 1), dict(bad_words_ids=[[1]] * (lr.MAX_BAD_WORDS + 1)), dict(bad_words_ids=[list(range(lr.MAX_BAD_WORD_LEN + 1))])):
        r = lr.normalize(over, V, [EOS])
        assert r.on and not r.device_route, over
    assert (lr.MAX_NGRAM, lr.MAX_BAD_WORDS, lr.MAX_BAD_WORD_LEN) == (16, 64, 8)


def test_process_on_a_batch_is_process_row_per_row():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(3, 320, generator=g) * 8).bfloat16()
    hist = torch.tensor([[5, 17, 5, 17], [40, 40, 40, 40], [99, 5, 17, 41]])
    words = [[3], [17, 5], [5, 17, 6]]
    got = lr.process(x, hist, 1.3, 2, words)
    assert got.dtype == torch.float32 and got.shape == x.shape
    for b in range(3):
        assert torch.equal(got[b].view(torch.int32), lr.process_row(x[b], hist[b], 1.3, 2, words).view(torch.int32))
    assert torch.equal(lr.process(x, [[5], [5, 17, 5], []], 1.3, 2, words)[1], lr.process_row(x[1], [5, 17, 5], 1.3, 2, words)), "ragged histories as lists"
    assert torch.equal(lr.process(x, torch.empty((3, 0), dtype=torch.long), 2.0, 1, ()), x.float())
    assert torch.equal(lr.Rules(1.3, 2, tuple(map(tuple, words))).apply(x, hist), got)


def test_header_binding_and_exports():
    """include/dynllava.h declares dl_logits_process and its parameter block, hip_ops' prototype table matches, the library exports it, the ABI version is unchanged."""
    from ctypes import c_int, c_int64, c_void_p

    from dynamic_llava_amd import hip_ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dynllava.h")).read(), flags=re.S)
    want = (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p])
    m = re.search(r"\bdl_logits_process\s*\(([^)]*)\)", hdr)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(want[1])
    assert hip_ops.SIGNATURES["dl_logits_process"] == want
    body = re.search(r"typedef struct dl_logits_params \{(.*?)\} dl_logits_params;", hdr, flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["float repetition_penalty", "int32_t no_repeat_ngram", "int32_t n_bad_words", "int32_t reserved[5]"]
    words = hip_ops.logits_params_words(1.3, 3, 2)
    assert words.dtype == torch.int32 and words.numel() * 4 == 32 and words.tolist()[1:] == [3, 2, 0, 0, 0, 0, 0]
    assert words[:1].view(torch.float32).item() == pytest.approx(1.3)
    for name, val in (("DL_LOGITS_MAX_NGRAM", lr.MAX_NGRAM), ("DL_LOGITS_MAX_BAD_WORDS", lr.MAX_BAD_WORDS), ("DL_LOGITS_MAX_BAD_WORD_LEN", lr.MAX_BAD_WORD_LEN)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1)) == val
    tab = hip_ops.bad_words_table([[7], [1, 2, 3]], "cpu")
    assert tab.dtype == torch.int32 and tab.shape == (lr.MAX_BAD_WORDS, 1 + lr.MAX_BAD_WORD_LEN)
    assert tab[0].tolist() == [1, 7] + [0] * 7 and tab[1].tolist() == [3, 1, 2, 3] + [0] * 5 and int(tab[2:].abs().sum()) == 0
    with pytest.raises(ValueError):
        hip_ops.bad_words_table([list(range(lr.MAX_BAD_WORD_LEN + 1))], "cpu")
    lib = hip_ops.load_library()
    assert lib.dl_version() == 4 and hip_ops.ABI_VERSION == 4
    assert hasattr(lib, "dl_logits_process")
    # argument checks run before any launch (no device needed): the pointers are never dereferenced
    p = ctypes.c_void_p(16)
    call = lambda dtype=hip_ops.DL_BF16, V=320, B=1, out=p, prm=p: lib.dl_logits_process(p, dtype, V, V, B, out, None, 0, None, prm, None, None)
    assert call(dtype=7) == -1 and call(V=0) == -1 and call(B=0) == -1 and call(out=None) == -1
    assert call(prm=None) == -1 and b"parameter block" in lib.dl_last_error()


def test_generate_validates_before_any_launch_and_reports_the_knob():
    """On a box without a GPU nothing can be launched: a ValueError (not a HipOpsError) shows the keywords were checked first."""
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM
    from oracle import fixtures as fx

    cfg = fx.tiny_config()
    m = DynamicLlavaLlamaForCausalLM(DynamicLlavaConfig.from_namespace(cfg), with_vision_tower=False)
    m._check_ready = lambda: None
    assert m.knobs()["device_logits_processors"] is True
    ids = torch.tensor([[1, 5, -200, 9]])
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-2), dict(no_repeat_ngram_size=1.5),
                dict(bad_words_ids=[[]]), dict(bad_words_ids=[[cfg.vocab_size]])):
        with pytest.raises(ValueError):
            m.generate(ids, max_new_tokens=2, **bad)
        with pytest.raises(ValueError):
            m.generate(ids, max_new_tokens=2, do_sample=True, seed=1, **bad)
    with pytest.raises(ValueError):  # score()'s labels together with processors
        m.generate(ids, max_new_tokens=2, repetition_penalty=1.3, _score_labels=torch.zeros((1, 2), dtype=torch.long))
