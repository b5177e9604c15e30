"""The logits processors of a decode step (dl_logits_process, csrc/logits_proc.hip), written once in plain torch / Python.

Same role as sampling.py and scoring.py: this file is the contract the kernel is tested against; it runs on the CPU (and on any torch device) and
is what the host routes of generate() (_generate_sample, _generate_on_cache) apply to a step's logits themselves.

The three processors are HF's RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and NoBadWordsLogitsProcessor, chained in HF's order
(tests/test_logits_rules_cpu.py holds this file to the installed transformers bit for bit).  The reference generates from `inputs_embeds`
(dynamic_llava_llama.py:117-152), so HF's processors see an empty `input_ids` at the first step: the history of a row is the tokens generated in this
call only, never the prompt.

`process_row(logits_row, history, repetition_penalty, no_repeat_ngram_size, bad_words)` -> fp32 [V], with g = history (the row's tokens emitted so
far, in order) and s = len(g):

1. x_v = float32(logit_v); y = x.
2. Repetition penalty, p > 0, p != 1: for every distinct token t in g, y_t = x_t * p if x_t < 0, else x_t / p -- one fp32 operation on the original
   x_t (p rounded to fp32 first), the division correctly rounded.  A token that occurs several times is penalised once.  -0.0 and +0.0 take the
   division branch; -inf stays -inf.
3. No-repeat n-gram, n >= 1, when s + 1 >= n: with pre = the last n - 1 tokens of g (empty for n = 1), every i in [0, s - n] with
   g[i : i + n - 1] == pre gives y[g[i + n - 1]] = -inf.
4. Bad words: a word w of length 1 bans w[0] at every step; a longer word bans w[-1] when len(w) <= s and the last len(w) - 1 tokens of g
   equal w[:-1].  (len(w) <= s, not len(w) - 1 <= s: HF's SequenceBiasLogitsProcessor, which NoBadWordsLogitsProcessor is, skips a word "longer
   than the context", so a word whose prefix is the WHOLE history does not act yet.  The installed processors decide; the test pins it.)
   As in HF, a one-token word equal to an id of the request's EOS set is dropped when the request is parsed (`normalize`).
5. Bans win over the penalty.

An id in the history outside [0, V) (nothing generate() produces; the kernel's interface allows it) is never used as an index.  The EOS ban of
min_new_tokens, temperature, top-k and top-p come after this stage, inside the bookkeeping kernels: HF's order."""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Tuple

import torch

# what the device route takes (mirrored in include/dynllava.h: DL_LOGITS_MAX_*); a request beyond them runs the plain loop over forward() with this file's rule
MAX_NGRAM = 16
MAX_BAD_WORDS = 64
MAX_BAD_WORD_LEN = 8


@dataclass(frozen=True)
class Rules:
    """A request's processors, validated: repetition_penalty 1.0, no_repeat_ngram_size 0 and an empty bad_words mean "off"."""

    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    bad_words: Tuple[Tuple[int, ...], ...] = ()

    @property
    def on(self) -> bool:
        return self.repetition_penalty != 1.0 or self.no_repeat_ngram_size > 0 or len(self.bad_words) > 0

    @property
    def device_route(self) -> bool:
        """True when dl_logits_process takes the request (inside the captured graphs); False: the plain loop over forward() applies `process`."""
        return (self.no_repeat_ngram_size <= MAX_NGRAM and len(self.bad_words) <= MAX_BAD_WORDS
                and all(len(w) <= MAX_BAD_WORD_LEN for w in self.bad_words))

    def apply(self, logits, history):
        return process(logits, history, self.repetition_penalty, self.no_repeat_ngram_size, self.bad_words)


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def normalize(kwargs, vocab_size, eos_set=()) -> Rules:
    """generate()'s kwargs -> Rules.  None, repetition_penalty 1.0, no_repeat_ngram_size 0 and an empty bad_words_ids mean "off".  Raises ValueError
    for a repetition_penalty that is not a finite number > 0, a no_repeat_ngram_size that is not an int >= 0 and a bad_words_ids that is not a list
    of non-empty lists of ints in [0, vocab_size).  eos_set: the request's EOS ids -- a one-token bad word equal to one of them is dropped (HF)."""
    p = kwargs.get("repetition_penalty")
    if p is None:
        p = 1.0
    elif isinstance(p, bool) or not isinstance(p, numbers.Real) or not math.isfinite(float(p)) or not float(p) > 0.0:
        raise ValueError(f"repetition_penalty must be a finite float > 0 (got {p!r})")
    n = kwargs.get("no_repeat_ngram_size")
    if n is None:
        n = 0
    elif not _is_int(n) or int(n) < 0:
        raise ValueError(f"no_repeat_ngram_size must be an int >= 0 (got {n!r})")
    bw = kwargs.get("bad_words_ids")
    words = []
    if bw is not None:
        if not isinstance(bw, (list, tuple)):
            raise ValueError(f"bad_words_ids must be a list of non-empty lists of token ids (got {bw!r})")
        eos = {int(e) for e in (eos_set or ())}
        for w in bw:
            if not isinstance(w, (list, tuple)) or len(w) == 0:
                raise ValueError(f"bad_words_ids must be a list of non-empty lists of token ids (got the entry {w!r})")
            if not all(_is_int(t) and 0 <= int(t) < int(vocab_size) for t in w):
                raise ValueError(f"bad_words_ids: every id must be an int in [0, {int(vocab_size)}) (got the entry {w!r})")
            if len(w) == 1 and int(w[0]) in eos:
                continue  # HF: NoBadWordsLogitsProcessor filters [eos] out, so the row can still end
            words.append(tuple(int(t) for t in w))
    return Rules(float(p), int(n), tuple(words))


def process_row(logits_row, history, repetition_penalty=None, no_repeat_ngram_size=None, bad_words=()):
    """One row of one step -> fp32 [V] (a new tensor on logits_row's device).  history: the row's tokens emitted so far (a sequence or a 1-d tensor)."""
    assert logits_row.dim() == 1
    x = logits_row.float()
    y = x.clone()
    V = x.shape[0]
    g = [int(t) for t in (history.tolist() if torch.is_tensor(history) else history)]
    s = len(g)
    p = 1.0 if repetition_penalty is None else float(repetition_penalty)
    if p > 0.0 and p != 1.0:
        seen = sorted({t for t in g if 0 <= t < V})
        if seen:
            idx = torch.tensor(seen, dtype=torch.long, device=x.device)
            xt = x[idx]
            pt = torch.tensor(p, dtype=torch.float32, device=x.device)  # (a tensor, not a Python number: torch then divides instead of multiplying by 1 / p)
            y[idx] = torch.where(xt < 0, xt * pt, xt / pt)
    banned = set()
    n = 0 if no_repeat_ngram_size is None else int(no_repeat_ngram_size)
    if n >= 1 and s + 1 >= n:
        pre = g[s - (n - 1):] if n > 1 else []
        for i in range(0, s - n + 1):
            if g[i : i + n - 1] == pre:
                banned.add(g[i + n - 1])
    for w in bad_words or ():
        w = [int(t) for t in w]
        if len(w) == 1:
            banned.add(w[0])
        elif len(w) <= s and g[s - (len(w) - 1):] == w[:-1]:
            banned.add(w[-1])
    hit = sorted(t for t in banned if 0 <= t < V)
    if hit:
        y[torch.tensor(hit, dtype=torch.long, device=x.device)] = float("-inf")
    return y


def process(logits, history, repetition_penalty=None, no_repeat_ngram_size=None, bad_words=()):
    """A batch [B, V] with history [B, s] (a tensor, or a list of per-row sequences) -> fp32 [B, V]: process_row per row."""
    assert logits.dim() == 2
    rows = history.tolist() if torch.is_tensor(history) else list(history)
    assert len(rows) == logits.shape[0]
    return torch.stack([process_row(logits[b], rows[b], repetition_penalty, no_repeat_ngram_size, bad_words) for b in range(logits.shape[0])])
