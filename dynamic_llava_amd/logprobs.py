"""The log-probability rule of dl_decode_logprobs (csrc/logprobs.hip), written once in plain torch / Python integers.

Same role as scoring.py has for dl_decode_score: this file is the contract the kernel is tested against; it runs on the CPU.  The quantity is what
the reference's answer-producing drivers derive from `output_scores` (llava/eval/model_vqa_science_for_ppl.py:116-140: softmax, log, max per step -- the
log-probability of the token just emitted), and what OpenAI / vLLM call `logprobs` + `top_logprobs`.

The distribution is always that of the model's own step logits -- the raw logits generate(output_logits=True) reports, the quantity score() uses -- taken
before logits processors, before the EOS ban of min_new_tokens and before temperature / top-k / top-p.

One step of one row, `reference_row(logits_row, token, n)`:

1. m, the masses, M and lse are exactly scoring.masses / scoring.lse_of (steps 1-5 of scoring.py).
2. logprob(v) = -((m - x_v) + lse): two fp32 operations in this order, then an exact negation.  For any token it is therefore the bit-exact negative of
   scoring.reference_step(row, v)'s nll.  A token outside [0, V) reports 0.0.
3. The top-n list is the first n entries of the vocabulary ordered by (logit descending, index ascending); entry 0 is the greedy token.  -inf logits take
   part in that order and report -inf.

The row needs one finite maximum (no NaN, no +inf), V <= 65536 (sampling.MAX_VOCAB), 0 <= n <= MAX_TOP_LOGPROBS and n <= V."""
from __future__ import annotations

import torch

from .sampling import MAX_VOCAB
from .scoring import lse_of, masses

MAX_TOP_LOGPROBS = 8  # include/dynllava.h DL_MAX_TOP_LOGPROBS


def validate(kwargs, vocab_size):
    """generate()'s check of output_logprobs / top_logprobs, before any launch -> -1 (not asked for) or n, the number of alternatives per step."""
    want = kwargs.get("output_logprobs", False)
    n = kwargs.get("top_logprobs", 0)
    if not isinstance(want, bool):
        raise ValueError("output_logprobs must be a bool")
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MAX_TOP_LOGPROBS:
        raise ValueError(f"top_logprobs must be an int in 0..{MAX_TOP_LOGPROBS} (got {n!r})")
    if n > 0 and not want:
        raise ValueError("top_logprobs needs output_logprobs=True")
    if not want:
        return -1
    if not kwargs.get("return_dict_in_generate"):
        raise ValueError("output_logprobs needs return_dict_in_generate=True")
    if kwargs.get("_score_labels") is not None:
        raise ValueError("score() reports the labels' nll itself: it takes neither output_logprobs nor top_logprobs")
    if int(vocab_size) > MAX_VOCAB:
        raise ValueError(f"output_logprobs takes vocabularies of up to {MAX_VOCAB} entries (dl_decode_logprobs' 64-bit fixed-point masses)")
    if n > int(vocab_size):
        raise ValueError(f"top_logprobs={n} exceeds the vocabulary ({int(vocab_size)} entries)")
    return n


def top_order(logits_row, n):
    """Step 3: the first n indices of the row in (logit descending, index ascending) order -> int64 [n]."""
    x = logits_row.detach().float().cpu()
    assert 0 <= n <= x.shape[0]
    return torch.argsort(-x, stable=True)[:n]  # (the negation is exact; a stable ascending sort keeps equal logits in index order)


def reference_row_tokens(logits_row, tokens, n=0):
    """One step of one row asked about several tokens (the masses are summed once) -> (logprobs fp32 [len(tokens)], top_logprobs fp32 [n], top_ids int64 [n])."""
    x = logits_row.detach().float().cpu()
    m, _, mass = masses(x)
    lse = lse_of(int(mass.sum()))
    lp_of = lambda xv: -((m - xv) + lse)
    tokens = torch.as_tensor(tokens, dtype=torch.int64).reshape(-1)
    inside = (tokens >= 0) & (tokens < x.shape[0])
    lp = torch.where(inside, lp_of(x[tokens.clamp(0, x.shape[0] - 1)]), torch.zeros((), dtype=torch.float32))
    ids = top_order(x, n)
    return lp, lp_of(x[ids]), ids


def reference_row(logits_row, token, n=0):
    """One step of one row -> (logprob fp32 scalar tensor, top_logprobs fp32 [n], top_ids int64 [n])."""
    lp, top_lp, ids = reference_row_tokens(logits_row, [int(token)], n)
    return lp[0], top_lp, ids


def reference_rows(logits, tokens, n=0):
    """A batch [B, V] with the picked tokens [B] -> (logprobs fp32 [B], top_logprobs fp32 [B, n], top_ids int64 [B, n]), on the CPU."""
    B = logits.shape[0]
    lp, top_lp, top_ids = torch.zeros(B, dtype=torch.float32), torch.zeros((B, n), dtype=torch.float32), torch.zeros((B, n), dtype=torch.int64)
    for b in range(B):
        lp[b], top_lp[b], top_ids[b] = reference_row(logits[b], int(tokens[b]), n)
    return lp, top_lp, top_ids


def mask_after_eos(sequences, eos_ids, logprobs, top_logprobs=None, top_ids=None):
    """In place: the columns after a row's first EOS -- where `sequences` holds pad -- report 0.0 / -1; the EOS token's own entry stays.  The columns are
    found by position, not by value: pad may be an EOS id.  sequences [B, T]; logprobs [B, T]; top_logprobs / top_ids [B, T, n] or None."""
    if not len(eos_ids) or sequences.shape[1] == 0:
        return logprobs, top_logprobs, top_ids
    hit = torch.zeros_like(sequences, dtype=torch.bool)
    for e in eos_ids:
        hit |= sequences == int(e)
    after = (hit.long().cumsum(dim=1) - hit.long()) > 0  # an EOS strictly before this column
    after = after.to(logprobs.device)
    logprobs.masked_fill_(after, 0.0)
    if top_logprobs is not None:
        top_logprobs.masked_fill_(after[..., None], 0.0)
    if top_ids is not None:
        top_ids.masked_fill_(after[..., None], -1)
    return logprobs, top_logprobs, top_ids


def mask_after_columns(finish, logprobs, top_logprobs=None, top_ids=None):
    """mask_after_eos for rows that can also finish on a stop sequence or a stopping criterion: in place, the columns BEHIND column finish[b] of row b report
    0.0 / -1; the finishing token's own entry stays.  finish: int64 [B] (stopping.finish_columns; T or more where the row never finishes)."""
    after = torch.arange(logprobs.shape[1], dtype=torch.int64, device=logprobs.device)[None, :] > finish.to(logprobs.device)[:, None]
    logprobs.masked_fill_(after, 0.0)
    if top_logprobs is not None:
        top_logprobs.masked_fill_(after[..., None], 0.0)
    if top_ids is not None:
        top_ids.masked_fill_(after[..., None], -1)
    return logprobs, top_logprobs, top_ids


def host_result(step_logits, sequences, eos_ids, n, finish=None):
    """The host routes of generate(): the rule on every step's raw fp32 logits (a sequence of [B, V], one per column of `sequences`), masked ->
    the result keys on sequences' device.  finish: the rows' finish columns when they can finish on more than EOS (mask_after_columns), else None."""
    B, T = sequences.shape
    lp, top_lp, top_ids = torch.zeros((B, T), dtype=torch.float32), torch.zeros((B, T, n), dtype=torch.float32), torch.full((B, T, n), -1, dtype=torch.int64)
    seq = sequences.detach().cpu()
    for t in range(T):
        lp[:, t], top_lp[:, t], top_ids[:, t] = reference_rows(step_logits[t], seq[:, t], n)
    if finish is None:
        mask_after_eos(seq, eos_ids, lp, top_lp, top_ids)
    else:
        mask_after_columns(finish.cpu(), lp, top_lp, top_ids)
    dev = sequences.device
    out = {"logprobs": lp.to(dev)}
    if n > 0:
        out.update(top_logprobs=top_lp.to(dev), top_logprob_ids=top_ids.to(dev))
    return out
