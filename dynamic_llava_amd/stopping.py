"""The stopping rule of generate(stop_sequences= / stopping_criteria=) and of dl_decode_stop (csrc/stop.hip), written once in plain torch / Python, and the
token feed of generate(streamer=).

Same role as logits_rules.py and logprobs.py: this file is the contract the kernel is tested against; it runs on the CPU and is what the host routes of
generate() apply to the emitted tokens themselves.

A stop sequence is a non-empty tuple of token ids.  A row finishes at the first column c of its generated tokens at which out[b, c] is in the EOS set, or
out[b, c - n + 1 : c + 1] equals a stop sequence of length n <= c + 1.  This is the token-tail rule of the reference's KeywordsStoppingCriteria
(llava/mm_utils.py:257-267: `output_ids[0, -len(keyword):] == keyword`), per row instead of for row 0 only, on the tokens generated in this call: the
reference generates from `inputs_embeds`, so the prompt is never part of what a criterion sees, and a match never reaches across column 0.  The criterion's
second check (mm_utils.py:268-273), a substring search in the DECODED text of the tail, needs a tokenizer and is not built: a keyword that only appears
across a token boundary of another tokenisation does not stop a row here.

min_new_tokens does not hold back a stop-sequence match (HF's stopping criteria never look at it; only the EOS logit ban honours it).  The matched tokens
stay in `sequences`, as an EOS token does; the columns behind them hold pad_token_id.

The device route takes up to MAX_STOPS sequences of up to MAX_STOP_LEN tokens (dl_decode_stop compares them with the 64 lanes of one wave); a request past
either cap, or one that carries any other stopping criterion (a callable), runs the plain loop over forward() with this file's rule."""
from __future__ import annotations

import numbers

import torch

# what the device route takes (mirrored in include/dynllava.h: DL_STOP_MAX_SEQS / DL_STOP_MAX_LEN)
MAX_STOPS = 8
MAX_STOP_LEN = 8


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _sequence(s, vocab_size, what):
    """One stop sequence (a list / tuple of ints or a 1-D integer tensor) -> a tuple of ints, validated."""
    if torch.is_tensor(s):
        if s.dim() != 1 or s.is_floating_point() or s.is_complex() or s.dtype == torch.bool:
            raise ValueError(f"{what}: a stop sequence must be a 1-D integer tensor (got {s.dtype}, {tuple(s.shape)})")
        s = s.tolist()
    elif not isinstance(s, (list, tuple)):
        raise ValueError(f"{what} must hold non-empty lists of token ids or 1-D integer tensors (got the entry {s!r})")
    if len(s) == 0:
        raise ValueError(f"{what}: an empty stop sequence")
    if not all(_is_int(t) for t in s):
        raise ValueError(f"{what}: every id must be an int (got the entry {s!r})")
    if not all(0 <= int(t) < int(vocab_size) for t in s):
        raise ValueError(f"{what}: every id must be in [0, {int(vocab_size)}) (got the entry {s!r})")
    return tuple(int(t) for t in s)


def _criteria(kwargs):
    c = kwargs.get("stopping_criteria")
    if c is None:
        return []
    if not isinstance(c, (list, tuple)):  # (HF's StoppingCriteriaList is a list)
        raise ValueError(f"stopping_criteria must be a list of criteria (got {type(c).__name__})")
    return list(c)


def normalize(kwargs, vocab_size):
    """generate()'s kwargs -> the stop sequences, a tuple of tuples of ints: those of stop_sequences=, then those of every item of stopping_criteria= that carries
    a `keyword_ids` attribute (a list of 1-D tensors: the reference's KeywordsStoppingCriteria), in order, duplicates kept.  Only the token-tail rule of that
    criterion is reproduced; its decoded-text substring search needs a tokenizer and is not built.  None or empty input -> ().  Raises ValueError for an id
    outside [0, vocab_size), an empty sequence and a non-integer entry."""
    out = []
    ss = kwargs.get("stop_sequences")
    if ss is not None:
        if not isinstance(ss, (list, tuple)):
            raise ValueError(f"stop_sequences must be a list of non-empty lists of token ids or 1-D integer tensors (got {type(ss).__name__})")
        out += [_sequence(s, vocab_size, "stop_sequences") for s in ss]
    for c in _criteria(kwargs):
        ids = getattr(c, "keyword_ids", None)
        if ids is not None:
            if not isinstance(ids, (list, tuple)):
                raise ValueError(f"stopping_criteria: keyword_ids must be a list of 1-D tensors (got {type(ids).__name__})")
            out += [_sequence(s, vocab_size, "stopping_criteria.keyword_ids") for s in ids]
    return tuple(out)


def host_criteria(kwargs):
    """The items of stopping_criteria= that are not keyword criteria: callables (ids [B, t], scores) -> bool | BoolTensor [B], which only the plain host loop can
    serve (once per step, on the tokens generated in this call).  Raises ValueError for an item that is neither."""
    out = []
    for c in _criteria(kwargs):
        if getattr(c, "keyword_ids", None) is not None:
            continue
        if not callable(c):
            raise ValueError(f"stopping_criteria: an item is neither a keyword criterion nor callable ({c!r})")
        out.append(c)
    return tuple(out)


def device_route(stops) -> bool:
    """True when dl_decode_stop takes the list (inside the captured graphs)."""
    return len(stops) <= MAX_STOPS and all(len(s) <= MAX_STOP_LEN for s in stops)


def tail_matches(history, stops) -> bool:
    """One row: do its tokens so far (a sequence of ints) end in one of the stop sequences?  A sequence longer than the history never matches."""
    g = [int(t) for t in history]
    return any(len(s) <= len(g) and g[len(g) - len(s):] == [int(t) for t in s] for s in stops)


def finish_columns(out, eos, stops):
    """out: int64 [B, T], the generated tokens -> int64 [B] on out's device: the first column at which row b finishes (the module docstring's rule), T where it
    never does.  Found by value from column 0 on: what lies behind a row's finish (pad) is never consulted for that row."""
    B, T = out.shape
    hit = torch.zeros((B, T), dtype=torch.bool, device=out.device)
    for e in eos or ():
        hit |= out == int(e)
    for s in stops or ():
        n = len(s)
        if n > T:
            continue
        m = torch.ones((B, T - n + 1), dtype=torch.bool, device=out.device)
        for j, t in enumerate(s):  # m[:, i]: the window that starts at column i equals s; it ends -- the row finishes -- at column i + n - 1
            m &= out[:, j : j + T - n + 1] == int(t)
        hit[:, n - 1 :] |= m
    cols = torch.arange(T, dtype=torch.int64, device=out.device).expand(B, T)
    return torch.where(hit, cols, torch.full_like(cols, T)).min(dim=1).values if T > 0 else torch.zeros(B, dtype=torch.int64, device=out.device)


def reference_flags(out_ids, step, finished, table):
    """What dl_decode_stop leaves in `finished` (int32 [B]), on the CPU: a row that is not finished yet, whose t = min(step[b], out_cap) tokens out_ids[b, :t]
    end in one of the table's sequences, is set to 1; nothing else changes.  table: the words of dl_stop_table (include/dynllava.h; hip_ops.stop_table_words) --
    n_stops, 7 words nobody reads, then MAX_STOPS rows of a length and MAX_STOP_LEN ids; rows past n_stops and ids past a length are not read."""
    out_ids, step, table = out_ids.cpu(), step.cpu(), table.cpu()
    fin = finished.cpu().clone()
    cap = out_ids.shape[1]
    rows = table[8 : 8 + MAX_STOPS * (1 + MAX_STOP_LEN)].view(MAX_STOPS, 1 + MAX_STOP_LEN)
    stops = [tuple(int(v) for v in rows[i, 1 : 1 + int(rows[i, 0])]) for i in range(max(0, min(int(table[0]), MAX_STOPS))) if 1 <= int(rows[i, 0]) <= MAX_STOP_LEN]
    for b in range(out_ids.shape[0]):
        t = max(0, min(int(step[b]), cap))
        if int(fin[b]) == 0 and tail_matches(out_ids[b, :t].tolist(), stops):
            fin[b] = 1
    return fin


class Feed:
    """generate(streamer=)'s token feed: put(an empty int64 CPU tensor [B, 0]) first (what HF puts when driven by inputs_embeds: nothing of the prompt), then
    put(sequences[:, j].cpu()) for every column of the result, in order and once each, then end() once.  The device loop hands it whole chunks of columns
    as its observations arrive (`push`); a column behind the step at which every row has finished is never put, because generate() does not return it."""

    def __init__(self, streamer, B, eos, stops):
        self.streamer, self.eos, self.stops = streamer, tuple(eos), tuple(stops)
        self.seen = torch.zeros((B, 0), dtype=torch.int64)
        self.n_put = 0
        streamer.put(torch.zeros((B, 0), dtype=torch.int64))

    def push(self, cols):
        """cols: int64 CPU [B, k], the next k columns the device produced."""
        self.seen = torch.cat([self.seen, cols.to(torch.int64)], dim=1)
        width = min(self.seen.shape[1], int(finish_columns(self.seen, self.eos, self.stops).max()) + 1) if self.seen.shape[1] else 0
        self._put_upto(self.seen, width)

    def _put_upto(self, seq, width):
        for j in range(self.n_put, width):
            self.streamer.put(seq[:, j].clone())
        self.n_put = max(self.n_put, width)

    def finish(self, sequences):
        """sequences: what generate() returns, [B, W] -- the columns not yet put, then end()."""
        self._put_upto(sequences.detach().to("cpu", torch.int64), sequences.shape[1])
        self.streamer.end()
