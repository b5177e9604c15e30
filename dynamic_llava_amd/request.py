"""A generate() request, parsed by one function: the keywords resolved and validated before any device work (Request), the route it takes (route), and the one host loop both
host routes run (host_loop).  Pure Python on torch tensors.  (The host routes keep their **kwargs signatures: a request generate() hands to one is parsed there a second time.)"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

import torch

from . import constraints, guidance, logits_rules, logprobs, sampling, stopping
from .sampling import eos_ids  # the only resolver of eos_token_id; defined in that leaf module because sampling.device_route needs it too


def route(kwargs, rules, vocab_size, default_eos, constraint_on_host=False) -> str:
    """Which body of generate() serves the kwargs (the table is in DESIGN.md): "device" (the captured graphs), "host_sample" (_generate_sample), "host_greedy"
    (_generate_sample(greedy=True), without do_sample / sync_every) or "on_cache" (_generate_on_cache).  Past the device caps -- logits_rules.MAX_*, or more EOS
    ids than the step-closing kernels compare, or stopping.MAX_STOPS / MAX_STOP_LEN -- a request takes the plain loop over forward(), which applies the same rule on
    the host; so does a request with a stopping criterion that is a callable (stopping.host_criteria), which only the host can call.  constraint_on_host: the
    request's constraint is past constraints.MAX_STATES / MAX_EDGES, or is prefix_allowed_tokens_fn=, a callable like those criteria."""
    sample = bool(kwargs.get("do_sample", False))
    if sample and not sampling.device_route(kwargs, vocab_size, default_eos):
        return "host_sample"  # (KNOWN DEFECT: with past_key_values too -- _generate_sample never reads them, the dialogue is dropped without a word)
    if kwargs.get("past_key_values") is not None:
        return "on_cache"
    past_stop_caps = bool(stopping.host_criteria(kwargs)) or not stopping.device_route(stopping.normalize(kwargs, vocab_size))
    if (rules.on and not rules.device_route) or len(eos_ids(kwargs, default_eos)) > sampling.MAX_EOS_IDS or past_stop_caps or constraint_on_host:
        return "host_sample" if sample else "host_greedy"
    return "device"


def return_sequences(kwargs) -> int:
    """num_return_sequences, validated: n sampled answers per prompt.  None and 1 are the request without the keyword; n > 1 needs do_sample (HF's rule: greedy
    search returns one sequence), and is not built for score() nor on a caller's cache."""
    n = kwargs.get("num_return_sequences")
    if n is None:
        return 1
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"num_return_sequences must be an int >= 1 (got {n!r})")
    if n > 1 and not kwargs.get("do_sample", False):
        raise ValueError(f"num_return_sequences={n} needs do_sample=True: greedy search returns one sequence per prompt")
    if n > 1 and kwargs.get("_score_labels") is not None:
        raise ValueError("score() takes no num_return_sequences: a label sequence is scored once")
    if n > 1 and kwargs.get("past_key_values") is not None:
        raise NotImplementedError("num_return_sequences > 1 on generate(past_key_values=...) is not built: the fork follows a prefill")
    return n


@dataclass(frozen=True)
class Request:
    """Everything generate() and its host routes read from **kwargs."""
    eos: Tuple[int, ...]
    pad: int
    min_new: int  # as asked for; capped at max_new where it is used
    rules: logits_rules.Rules
    n_lp: int  # -1: no log-probabilities; else the number of alternatives per step
    sampled: Optional[tuple]  # (temperature, top_k, top_p, seed, row base) when the device sampler draws the tokens
    temperature: float  # the host loop's warpers (torch's RNG)
    top_k: int
    top_p: Optional[float]
    generator: Any
    want_dict: bool
    want_scores: bool  # `scores` in the result: the processed logits of every step
    want_logits: bool  # `logits` in the result: the raw ones (either makes the device loop read the step buffer after every step)
    sync_every: Optional[int]  # None: the model's decode_sync_every
    forced: Any  # score(): int64 [B, T] labels, validated there
    attention_mask: Any
    image_features: Any
    host_layout: bool
    route: str
    max_new_tokens: Optional[int]
    max_length: Optional[int]
    n_return: int = 1  # num_return_sequences: sampled answers per prompt, rows b * n .. b * n + n - 1 of every per-row result
    stops: Tuple[Tuple[int, ...], ...] = ()  # stop_sequences= and the keyword criteria of stopping_criteria= (stopping.normalize): a row finishes when its tokens end in one
    criteria: tuple = ()  # the other items of stopping_criteria=: callables, served by the host loop only
    streamer: Any = None  # put(tensor) / end(): receives the tokens as they come (stopping.Feed)
    constraint: Any = None  # constraint= / guided_choice= / allowed_token_ids=, compiled (constraints.Table): every row walks it, tokens without an edge are -inf
    allowed_fn: Any = None  # prefix_allowed_tokens_fn=: fn(batch_id, ids_1d) -> the allowed ids, served by the host loop only
    guidance: Optional[tuple] = None  # guidance_scale= (not None, not 1.0) with negative_prompt_ids= / negative_images=: (scale, cutoff or None) -- classifier-free guidance on paired rows (guidance.py)

    @property
    def can_finish(self) -> bool:
        """Some row may finish before max_new tokens: there is an EOS set, a stop sequence or a host criterion."""
        return bool(self.eos) or bool(self.stops) or bool(self.criteria)

    def max_new(self, lens) -> int:
        """The number of steps: max_new_tokens, or max_length - the longest prompt (HF's default: 20 steps)."""
        n = self.max_new_tokens
        if n is None:
            n = 20 if self.max_length is None else int(self.max_length) - max(lens)
        if n < 1:
            raise ValueError(f"max_new_tokens must be >= 1 (got {n})")
        return int(n)


def parse(kwargs, config, sync_every=None, batch=None) -> Request:
    """generate()'s **kwargs -> Request.  Every keyword is validated here, before any device work, in this order: the logits processors, score() with
    processors, the stop sequences and criteria, score() with those, the log-probabilities, what is not built (rejected, not silently ignored: DLL:117-152 forwards **kwargs to HF), num_return_sequences,
    the constraint (batch: the number of prompts, which a list of automata must match), the sampling parameters; the guidance keywords (guidance.validate) in front
    of them all."""
    V, eos = config.vocab_size, eos_ids(kwargs, config.eos_token_id)
    guide = guidance.validate(kwargs)
    if guide is not None and V > sampling.MAX_VOCAB:
        raise ValueError(f"guidance_scale takes vocabularies of up to {sampling.MAX_VOCAB} entries (the 64-bit fixed-point masses of its log-probabilities)")
    rules = logits_rules.normalize(kwargs, V, eos)  # (a one-token bad word equal to an EOS id is dropped, as in HF)
    forced = kwargs.get("_score_labels")
    if rules.on and forced is not None:
        raise ValueError("score() takes no logits processors: a label is scored on the model's own logits")
    stops, criteria = stopping.normalize(kwargs, V), stopping.host_criteria(kwargs)
    if (stops or criteria) and forced is not None:
        raise ValueError("score() takes neither stop sequences nor stopping criteria: the label sequence ends a row")
    streamer = kwargs.get("streamer")
    if streamer is not None and not (callable(getattr(streamer, "put", None)) and callable(getattr(streamer, "end", None))):
        raise ValueError(f"streamer must have put(tensor) and end() (got {type(streamer).__name__})")
    n_lp = logprobs.validate(kwargs, V)
    if "inputs_embeds" in kwargs:
        raise NotImplementedError("`inputs_embeds` is not supported")  # DLL:128-129
    if (kwargs.get("num_beams", 1) or 1) != 1:
        raise NotImplementedError("beam search is not built (harness default num_beams=1)")
    n_return = return_sequences(kwargs)
    constraint, allowed_fn = constraints.normalize(kwargs, V, eos, batch, n_return)
    rt, sampled = route(kwargs, rules, V, config.eos_token_id, allowed_fn is not None or (constraint is not None and not constraint.device_route)), None
    if kwargs.get("do_sample", False) and sampling.device_route(kwargs, V, config.eos_token_id):
        # seed=<int>: the draw moves into the captured graphs (device data, in no graph key).  Validated whatever the route: processors past the device caps still send it to the host loop
        sampled = sampling.normalize_params(kwargs.get("temperature"), kwargs.get("top_k"), kwargs.get("top_p")) + (int(kwargs["seed"]), int(kwargs.get("sample_row_base", 0) or 0))
    want_dict, pad, top_p = bool(kwargs.get("return_dict_in_generate")), kwargs.get("pad_token_id", config.pad_token_id), kwargs.get("top_p")
    return Request(eos=eos, pad=0 if pad is None else int(pad), min_new=int(kwargs.get("min_new_tokens", 0) or 0), rules=rules, n_lp=n_lp, sampled=sampled if rt == "device" else None,
                   temperature=float(kwargs.get("temperature", 1.0) or 1.0), top_k=int(kwargs.get("top_k", 0) or 0), top_p=None if top_p is None else float(top_p),
                   generator=kwargs.get("generator"), want_dict=want_dict, want_scores=want_dict and bool(kwargs.get("output_scores")), want_logits=want_dict and bool(kwargs.get("output_logits")),
                   sync_every=sync_every if kwargs.get("sync_every") is None else int(kwargs["sync_every"]), forced=forced, attention_mask=kwargs.get("attention_mask"),
                   image_features=kwargs.get("image_features"), host_layout=bool(kwargs.get("_host_layout")), route=rt, max_new_tokens=kwargs.get("max_new_tokens"), max_length=kwargs.get("max_length"), n_return=n_return,
                   stops=stops, criteria=criteria, streamer=streamer, constraint=constraint, allowed_fn=allowed_fn, guidance=guide)


def host_loop(logits, advance, req: Request, max_new: int, greedy: bool, finish=None, negative=None):
    """The plain decoding loop of the host routes.  logits: the first step's fp32 [B, V]; advance(next_ids [B]) -> the next step's, called once per token but the
    last.  Per step, in HF's order: the logits processors on the tokens emitted in this call, temperature, the EOS ban of min_new_tokens, top-k, top-p, then the
    argmax (`greedy`) or a draw with torch's generator; pad behind a row's EOS; stops when every row has finished.  -> (tokens: a list of [B], scores: the
    processed logits per step, raw: the model's own logits per step, kept only when log-probabilities are asked for).  No device work of its own.
    req.stops: a row also finishes when its emitted tokens end in a stop sequence (stopping.tail_matches; min_new_tokens does not hold that back).  req.criteria:
    every callable is called once per step as c(ids [B, t], scores [B, V]) -- the tokens emitted in this call, this step's included, as HF calls a criterion when
    driven by inputs_embeds, and the step's processed logits -- and returns a bool (every row) or a bool tensor [B].  req.streamer: put(an empty [B, 0] tensor)
    first, put(tokens [B] on the CPU) after every pick, end() once.  finish: a list that receives one int64 [B] tensor, the column at which each row finished
    (the number of tokens where it did not).
    req.constraint (constraints.Table): every row keeps a state; behind the logits processors and in front of the temperature, constraints.apply leaves only the
    tokens with an edge out of the row's state, and the row's token -- pad for a finished row, as the device appends it -- then moves the state
    (constraints.advance).  req.allowed_fn (prefix_allowed_tokens_fn=): at the same place, every unfinished row is masked to fn(b, the row's tokens emitted in
    this call, an int64 1-D tensor).
    req.guidance with negative = (the negative stream's first logits fp32 [B, V], its advance): in front of everything else guidance.apply turns the two streams'
    raw logits into the guided scores (HF's order: the first processor); both streams are advanced with the same picked token; `raw` stays the conditional stream's."""
    B, eos = logits.shape[0], list(req.eos)
    neg_logits, neg_advance = negative if (req.guidance is not None and negative is not None) else (None, None)
    states = None if req.constraint is None else req.constraint.starts(B // req.constraint.n_return)
    finished = torch.zeros(B, dtype=torch.bool, device=logits.device)
    finish_col = torch.full((B,), max_new, dtype=torch.int64, device=logits.device)
    toks, scores, raw = [], [], []
    if req.streamer is not None:
        req.streamer.put(torch.zeros((B, 0), dtype=torch.int64))
    for step in range(max_new):
        z = logits
        if req.n_lp >= 0:
            raw.append(z.clone())
        if neg_logits is not None:
            z = guidance.apply(z, neg_logits, *req.guidance)
        if req.rules.on:
            z = req.rules.apply(z, torch.stack(toks, dim=1) if toks else [[]] * B)
        if states is not None:
            z = constraints.apply_rows(req.constraint, z, states)
        elif req.allowed_fn is not None:
            ids, done = torch.stack(toks, dim=1) if toks else torch.zeros((B, 0), dtype=torch.int64, device=z.device), finished.tolist()
            z = torch.stack([z[b].float().clone() if done[b] else constraints.mask_to(z[b], req.allowed_fn(b, ids[b])) for b in range(B)])
        z = z / req.temperature  # (a new tensor; / 1.0 is exact)
        if step < req.min_new and eos:
            z[:, eos] = float("-inf")
        if req.top_k > 0:
            kth = torch.topk(z, min(req.top_k, z.shape[-1]), dim=-1).values[:, -1:]
            z = z.masked_fill(z < kth, float("-inf"))
        if req.top_p is not None and req.top_p < 1.0:
            sz, si = torch.sort(z, dim=-1, descending=False)
            remove = sz.softmax(dim=-1).cumsum(dim=-1) <= (1.0 - req.top_p)
            remove[:, -1] = False  # always keep the most probable token
            z = z.masked_fill(remove.scatter(1, si, remove), float("-inf"))
        scores.append(z)
        nxt = z.argmax(dim=-1) if greedy else torch.multinomial(z.softmax(dim=-1), 1, generator=req.generator)[:, 0]
        nxt = torch.where(finished, torch.full_like(nxt, req.pad), nxt)
        toks.append(nxt)
        if states is not None:
            states = [constraints.advance(req.constraint, s, t) for s, t in zip(states, nxt.tolist())]
        if req.streamer is not None:
            req.streamer.put(nxt.detach().to("cpu", torch.int64))
        was = finished
        for e in eos:
            finished = finished | (nxt == e)
        if req.stops or req.criteria:
            ids = torch.stack(toks, dim=1)
            if req.stops:
                finished = finished | torch.tensor([stopping.tail_matches(row, req.stops) for row in ids.tolist()], dtype=torch.bool, device=finished.device)
            for c in req.criteria:
                r = c(ids, z)
                finished = finished | (r.to(device=finished.device, dtype=torch.bool).reshape(B) if torch.is_tensor(r) else torch.full_like(finished, bool(r)))
        if finish is not None:
            finish_col = torch.where(finished & ~was, torch.full_like(finish_col, step), finish_col)
        if req.can_finish and bool(finished.all()):
            break
        if step + 1 < max_new:
            logits = advance(nxt)
            if neg_logits is not None:
                neg_logits = neg_advance(nxt)
    if finish is not None:
        finish.append(finish_col.clamp(max=len(toks)))
    if req.streamer is not None:
        req.streamer.end()
    return toks, scores, raw
