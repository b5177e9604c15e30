"""Constrained decoding (dl_logits_constrain, csrc/constrain.hip), written once in plain torch / Python.

Same role as logits_rules.py, sampling.py and stopping.py: this file is the contract the kernel is tested against; it runs on the CPU (and on any torch
device) and is what the host routes of generate() apply to a step's logits themselves (request.host_loop).

A constraint is a deterministic automaton over token ids.  Every row of a request keeps a state; at every step the tokens with no edge out of that state
are set to -inf before the selection rule runs, and the token the rule then picks moves the state.  That is HF's PrefixConstrainedLogitsProcessor with the
function `prefix -> allowed ids` given as data (tests/test_constraints_cpu.py holds `apply` to the installed transformers bit for bit), which is what lets
the captured decode graphs serve it: the automaton is device memory, one graph serves every automaton.

`TokenAutomaton(state_ptr, edge_tok, edge_next, accepting)` is the automaton in CSR form: state s owns edges state_ptr[s] : state_ptr[s + 1], an edge is
(token, next state), a state's edges are kept sorted by token, state 0 is the start state, `accepting` marks the states in which a row may end.
`from_choices(seqs)` builds the trie of a list of answers, `from_allowed(ids)` the one-state whitelist.

`compile(automata, eos, B, n_return)` makes the form the device and the host loop walk (`Table`): one automaton for every row or a list of B merged into
one table with per-row start states; every accepting state gets one edge per EOS id of the request, leading to DONE = -1.

The rule, per row and step:

1. `advance(table, state, tok)`: the `next` of the state's edge with token `tok`; DONE when the state is DONE or there is no such edge (only a finished row,
   whose token is pad, misses an edge).
2. `apply(table, z, state)`: in DONE the row unchanged; otherwise fp32 z with every token that has no edge out of `state` at -inf, the allowed ones keep
   their bits.
3. The step runs after the logits processors (repetition penalty, n-gram and bad-word bans: HF's order) and before temperature, the EOS ban of
   min_new_tokens, top-k, top-p and the pick.

A row that the processors and the constraint together leave entirely -inf (a bad word that is a state's only edge, say) is the caller's error, as in HF:
nothing defends against it.  min_new_tokens > 0 is refused with a constraint (the EOS ban could empty a terminal accepting state's row)."""
from __future__ import annotations

import bisect
import numbers
import operator
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

DONE = -1
# what the device route takes, counted after the EOS edges are added (mirrored in include/dynllava.h: DL_CONSTRAIN_MAX_*); a request beyond them runs the
# plain loop over forward() with this file's rule
MAX_STATES = 4096
MAX_EDGES = 131072


def _is_int(v) -> bool:
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _ints(v, what):
    """A list / tuple of ints or a 1-D integer tensor -> a list of ints."""
    if torch.is_tensor(v):
        if v.dim() != 1 or v.is_floating_point() or v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f"{what} must be a 1-D integer tensor (got {v.dtype}, {tuple(v.shape)})")
        return [int(t) for t in v.tolist()]
    if isinstance(v, (list, tuple)) and all(type(t) is int for t in v):  # (the common case, without the abstract-class checks: a whitelist has tens of thousands of ids)
        return list(v)
    if not isinstance(v, (list, tuple)) or not all(_is_int(t) for t in v):
        raise ValueError(f"{what} must be a list of ints or a 1-D integer tensor (got {v!r})")
    return [int(t) for t in v]


class TokenAutomaton:
    """A deterministic automaton over token ids in CSR form (the module docstring).  Raises ValueError for a state_ptr that is not a non-decreasing
    [0 .. n_edges] of at least two entries, a negative token (or one >= vocab_size, when that is given here or to `check_vocab`), a next_state outside
    [0, n_states) and a state with two edges of one token.  The edges of a state are stored sorted by token, whatever order they came in."""

    def __init__(self, state_ptr, edge_tok, edge_next, accepting, vocab_size=None):
        ptr, tok, nxt = _ints(state_ptr, "state_ptr"), _ints(edge_tok, "edge_tok"), _ints(edge_next, "edge_next")
        acc = [bool(a) for a in (accepting.tolist() if torch.is_tensor(accepting) else accepting)]
        n = len(ptr) - 1
        if n < 1 or ptr[0] != 0 or ptr[-1] != len(tok) or any(a > b for a, b in zip(ptr, ptr[1:])):
            raise ValueError(f"state_ptr must rise from 0 to the number of edges ({len(tok)}) over at least one state (got {ptr[:8]}{'...' if len(ptr) > 8 else ''})")
        if len(nxt) != len(tok) or len(acc) != n:
            raise ValueError(f"{len(tok)} edge tokens, {len(nxt)} edge targets; {n} states, {len(acc)} accepting flags")
        if nxt and (min(nxt) < 0 or max(nxt) >= n):
            raise ValueError(f"an edge leads to a state outside [0, {n})")
        if tok and min(tok) < 0:
            raise ValueError("an edge has a negative token id")
        self.state_ptr, self.edge_tok, self.edge_next, self.accepting = ptr, [], [], acc
        for s in range(n):
            ts, ns = tok[ptr[s] : ptr[s + 1]], nxt[ptr[s] : ptr[s + 1]]
            if not all(map(operator.lt, ts, ts[1:])):  # (not yet sorted and distinct)
                pairs = sorted(zip(ts, ns))
                if any(a[0] == b[0] for a, b in zip(pairs, pairs[1:])):
                    raise ValueError(f"state {s} has two edges with the same token: the automaton must be deterministic")
                ts, ns = [p[0] for p in pairs], [p[1] for p in pairs]
            self.edge_tok += ts
            self.edge_next += ns
        if vocab_size is not None:
            self.check_vocab(vocab_size)

    @property
    def n_states(self) -> int:
        return len(self.state_ptr) - 1

    @property
    def n_edges(self) -> int:
        return len(self.edge_tok)

    def check_vocab(self, vocab_size):
        if self.edge_tok and max(self.edge_tok) >= int(vocab_size):
            raise ValueError(f"an edge's token {max(self.edge_tok)} is outside [0, {int(vocab_size)})")
        return self

    def edges(self, s):
        """State s's edges as (token, next state) pairs, sorted by token."""
        a, b = self.state_ptr[s], self.state_ptr[s + 1]
        return list(zip(self.edge_tok[a:b], self.edge_next[a:b]))

    @classmethod
    def from_choices(cls, seqs, vocab_size=None):
        """The trie of a list of non-empty token sequences: a row says exactly one of them.  The node a choice ends in is accepting (a choice that is a prefix of
        another gives a node that is accepting and has children); a choice given twice counts once."""
        if not isinstance(seqs, (list, tuple)) or len(seqs) == 0:
            raise ValueError(f"guided_choice must be a non-empty list of non-empty token sequences (got {seqs!r})")
        children, acc = [{}], [False]
        for q in seqs:
            q = _ints(q, "guided_choice: a choice")
            if len(q) == 0:
                raise ValueError("guided_choice: an empty choice")
            s = 0
            for t in q:
                if t not in children[s]:
                    children[s][t] = len(children)
                    children.append({})
                    acc.append(False)
                s = children[s][t]
            acc[s] = True
        ptr, tok, nxt = [0], [], []
        for c in children:
            for t in sorted(c):
                tok.append(t)
                nxt.append(c[t])
            ptr.append(len(tok))
        return cls(ptr, tok, nxt, acc, vocab_size)

    @classmethod
    def from_allowed(cls, ids, vocab_size=None):
        """A fixed whitelist: one accepting state with a self-loop per id (an id given twice counts once)."""
        ids = sorted(set(_ints(ids, "allowed_token_ids")))
        if not ids:
            raise ValueError("allowed_token_ids must hold at least one id")
        return cls([0, len(ids)], ids, [0] * len(ids), [True], vocab_size)


@dataclass(frozen=True)
class Table:
    """A request's constraint in the form that is walked (`compile`): the merged CSR table with the EOS edges in place, and the start state of every prompt."""
    state_ptr: Tuple[int, ...]
    edge_tok: Tuple[int, ...]
    edge_next: Tuple[int, ...]  # DONE: the edge an EOS id takes out of an accepting state
    prompt_start: Tuple[int, ...]  # one entry: every prompt starts there; else one per prompt
    n_return: int = 1
    eos: Tuple[int, ...] = ()
    _tensors: dict = field(default_factory=dict, compare=False, repr=False)

    @property
    def n_states(self) -> int:
        return len(self.state_ptr) - 1

    @property
    def n_edges(self) -> int:
        return len(self.edge_tok)

    @property
    def device_route(self) -> bool:
        """True when dl_logits_constrain takes the table (inside the captured graphs)."""
        return self.n_states <= MAX_STATES and self.n_edges <= MAX_EDGES

    def starts(self, B=None):
        """-> the rows' start states, a list of B * n_return ints: rows b * n .. b * n + n - 1 share prompt b's."""
        ps = list(self.prompt_start)
        if len(ps) == 1 and B is not None:
            ps = ps * int(B)
        elif B is not None and len(ps) != int(B):
            raise ValueError(f"constraint: {len(ps)} automata for {int(B)} prompts")
        return [s for s in ps for _ in range(self.n_return)]

    def words(self):
        """-> (state_ptr int32 [n_states + 1], edges int32 [n_edges, 2]) on the CPU: what hip_ops.constraint_table_write copies into the device block."""
        if "words" not in self._tensors:
            self._tensors["words"] = (torch.tensor(self.state_ptr, dtype=torch.int32),
                                      torch.tensor([self.edge_tok, self.edge_next], dtype=torch.int32).t().contiguous().reshape(-1, 2))
        return self._tensors["words"]

    def allowed(self, state):
        """The tokens with an edge out of `state`, sorted (none in DONE)."""
        if state == DONE:
            return []
        return list(self.edge_tok[self.state_ptr[state] : self.state_ptr[state + 1]])


def compile(automata, eos, B=None, n_return=1, vocab_size=None, min_new=0) -> Table:  # noqa: A001 (the issue's name)
    """One TokenAutomaton (every row walks it) or a list of B of them (one per prompt) -> Table.  The automata are merged into one table, an automaton that occurs
    several times in the list once; every accepting state gets one edge per distinct id of `eos` (the request's EOS ids) leading to DONE.  Raises ValueError
    for a list whose length is not B, an EOS id that is already an explicit edge of an accepting state, a state reachable from a start state that is left with no
    edge at all (a dead end: a row there could say nothing -- this includes a terminal accepting state of a request without EOS ids), a token outside
    [0, vocab_size) and min_new > 0."""
    if int(min_new or 0) > 0:
        raise ValueError("a constraint takes no min_new_tokens: the EOS ban could leave a row without any allowed token")
    if isinstance(automata, TokenAutomaton):
        autos, shared = [automata], True
    else:
        if not isinstance(automata, (list, tuple)) or len(automata) == 0 or not all(isinstance(a, TokenAutomaton) for a in automata):
            raise ValueError("constraint must be a TokenAutomaton or a non-empty list of them, one per prompt")
        autos, shared = list(automata), False
        if B is not None and len(autos) != int(B):
            raise ValueError(f"constraint: {len(autos)} automata for {int(B)} prompts")
    n_return = int(n_return or 1)
    eos_set = sorted({int(e) for e in (eos or ())})
    ptr, tok, nxt, base_of, prompt_start = [0], [], [], {}, []
    for a in autos:
        if id(a) not in base_of:
            if vocab_size is not None:
                a.check_vocab(vocab_size)
            base = base_of[id(a)] = len(ptr) - 1
            for s in range(a.n_states):
                ts, ns = a.edge_tok[a.state_ptr[s] : a.state_ptr[s + 1]], [n + base for n in a.edge_next[a.state_ptr[s] : a.state_ptr[s + 1]]]
                if a.accepting[s] and eos_set:
                    hit = set(ts).intersection(eos_set)
                    if hit:
                        raise ValueError(f"the EOS id {min(hit)} is already an edge of an accepting state: the row could not end there")
                    pairs = sorted(zip(ts + eos_set, ns + [DONE] * len(eos_set)))
                    ts, ns = [p[0] for p in pairs], [p[1] for p in pairs]
                tok += ts
                nxt += ns
                ptr.append(len(tok))
        prompt_start.append(base_of[id(a)])
    # dead ends, among the states a row can reach
    seen, todo = set(prompt_start), list(set(prompt_start))
    while todo:
        s = todo.pop()
        if ptr[s] == ptr[s + 1]:
            raise ValueError(f"state {s} can be reached and has no edge at all: a row there could say nothing" + ("" if eos_set else " (an accepting state ends a row through an EOS id, and the request has none)"))
        for n in nxt[ptr[s] : ptr[s + 1]]:
            if n != DONE and n not in seen:
                seen.add(n)
                todo.append(n)
    return Table(tuple(ptr), tuple(tok), tuple(nxt), tuple(prompt_start[:1] if shared else prompt_start), n_return, tuple(int(e) for e in (eos or ())))


def advance(table: Table, state: int, tok: int) -> int:
    """The state behind `tok`: the edge's next state; DONE in DONE and where `state` has no edge with that token."""
    if state == DONE:
        return DONE
    a, b = table.state_ptr[state], table.state_ptr[state + 1]
    i = bisect.bisect_left(table.edge_tok, int(tok), a, b)
    return table.edge_next[i] if i < b and table.edge_tok[i] == int(tok) else DONE


def apply(table: Table, z_row, state: int):
    """One row of one step -> fp32 [V] (a new tensor on z_row's device): unchanged in DONE, else -inf wherever `state` has no edge."""
    assert z_row.dim() == 1
    x = z_row.float()
    if state == DONE:
        return x.clone()
    return mask_to(x, table.allowed(state))


def mask_to(z_row, ids):
    """fp32 [V] with every entry but `ids` at -inf; the entries of `ids` keep their bits (ids outside [0, V) are ignored)."""
    x = z_row.float()
    y = torch.full_like(x, float("-inf"))
    keep = [int(t) for t in ids if 0 <= int(t) < x.shape[0]]
    if keep:
        idx = torch.tensor(keep, dtype=torch.long, device=x.device)
        y[idx] = x[idx]
    return y


def apply_rows(table: Table, z, states):
    """A batch [B, V] with the rows' states -> fp32 [B, V]: `apply` per row."""
    assert z.dim() == 2 and len(states) == z.shape[0]
    return torch.stack([apply(table, z[b], int(states[b])) for b in range(z.shape[0])])


def walk(table: Table, start: int, tokens):
    """The states in which a row's tokens are chosen: [start, advance(start, t0), ...], len(tokens) + 1 entries."""
    out = [int(start)]
    for t in tokens:
        out.append(advance(table, out[-1], int(t)))
    return out


def complete(table: Table, sequences, B=None):
    """`constraint_complete` of a result: bool [rows] on the CPU -- row r ended through an EOS edge (it reached DONE by an edge, not by a token without an edge),
    instead of being cut off by max_new_tokens or a stop sequence.  sequences: int64 [rows, T], the generated tokens (pad behind a row's end)."""
    rows = sequences.tolist()
    starts = table.starts(B if B is not None else (len(rows) // table.n_return if len(table.prompt_start) == 1 else None))
    assert len(starts) == len(rows), (len(starts), len(rows))
    out = []
    for r, s in zip(rows, starts):
        done = False
        for t in r:
            a, b = table.state_ptr[s], table.state_ptr[s + 1]
            i = bisect.bisect_left(table.edge_tok, int(t), a, b)
            if not (i < b and table.edge_tok[i] == int(t)):
                break  # no edge: nothing a live row emits (a stop sequence finished it and this is pad)
            s = table.edge_next[i]
            if s == DONE:
                done = True
                break
        out.append(done)
    return torch.tensor(out, dtype=torch.bool)


# ---- generate()'s keywords ------------------------------------------------------------------------------------------------------------------------------
KEYWORDS = ("constraint", "guided_choice", "allowed_token_ids", "prefix_allowed_tokens_fn")


def normalize(kwargs, vocab_size, eos, B=None, n_return=1) -> Tuple[Optional[Table], Optional[object]]:
    """generate()'s kwargs -> (the compiled Table or None, prefix_allowed_tokens_fn or None).  At most one of constraint= (a TokenAutomaton or a list of B),
    guided_choice= (a list of token sequences, for every row), allowed_token_ids= (a list of ids, for every row) and prefix_allowed_tokens_fn= (HF's callable
    fn(batch_id, ids_1d) -> list of ids, called with the tokens emitted in this call) may be given; None is "not given".  Raises ValueError for two of them, for
    score() with any, and for whatever TokenAutomaton and `compile` refuse."""
    given = [k for k in KEYWORDS if kwargs.get(k) is not None]
    if not given:
        return None, None
    if len(given) > 1:
        raise ValueError(f"at most one of {', '.join(KEYWORDS)} may be given (got {', '.join(given)})")
    if kwargs.get("_score_labels") is not None:
        raise ValueError("score() takes no constraint: a label is scored on the model's own logits")
    k, v = given[0], kwargs[given[0]]
    min_new = int(kwargs.get("min_new_tokens", 0) or 0)
    if k == "prefix_allowed_tokens_fn":
        if not callable(v):
            raise ValueError(f"prefix_allowed_tokens_fn must be callable as fn(batch_id, ids_1d) -> list of ids (got {type(v).__name__})")
        if min_new > 0:
            raise ValueError("a constraint takes no min_new_tokens: the EOS ban could leave a row without any allowed token")
        return None, v
    if k == "guided_choice":
        v = TokenAutomaton.from_choices(v)
    elif k == "allowed_token_ids":
        v = TokenAutomaton.from_allowed(v)
    return compile(v, eos, B, n_return, vocab_size=vocab_size, min_new=min_new), None
