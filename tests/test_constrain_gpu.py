"""GPU: the constraint kernel (dl_logits_constrain, through ops.logits_constrain) against the rule in dynamic_llava_amd/constraints.py.

Everything is compared as bits: the kernel converts a logit to fp32 and either keeps it or replaces it by -inf, and it stores one state per row; there is
no arithmetic and no tolerance to state.  `out` and `state_hist` lie between guard bands filled with NaN bits, and every slot of state_hist but the one the
launch owns must keep what it held."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import constraints as C  # noqa: E402

SEED = 20261021
G = 64  # guard band, elements
NAN_BITS = 0x7FC00000
EOS = 2


def _bits(t):
    return t.contiguous().view(torch.int32)


def _automaton(V):
    """States by out-degree: 0: one token; 1: two tokens, at lo and hi - 1 of the second tile; 2 (accepting: + the EOS edge): tokens in the first and the last
    tile only; 3: all V tokens; 4: one token, the last of the vocabulary."""
    last_lo = ((V - 1) // 2048) * 2048
    e = [[(7, 1)],
         [(2048, 2), (min(4095, V - 1), 3)],
         [(t, 4) for t in sorted({0, 5, 2047, last_lo, V - 1})],
         [(t, 3) for t in range(V)],
         [(V - 1, 0)]]
    ptr, tok, nxt = [0], [], []
    for s in e:
        tok += [t for t, _ in s]
        nxt += [n for _, n in s]
        ptr.append(len(tok))
    return C.compile(C.TokenAutomaton(ptr, tok, nxt, [False, False, True, False, False], vocab_size=V), (EOS,))


_TABLES = {}


def _table(V):
    if V not in _TABLES:
        from dynamic_llava_amd import hip_ops as ops

        t = _automaton(V)
        _TABLES[V] = (t, ops.constraint_table_write(ops.constraint_table_block("cuda"), *t.words()))
    return _TABLES[V]


def _rows(V, cap):
    """(step, the state in slot s - 1, the token in column s - 1, start) per row: every way the state is found."""
    return [
        (0, C.DONE, 0, 4),  # step 0: the start state -- out-degree 1
        (0, C.DONE, 0, 1),  # two tokens at the edges of one tile
        (0, C.DONE, 0, 3),  # all V tokens
        (0, C.DONE, 0, 2),  # first and last tile only, + EOS
        (0, C.DONE, 0, C.DONE),  # a row that starts DONE passes through
        (3, 0, 7, 3),  # step > 0 advances on out_ids[b, s - 1]: 0 -7-> 1 (start is not read)
        (1, 1, 2048, 0),  # 1 -> 2
        (2, 2, EOS, 0),  # the EOS edge of an accepting state: DONE
        (4, 3, V - 2, 0),  # 3 -> 3
        (2, 0, 8, 0),  # an id with no edge: DONE
        (2, 0, V, 0),  # ids outside [0, V): DONE
        (2, 3, -1, 0),
        (2, 0, 2 ** 32 + 7, 0),  # (not 7: a 32-bit compare would follow the edge)
        (5, C.DONE, 7, 0),  # DONE stays DONE
        (cap, 1, min(4095, V - 1), 0),  # step == out_cap: slot out_cap
        (cap + 5, 4, V - 1, 0),  # step > out_cap is clamped: reads column out_cap - 1, writes slot out_cap
        (-2, 0, 7, 2),  # step < 0 is clamped to 0
    ]


def _expect(t, x, rows, cap, hist0, n_states=None):
    """The rule on the CPU -> (out fp32 [B, V], state_hist)."""
    V = x.shape[1]
    ns = t.n_states if n_states is None else n_states
    out, hist = [], hist0.clone()
    for b, (step, prev, tok, start) in enumerate(rows):
        s = min(max(step, 0), cap)
        state = start if s == 0 else (C.advance(t, prev, tok) if 0 <= tok < V else C.DONE)
        if not 0 <= state < ns:
            state = C.DONE
        hist[b, s] = state
        out.append(C.apply(t, x[b], state))
    return torch.stack(out), hist


def _launch(t, tab, x, rows, cap, layout="aligned", in_place=False):
    """-> (out, state_hist, expected out, expected state_hist), all on the CPU.  layout "odd": a row stride of V + 3 and an input base that is not 16-byte aligned, and
    an output base that is not either (the scalar paths); in_place: out is the fp32 input itself."""
    from dynamic_llava_amd import hip_ops as ops

    B, V = x.shape
    g = torch.Generator().manual_seed(SEED + 7)
    ids = torch.randint(0, V, (B, max(cap, 1)), generator=g).to(torch.int64)[:, :cap]
    hist0 = torch.randint(0, t.n_states, (B, cap + 1), generator=g).to(torch.int32)
    for b, (step, prev, tok, _) in enumerate(rows):
        s = min(max(step, 0), cap)
        if s > 0:
            ids[b, s - 1], hist0[b, s - 1] = tok, prev
    step = torch.tensor([r[0] for r in rows], dtype=torch.int32).cuda()
    start = torch.tensor([r[3] for r in rows], dtype=torch.int32).cuda()
    off = 1 if layout == "odd" else 0
    hbuf = torch.full((G + B * (cap + 1) + G,), NAN_BITS, dtype=torch.int32)
    hbuf[G : G + B * (cap + 1)] = hist0.reshape(-1)
    hbuf = hbuf.cuda()
    hist = hbuf[G : G + B * (cap + 1)].view(B, cap + 1)
    obuf = torch.full((G + off + B * V + G,), float("nan"), dtype=torch.float32).cuda()
    out = obuf[G + off : G + off + B * V].view(B, V)
    if in_place:
        assert x.dtype == torch.float32
        out.copy_(x)
        xd = out
    elif layout == "odd":
        store = torch.zeros(1 + B * (V + 3), dtype=x.dtype).cuda()
        xd = store[1:].view(B, V + 3)[:, :V]
        xd.copy_(x)
    else:  # a 16-byte aligned base and a row stride of whole 16-byte groups: the vector loads, with the row's last partial group where V is no multiple of 8
        xd = torch.zeros((B, -(-V // 8) * 8), dtype=x.dtype).cuda()[:, :V]
        xd.copy_(x)
    x_before, ids_d = xd.clone(), ids.cuda()
    ops.logits_constrain(xd, out, tab, start, hist, ids_d if cap > 0 else None, step if cap > 0 else None)
    torch.cuda.synchronize()
    nan = torch.full((G,), NAN_BITS, dtype=torch.int32)
    assert torch.equal(_bits(obuf[:G].cpu()), nan) and torch.equal(_bits(obuf[G + off + B * V :].cpu()), nan), "out's guard bands"
    assert torch.equal(hbuf[:G].cpu(), nan) and torch.equal(hbuf[G + B * (cap + 1) :].cpu(), nan), "state_hist's guard bands"
    if not in_place:
        assert torch.equal(xd.view(torch.int16 if x.element_size() == 2 else torch.int32), x_before.view(torch.int16 if x.element_size() == 2 else torch.int32)), "the input is only read"
    assert torch.equal(ids_d.cpu(), ids)
    want, want_hist = _expect(t, x, rows, cap, hist0)
    return out.cpu(), hist.cpu(), want, want_hist


def _logits(B, V, dtype, seed):
    g = torch.Generator().manual_seed(SEED + seed)
    x = (torch.randn(B, V, generator=g) * 8).to(dtype)
    x[0, 7], x[0, V - 1], x[0, 2048], x[0, 0] = float("-inf"), -0.0, 3.0e4, 0.0  # hard values where edges point
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("V", [32000, 2048 + 5])
def test_kernel_matches_the_rule(V, layout, dtype):
    """B = 3 over every way a row finds its state (and B = 1 over the first six), a different state per row."""
    cap = 8
    t, tab = _table(V)
    rows = _rows(V, cap)
    rows += rows[: (-len(rows)) % 3]
    batches = [rows[i : i + 3] for i in range(0, len(rows), 3)] + [[r] for r in rows[:6]]
    for i, batch in enumerate(batches):
        x = _logits(len(batch), V, dtype, i)
        got, hist, want, want_hist = _launch(t, tab, x, batch, cap, layout)
        assert torch.equal(_bits(got), _bits(want)), (i, batch, int((_bits(got) != _bits(want)).sum()))
        assert torch.equal(hist, want_hist), (i, batch, hist.tolist(), want_hist.tolist())  # slot s holds the state, every other slot what it held


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("V", [32000, 2048 + 5])
def test_in_place_fp32(V, layout):
    cap = 8
    t, tab = _table(V)
    rows = _rows(V, cap)
    for i in range(0, len(rows) - 2, 3):
        x = _logits(3, V, torch.float32, 40 + i)
        got, hist, want, want_hist = _launch(t, tab, x, rows[i : i + 3], cap, layout, in_place=True)
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(hist, want_hist), (i, rows[i : i + 3])


def test_what_the_states_allow():
    """The cases are what they claim: the out-degrees, the DONE rows and the live ones."""
    V, cap = 32000, 8
    t, tab = _table(V)
    assert [len(t.allowed(s)) for s in range(5)] == [1, 2, 6, V, 1] and t.allowed(1) == [2048, 4095] and t.allowed(2) == [0, EOS, 5, 2047, 30720, V - 1]
    rows = _rows(V, cap)
    x = _logits(len(rows), V, torch.bfloat16, 99)
    got, hist, want, want_hist = _launch(t, tab, x, rows, cap)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(hist, want_hist)
    states = [int(want_hist[b, min(max(r[0], 0), cap)]) for b, r in enumerate(rows)]
    assert states == [4, 1, 3, 2, C.DONE, 1, 2, C.DONE, 3, C.DONE, C.DONE, C.DONE, C.DONE, C.DONE, 3, 0, 2]
    for b, s in enumerate(states):
        kept = (got[b] > float("-inf")).sum().item()
        if s == C.DONE or s == 3:
            assert torch.equal(_bits(got[b]), _bits(x[b].float()))  # passes through, -inf and -0.0 included
        else:
            assert kept <= len(t.allowed(s)) and torch.equal(got[b][t.allowed(s)], x[b].float()[t.allowed(s)])


def test_no_step_is_step_zero():
    V = 2048 + 5
    t, tab = _table(V)
    x = _logits(2, V, torch.float16, 5)
    got, hist, want, want_hist = _launch(t, tab, x, [(0, C.DONE, 0, 1), (0, C.DONE, 0, 2)], 0)
    assert torch.equal(_bits(got), _bits(want)) and hist.tolist() == [[1], [2]]


def _bad_block(t, patch):
    from dynamic_llava_amd import hip_ops as ops

    blk = ops.constraint_table_write(torch.zeros(ops.CONSTRAIN_TABLE_WORDS, dtype=torch.int32), *t.words())
    patch(blk, ops.CONSTRAIN_HEADER_WORDS, ops.CONSTRAIN_HEADER_WORDS + ops.CONSTRAIN_MAX_STATES + 1)
    return blk.cuda()


def test_bad_tables_are_refused_never_followed():
    """Tables built directly, as a stale or overwritten block would look: counts past the caps, a `next` out of range, edge ranges outside the table, a start
    state out of range.  The affected rows behave as DONE (the logits pass through, DONE is stored); nothing else is written."""
    from dynamic_llava_amd import hip_ops as ops

    V, cap = 2048 + 5, 8
    t, _ = _table(V)
    rows = [(0, C.DONE, 0, 1), (3, 0, 7, 0), (2, 1, 2048, 0)]  # good table: states 1, 1, 2
    x = _logits(3, V, torch.bfloat16, 60)
    passthrough = x.float()

    def run(tab, rows_=rows):
        got, hist, want, want_hist = _launch(t, tab, x, rows_, cap)
        return got, hist, want_hist

    def all_done(tab, why):
        got, hist, want_hist = run(tab)
        for b, r in enumerate(rows):
            want_hist[b, r[0]] = C.DONE
        assert torch.equal(_bits(got), _bits(passthrough)) and torch.equal(hist, want_hist), why

    def set_word(i, v):
        def patch(blk, p0, e0):
            blk[i] = v
        return patch

    all_done(_bad_block(t, set_word(0, ops.CONSTRAIN_MAX_STATES + 1)), "n_states past the cap")
    all_done(_bad_block(t, set_word(0, 2 ** 31 - 1)), "n_states huge")
    all_done(_bad_block(t, set_word(0, 0)), "no states")
    all_done(_bad_block(t, set_word(0, -4)), "n_states negative")
    all_done(_bad_block(t, set_word(1, ops.CONSTRAIN_MAX_EDGES + 1)), "n_edges past the cap")
    all_done(_bad_block(t, set_word(1, -1)), "n_edges negative")

    # a `next` out of range: the edge 0 -7-> 1 now leads nowhere a state is; rows 0 and 2 do not take it
    for bad_next in (t.n_states, 10 ** 6, -5):
        def patch(blk, p0, e0, v=bad_next):
            blk[e0 + 2 * t.state_ptr[0] + 1] = v
        got, hist, want_hist = run(_bad_block(t, patch))
        want_hist[1, 3] = C.DONE
        assert torch.equal(_bits(got[1]), _bits(passthrough[1])) and torch.equal(hist, want_hist), bad_next
        assert torch.equal(_bits(got[0]), _bits(C.apply(t, x[0], 1))) and torch.equal(_bits(got[2]), _bits(C.apply(t, x[2], 2)))

    # state 1's edge range runs past n_edges / is reversed / starts below 0: rows 0 and 1 (state 1) are DONE, row 2 walks OUT of state 1 and is DONE too
    for lo_hi in ((t.state_ptr[1], t.n_edges + 1), (t.state_ptr[2], t.state_ptr[1]), (-3, t.state_ptr[2]), (0, 2 ** 31 - 1)):
        def patch(blk, p0, e0, v=lo_hi):
            blk[p0 + 1], blk[p0 + 2] = v
        got, hist, want_hist = run(_bad_block(t, patch))
        for b, r in enumerate(rows):
            want_hist[b, r[0]] = C.DONE
        # (state 0's and state 2's own ranges share the patched words: whichever states the rows reach, nothing outside the table is read and DONE is what they get)
        assert torch.equal(hist, want_hist) and torch.equal(_bits(got), _bits(passthrough)), lo_hi

    # a start state out of range
    _, tab = _table(V)
    for bad_start in (t.n_states, -7, 2 ** 31 - 1):
        r2 = [(0, C.DONE, 0, bad_start), rows[1], rows[2]]
        got, hist, want_hist = run(tab, r2)
        assert int(hist[0, 0]) == C.DONE and torch.equal(hist, want_hist) and torch.equal(_bits(got[0]), _bits(passthrough[0]))

    # an edge list that is not sorted must not index past the tile's mask: state 3's V edges with two tokens swapped for far-away values
    def patch(blk, p0, e0):
        blk[e0 + 2 * (t.state_ptr[3] + 10)] = 10 ** 6
        blk[e0 + 2 * (t.state_ptr[3] + 11)] = -9
    got, hist, _ = run(_bad_block(t, patch), [(0, C.DONE, 0, 3)] * 3)
    sel = got > float("-inf")
    assert hist[:, 0].tolist() == [3, 3, 3] and torch.equal(got[sel], x.float()[sel])  # (what a search in an unsorted list leaves out is unspecified; what is kept is exact)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_chained_with_the_step_closing_kernel(dtype):
    """Four steps of dl_logits_constrain + dl_decode_advance walk a trie exactly as the host rule does: argmax of the constrained row, EOS from accepting
    states, pad behind it, and the states of every step in state_hist."""
    from dynamic_llava_amd import hip_ops as ops

    V, B, cap, PAD = 32000, 3, 6, 1
    choices = [[31999, 5], [31999], [4000, 4001, 4002], [7]]
    t = C.compile(C.TokenAutomaton.from_choices(choices, vocab_size=V), (EOS,))
    tab = ops.constraint_table_write(ops.constraint_table_block("cuda"), *t.words())
    g = torch.Generator().manual_seed(SEED + 11)
    start = torch.zeros(B, dtype=torch.int32, device="cuda")
    hist = torch.full((B, cap + 1), C.DONE, dtype=torch.int32, device="cuda")
    ids, step, fin = torch.zeros((B, cap), dtype=torch.int64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    nxt, proc = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.empty((B, V), dtype=torch.float32, device="cuda")
    states, done, rows = [0] * B, [False] * B, [[] for _ in range(B)]
    for j in range(cap):
        x = (torch.randn(B, V, generator=g) * 4).to(dtype)
        x[0, 31999] += 50.0 if j == 0 else 0.0  # row 0 starts down the shared prefix
        ops.logits_constrain(x.cuda(), proc, tab, start, hist, ids, step)
        ops.decode_advance(proc, nxt, ids, step, fin, EOS, PAD)
        torch.cuda.synchronize()
        want = C.apply_rows(t, x, states)
        assert torch.equal(_bits(proc.cpu()), _bits(want)), j
        assert hist[:, j].cpu().tolist() == states, (j, hist.cpu().tolist())
        for b in range(B):
            tok = PAD if done[b] else int(want[b].argmax())
            rows[b].append(tok)
            done[b] = done[b] or tok == EOS
            states[b] = C.advance(t, states[b], tok)
        assert nxt.cpu().tolist() == [r[-1] for r in rows], j
    assert all(done) and ids.cpu().tolist() == rows
    for r in rows:
        assert r[: r.index(EOS)] in choices and set(r[r.index(EOS) + 1 :]) <= {PAD}
    assert C.complete(t, ids.cpu()).tolist() == [True] * B
