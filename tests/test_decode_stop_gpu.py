"""GPU: dl_decode_stop (through the C ABI) against the rule in dynamic_llava_amd/stopping.py (reference_flags), bit for bit.

216 rows over a 3-token vocabulary with out_cap 12, so that matches are common: nine launches of 24 rows, launch n with n stop sequences (0..8) whose lengths
walk through 1..8.  Per launch the rows' `step` values are 0, 1, one below / at / one past a sequence's length, out_cap and past out_cap; some rows are already
finished; some have a sequence planted at their tail; one row's would-be match continues into the end of the previous row (the sequence is longer than the row:
it must not stop); the table's unused rows hold one-token sequences that would match almost every row, the ids behind a sequence's length and the reserved words
hold garbage.  Every buffer lies inside guard bands: out_ids, step, the table and the bands must come back untouched, `finished` equal to the rule."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import hip_ops as ops  # noqa: E402
from dynamic_llava_amd import stopping  # noqa: E402

CAP, ROWS, VOCAB, GUARD = 12, 24, 3, 64
S64, S32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
W = ops.STOP_TABLE_WORDS


def _lengths(n):
    """The lengths of launch n's sequences: over the nine launches every length 1..8 occurs, alone and beside others."""
    return [(n + 3 * i) % 8 + 1 for i in range(n)]


def _case(n, g):
    lens = _lengths(n)
    seqs = [torch.randint(0, VOCAB, (L,), generator=g).tolist() for L in lens]
    out = torch.randint(0, VOCAB, (ROWS, CAP), generator=g)
    marks = sorted({0, 1, CAP, CAP + 3} | {max(0, min(CAP, L + d)) for L in lens for d in (-1, 0, 1)})
    step = torch.tensor([marks[b % len(marks)] if b < 16 else int(torch.randint(0, CAP + 1, (1,), generator=g)) for b in range(ROWS)], dtype=torch.int32)
    fin = torch.zeros(ROWS, dtype=torch.int32)
    fin[5::7] = 1  # rows that are already finished
    for b in range(2, ROWS, 3):  # a sequence planted at the row's tail (where it fits)
        if seqs:
            s, t = seqs[b % n], min(int(step[b]), CAP)
            if len(s) <= t:
                out[b, t - len(s) : t] = torch.tensor(s)
    if n >= 1 and min(lens) >= 3:  # (launches 2 and 4) the match that would continue into the previous row: the longest sequence, cut between rows 9 and 10; nothing shorter fits row 10
        s = seqs[lens.index(max(lens))]
        k = len(s) - 2
        out[9, CAP - k :] = torch.tensor(s[:k])
        out[10, :2] = torch.tensor(s[k:])
        step[10], fin[10] = 2, 0
    tab = torch.randint(0, VOCAB, (W,), generator=g, dtype=torch.int32)  # garbage everywhere, then what is read
    tab[0] = n
    tab[1:8] = torch.tensor([8, -1, 3, 1, 1, 2, 99], dtype=torch.int32)
    for i in range(8):
        if i < n:
            tab[8 + 9 * i] = lens[i]
            tab[9 + 9 * i : 9 + 9 * i + lens[i]] = torch.tensor(seqs[i], dtype=torch.int32)
        else:
            tab[8 + 9 * i], tab[9 + 9 * i] = 1, i % VOCAB  # an unused row that would match a third of all rows
    return out, step, fin, tab


def _cases():
    g = torch.Generator().manual_seed(1234)
    return [_case(n, g) for n in range(9)]


def _banded(t, sentinel):
    buf = torch.full((t.numel() + 2 * GUARD,), sentinel, dtype=t.dtype)
    buf[GUARD : GUARD + t.numel()] = t.reshape(-1)
    return buf.cuda()


def test_cases_cover_what_they_claim():
    """On the CPU: at least a fifth of the rows stop and at least a fifth do not; the named situations occur."""
    cases = _cases()
    assert len(cases) * ROWS >= 200
    stop = live = crossing = 0
    for n, (out, step, fin, tab) in enumerate(cases):
        want = stopping.reference_flags(out, step, fin, tab)
        stop += int(((want == 1) & (fin == 0)).sum())
        live += int((want == 0).sum())
        assert bool((want[fin == 1] == 1).all())
        if n == 0:
            assert torch.equal(want, fin)  # n_stops = 0 writes nothing, whatever the table holds
        if n >= 1 and min(_lengths(n)) >= 3:
            crossing += 1
            assert int(want[10]) == 0 and stopping.tail_matches(out.reshape(-1)[: 10 * CAP + 2].tolist(), [tab[9 + 9 * i : 9 + 9 * i + int(tab[8 + 9 * i])].tolist() for i in range(n)])
    total = len(cases) * ROWS
    assert stop * 5 >= total and live * 5 >= total, (stop, live, total)
    assert sorted({L for n in range(9) for L in _lengths(n)}) == list(range(1, 9))
    steps = {int(s) for c in cases for s in c[1]}
    assert {0, 1, CAP, CAP + 3} <= steps and crossing == 2


def test_finished_flags_equal_the_rule_and_nothing_else_is_written():
    lib = ops.load_library()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n, (out, step, fin, tab) in enumerate(_cases()):
        bufs = [_banded(out, S64), _banded(step, S32), _banded(fin, S32), _banded(tab, S32)]
        before = [b.clone() for b in bufs]
        ptr = [ctypes.c_void_p(b.data_ptr() + GUARD * b.element_size()) for b in bufs]
        assert lib.dl_decode_stop(ptr[0], CAP, ROWS, ptr[1], ptr[2], ptr[3], stream) == 0, lib.dl_last_error()
        torch.cuda.synchronize()
        want = stopping.reference_flags(out, step, fin, tab)
        got = bufs[2][GUARD : GUARD + ROWS].cpu()
        assert torch.equal(got, want), (n, got.tolist(), want.tolist())
        for k in (0, 1, 3):  # out_ids, step and the table, bands included
            assert torch.equal(bufs[k], before[k]), (n, k)
        assert torch.equal(bufs[2][:GUARD], before[2][:GUARD]) and torch.equal(bufs[2][GUARD + ROWS :], before[2][GUARD + ROWS :]), n


def test_wrapper_and_bad_arguments():
    out, step, fin, tab = (t.cuda() for t in _cases()[3])
    want = stopping.reference_flags(out, step, fin, tab)
    assert ops.decode_stop(out, step, fin, tab) is fin
    torch.cuda.synchronize()
    assert torch.equal(fin.cpu(), want)
    assert torch.equal(ops.decode_stop(out, step, fin, tab).cpu(), want)  # a second launch changes nothing: finished rows are not touched
    lib = ops.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    good = dict(out=p(out), cap=CAP, B=ROWS, step=p(step), fin=p(fin), tab=p(tab))
    for kw in (dict(out=None), dict(step=None), dict(fin=None), dict(tab=None), dict(B=0), dict(B=-1), dict(cap=0)):
        a = dict(good, **kw)
        assert lib.dl_decode_stop(a["out"], a["cap"], a["B"], a["step"], a["fin"], a["tab"], None) == -1, kw
    torch.cuda.synchronize()
    assert torch.equal(fin.cpu(), want)  # nothing was enqueued
