"""GPU: dl_decode_logprobs (through the C ABI) against the rule in dynamic_llava_amd/logprobs.py.

Tolerance.  Kernel and host rule see the same logits: the maximum, the order of the top-n list, the token's logit and both subtractions are exact in both, so the
two can differ only through their exponentials and logarithms -- the situation of dl_decode_score, and the same bound (score_cases.device_tol, derived there):

    tol = (2 * 2^-23 + V * 2^-40 + 2^-23) + 2 * ulp32(lse_ref) + ulp32(logprob_ref)

Everything that is an integer (the ids) and every comparison between two launch forms, between an entry of the list and the same token's own value, and with
dl_decode_score on the same logits is exact.  Every launch runs on sentinel-filled buffers and checks that only its own slots changed."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import score_cases as cs  # noqa: E402
from dynamic_llava_amd import logprobs as lpr  # noqa: E402

CAP, NMAX = 4, 8
S_LP, S_ID = -77.0, -9  # sentinels


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _row(V, dtype, name, seed):
    return dict(cs.families(V, dtype, seed=seed))[name]


@functools.lru_cache(maxsize=None)
def _ref(V, dtype, name, seed):
    """The rule on one row, once: (lse fp32, top_logprobs [8], top_ids [8], the logprob of each of the row's five tokens)."""
    row = _row(V, dtype, name, seed)
    five = cs.labels_for(row, seed=seed)
    lps, top_lp, top_ids = lpr.reference_row_tokens(row, five, NMAX)
    lse = -float(top_lp[0])  # entry 0 is the maximum: -((m - m) + lse)
    return lse, top_lp, top_ids, five, lps


def _batch(V, dtype, B, name):
    """[B, V]: row b is family `name` drawn with seed b; its token is one of (argmax, minimum, 0, V - 1, random), rotating with the row."""
    x = torch.stack([_row(V, dtype, name, b) for b in range(B)])
    which = [b % 5 for b in range(B)]
    toks = torch.tensor([_ref(V, dtype, name, b)[3][which[b]] for b in range(B)], dtype=torch.int64)
    return x, toks, which


def _launch(xd, toks, n, steps=None, cap=CAP, stride=NMAX):
    """One launch on sentinel-filled buffers; steps [B]: the step counters as the step-closing launch left them (default: row b fills slot b % cap).
    -> logprobs [B, cap], top_logprobs / top_ids [B, cap, stride] on the CPU."""
    from dynamic_llava_amd import hip_ops as ops

    B, dev = xd.shape[0], xd.device
    steps = [b % cap + 1 for b in range(B)] if steps is None else steps
    lp = torch.full((B, cap), S_LP, dtype=torch.float32, device=dev)
    top_lp = torch.full((B, cap, stride), S_LP, dtype=torch.float32, device=dev)
    top_ids = torch.full((B, cap, stride), S_ID, dtype=torch.int64, device=dev)
    ops.decode_logprobs(xd, toks.to(dev), torch.tensor(steps, dtype=torch.int32, device=dev), lp, n, top_lp, top_ids)
    torch.cuda.synchronize()
    return lp.cpu(), top_lp.cpu(), top_ids.cpu()


def _only_these_slots(out, n, steps, cap=CAP):
    """Slots other than step - 1, entries n.. of the written slot, and rows whose slot lies outside [0, cap) hold their sentinels."""
    lp, top_lp, top_ids = (t.clone() for t in out)
    for b, s in enumerate(steps):
        if 0 <= s - 1 < cap:
            lp[b, s - 1], top_lp[b, s - 1, :n], top_ids[b, s - 1, :n] = S_LP, S_LP, S_ID
    return bool((lp == S_LP).all()) and bool((top_lp == S_LP).all()) and bool((top_ids == S_ID).all())


def _close(got, ref, lse, V):
    if torch.isinf(ref):
        return bool(got == ref)
    return abs(float(got) - float(ref)) <= cs.device_tol(V, lse, float(ref))


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", [320, 32000, 32003, 65536])
def test_kernel_matches_the_rule(V, dtype):
    """Every family at B in {1, 3, 32} and n in {0, 1, 5, 8}: ids exact, every value within tol."""
    worst = 0.0
    for name in [n_ for n_, _ in cs.families(V, dtype)]:
        for B in (1, 3, 32):
            x, toks, which = _batch(V, dtype, B, name)
            xd = x.cuda()
            steps = [b % CAP + 1 for b in range(B)]
            for n in (0, 1, 5, 8):
                out = _launch(xd, toks, n)
                assert _only_these_slots(out, n, steps), (name, B, n)
                for b in range(B):
                    lse, top_lp, top_ids, _, lps = _ref(V, dtype, name, b)
                    s = steps[b] - 1
                    assert out[2][b, s, :n].tolist() == top_ids[:n].tolist(), (name, B, n, b)
                    pairs = [(out[0][b, s], lps[which[b]])] + [(out[1][b, s, k], top_lp[k]) for k in range(n)]
                    for k, (got, ref) in enumerate(pairs):
                        assert _close(got, ref, lse, V), (name, B, n, b, k, float(got), float(ref), cs.device_tol(V, lse, float(ref)))
                        if torch.isfinite(ref):
                            worst = max(worst, abs(float(got) - float(ref)) / cs.device_tol(V, lse, float(ref)))
    print(f"V={V} {dtype}: worst |kernel - rule| / tol = {worst:.3f}")


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", [320, 32000, 32003, 65536])
def test_same_bits_as_the_list_entry_and_as_the_scorer(V, dtype):
    """A token that is among the top-n: its `logprobs` value and its `top_logprobs` entry are the same bits.  Any token: `logprobs` is the bit-exact negative of
    the nll dl_decode_score writes for that token as the label on the same device logits."""
    from dynamic_llava_amd import hip_ops as ops

    B = 32
    for name in ("gauss6", "neginf", "equal"):
        x, toks, _ = _batch(V, dtype, B, name)
        xd = x.cuda()
        steps = [b % CAP + 1 for b in range(B)]
        first = _launch(xd, toks, NMAX)
        listed = torch.stack([first[2][b, steps[b] - 1, b % NMAX] for b in range(B)])  # entry b % 8 of row b's list
        for tk in (listed, toks):
            lp, top_lp, top_ids = _launch(xd, tk, NMAX)
            nll = torch.full((B, CAP), S_LP, dtype=torch.float32, device="cuda")
            labels = torch.full((B, CAP), -100, dtype=torch.int64, device="cuda")
            st = torch.tensor([s - 1 for s in steps], dtype=torch.int32, device="cuda")  # the scorer fills slot step, this kernel slot step - 1
            labels[torch.arange(B, device="cuda"), st.long()] = tk.cuda()
            ops.decode_score(xd, torch.zeros(B, dtype=torch.int64, device="cuda"), labels, nll, None, None, st)
            torch.cuda.synchronize()
            for b in range(B):
                s = steps[b] - 1
                assert torch.equal(_bits(lp[b, s]), _bits(-nll.cpu()[b, s])), (name, b, float(lp[b, s]), float(nll[b, s]))
                where = (top_ids[b, s] == tk[b]).nonzero()
                if tk is listed:
                    assert where.numel() == 1 and int(where) == b % NMAX, (name, b)
                for k in where.flatten().tolist():
                    assert torch.equal(_bits(lp[b, s]), _bits(top_lp[b, s, k])), (name, b, k)


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", [320, 32000, 32003, 65536])
def test_same_bits_whatever_the_launch_form(V, dtype):
    """Row b of a 32-row launch, its own 1-row launch, a launch on an odd row stride, one on a base pointer one element off a 16-byte boundary (both scalar-load
    routes) and a second run: the same bits."""
    B = 32
    same = lambda a, b: torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(a[2], b[2])
    for name in ("gauss6", "neginf"):
        x, toks, _ = _batch(V, dtype, B, name)
        xd = x.cuda()
        steps = [b % CAP + 1 for b in range(B)]
        full = _launch(xd, toks, NMAX)
        assert same(_launch(xd, toks, NMAX), full), name
        for b in range(B):
            one = _launch(xd[b : b + 1], toks[b : b + 1], NMAX, steps=[steps[b]])
            assert same([t[0] for t in one], [t[b] for t in full]), (name, b)
        wide = torch.zeros((B, V + 1), dtype=dtype, device="cuda")
        wide[:, :V] = xd
        strided = wide[:, :V]
        assert strided.stride(0) == V + 1
        assert same(_launch(strided, toks, NMAX), full), name
        flat = torch.zeros(B * V + 1, dtype=dtype, device="cuda")
        off = flat[1:].view(B, V)
        off.copy_(xd)
        assert off.data_ptr() % 16 != 0
        assert same(_launch(off, toks, NMAX), full), name
        for n in (0, 1, 5):  # fewer alternatives: a prefix of the same list, the same token value
            part = _launch(xd, toks, n)
            assert torch.equal(_bits(part[0]), _bits(full[0])) and _only_these_slots(part, n, steps)
            for b in range(B):
                assert torch.equal(_bits(part[1][b, steps[b] - 1, :n]), _bits(full[1][b, steps[b] - 1, :n])) and torch.equal(part[2][b, steps[b] - 1, :n], full[2][b, steps[b] - 1, :n])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_guard_bands(dtype):
    """step = 0 (nothing committed yet), step > cap and a negative step write nothing; a token outside [0, V) writes 0.0 and still the list; a narrow top buffer
    (stride 5) keeps its rows apart; the words around the three buffers stay intact."""
    from dynamic_llava_amd import hip_ops as ops

    V, B, cap, stride, n, G = 32003, 6, 3, 5, 5, 64
    x = torch.stack([_row(V, dtype, "gauss6", b) for b in range(B)])
    xd = x.cuda()
    steps = [0, cap + 1, 1, cap, -2, 2]
    toks = torch.tensor([5, 5, V, 7, 5, -1], dtype=torch.int64)

    def banded(fill, dt, per):
        buf = torch.full((G + B * cap * per + G,), fill, dtype=dt, device="cuda")
        return buf, buf[G : G + B * cap * per]

    lp_buf, lp = banded(S_LP, torch.float32, 1)
    tl_buf, top_lp = banded(S_LP, torch.float32, stride)
    ti_buf, top_ids = banded(S_ID, torch.int64, stride)
    lp, top_lp, top_ids = lp.view(B, cap), top_lp.view(B, cap, stride), top_ids.view(B, cap, stride)
    ops.decode_logprobs(xd, toks.cuda(), torch.tensor(steps, dtype=torch.int32, device="cuda"), lp, n, top_lp, top_ids)
    torch.cuda.synchronize()
    out = (lp.cpu(), top_lp.cpu(), top_ids.cpu())
    assert _only_these_slots(out, n, steps, cap=cap)
    for buf, fill in ((lp_buf, S_LP), (tl_buf, S_LP), (ti_buf, S_ID)):
        assert bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())
    for b in (2, 3, 5):
        s = steps[b] - 1
        ref_lp, ref_top, ref_ids = lpr.reference_row(x[b], int(toks[b]), n)
        lse = -float(ref_top[0])
        assert out[2][b, s].tolist() == ref_ids.tolist()
        assert all(_close(out[1][b, s, k], ref_top[k], lse, V) for k in range(n))
        if b == 3:
            assert _close(out[0][b, s], ref_lp, lse, V) and float(out[0][b, s]) < 0.0
        else:
            assert float(out[0][b, s]) == 0.0 and float(ref_lp) == 0.0  # the token is no index of the row


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", [320, 32003, 65536])
def test_tie_heavy_rows(V, dtype):
    """All logits equal: the list is 0 .. n - 1 in order, every value the same bits.  Two values alternating (the larger one at the odd indices): 1, 3, 5, ...;
    at V = 320 with only three entries at the larger value the list continues with the smaller one's 0, 2, 4, ..."""
    equal = torch.full((V,), -2.5).to(dtype)
    alt = torch.tensor([0.25, 1.5]).repeat(V // 2 + 1)[:V].to(dtype)
    three = torch.full((V,), 0.25)
    three[[1, 3, 5]] = 1.5
    x = torch.stack([equal, alt, three.to(dtype)])
    lp, top_lp, top_ids = _launch(x.cuda(), torch.tensor([V - 1, 0, 2]), NMAX, steps=[1, 1, 1])
    assert top_ids[0, 0].tolist() == list(range(8)) and top_ids[1, 0].tolist() == list(range(1, 16, 2)) and top_ids[2, 0].tolist() == [1, 3, 5, 0, 2, 4, 6, 7]
    assert torch.equal(_bits(top_lp[0, 0]), _bits(lp[0, 0].repeat(8)))
    for b in range(3):
        ref_lp, ref_top, ref_ids = lpr.reference_row(x[b], [V - 1, 0, 2][b], NMAX)
        lse = -float(ref_top[0])
        assert top_ids[b, 0].tolist() == ref_ids.tolist()
        assert _close(lp[b, 0], ref_lp, lse, V) and all(_close(top_lp[b, 0, k], ref_top[k], lse, V) for k in range(NMAX))
    assert len(set(_bits(top_lp[1, 0]).tolist())) == 1 and torch.equal(_bits(top_lp[2, 0, 3:]), _bits(lp[2, 0].repeat(5)))


def test_argument_rejection():
    """Return codes, not faults: the checks come before any launch."""
    from dynamic_llava_amd import hip_ops

    lib = hip_ops.load_library()
    p = ctypes.c_void_p(16)  # never dereferenced
    args = lambda V=32000, n=0, stride=8, top=p, lp=p: (p, hip_ops.DL_BF16, V, V, 1, p, p, 4, lp, n, stride, top, top, None)
    assert lib.dl_decode_logprobs(*args(V=65537)) != 0 and b"65536" in lib.dl_last_error()
    for kw in (dict(n=9), dict(n=-1), dict(V=4, n=5), dict(n=6, stride=5), dict(n=1, top=None), dict(lp=None)):
        assert lib.dl_decode_logprobs(*args(**kw)) != 0, kw
    x, ids, st = torch.zeros((1, 320), device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(hip_ops.HipOpsError):
        hip_ops.decode_logprobs(x, ids, st, torch.zeros((1, 4), device="cuda"), 2)  # alternatives without their buffers
    with pytest.raises(hip_ops.HipOpsError):
        hip_ops.decode_logprobs(x, ids, st, None)
