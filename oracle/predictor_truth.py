"""Truth and the acceptance criterion for the code that takes the model's discrete decisions: the text predictor (csrc/tp_body.h, three launches or extra
workgroups of dl_gemv_gu_tp), the small kernels of the vision predictor (csrc/predictors.hip: vp_build_index, vp_pool_concat, vp_head) and the greedy
advance (dl_decode_advance: csrc/advance.hip, closing the step by csrc/step_close.h).  docs/predictor_exactness.md has the construction, the mutant table and the measured figures.

Every stage is judged from the kernel's OWN previous intermediate (h1 / a1 in the caller's workspace, the vision predictor's workspace regions), so the error
of one stage never widens the set of the next.

  dense stage   out = RNE_T(gelu(RNE_T(dot + b)))  (the last layer: RNE_T(dot + b)).  The fp32 pre-activation of a K-term dot product accumulated in ANY order,
                with or without fma, lies within (K + 8) 2^-24 sum|w x| of the fp64 value (the bias counts as one more term; the +8 covers the add of the
                bias and the second-order terms for K <= 2^16).  The two ends of that interval are rounded to T (monotone); GELU maps the interval between
                them onto [min, max] of its values at the ends, and at its minimum (x = -0.7518) when the interval straddles it, widened by gelu_truth's
                bound; the ends of that are rounded to T.  Lattice inputs: every partial sum is an integer below 2^24, the pre-activation is exact.
  stage 1       reads LN(x) rounded to T out of LDS, which nobody can observe: the interval of every xs_k is ln_truth's, the pre-activation interval the
                interval product with w.
  pool_concat   local half: a copy.  global half: RNE_T(RNE_T(tot) / RNE_T(n)), tot within (n + 8) 2^-24 sum|x| of the fp64 sum; the division is one fp32
                operation of two T values, monotone in tot.
  score         (l0 - m) - log(exp(l0 - m) + exp(l1 - m)), m = max(l0, l1), on the kernel's own logits: within RHO_SCORE (1 + |s|) of fp64 (an absolute
                term: for l0 >> l1 the score is -exp(l1 - l0), far below one fp32 ulp of the 1 + exp(..) it is computed from).
  decision      == (l0 > l1) on the kernel's own logits, always; against truth where the feasible sets of the two logits are disjoint.
  advance       a plain restatement (advance_ref), bit for bit."""
from __future__ import annotations

import math

import torch

from oracle import linear_truth as lt
from oracle import rowwise_truth as rt

BF16, F16, F32 = rt.BF16, rt.F16, rt.F32
U32, TINY32 = rt.U32, rt.TINY32
EPS = 1e-5
LIMIT = lt.LIMIT
# measured on the CPU (docs/predictor_exactness.md, "Measured"; tests/test_predictor_truth_cpu.py re-derives it): 4 x the largest
# |fp32 - fp64| / (1 + |s|) of torch's fp32 score expression over every pair of a 2048-point grid of 16-bit logits, rounded up to two digits
RHO_SCORE = 4.3e-7  # 4 x 1.06e-7 (fp16 grid)
SLACK = 8  # the "+ 8" of the accumulation bound


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_argmin():
    """The minimiser of x Phi(x): Phi(x) + x phi(x) = 0, by bisection."""
    f = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0))) + x * math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    a, b = -1.0, -0.5
    for _ in range(80):
        m = 0.5 * (a + b)
        a, b = (m, b) if f(m) < 0 else (a, m)
    return 0.5 * (a + b)


GELU_XMIN = _gelu_argmin()  # -0.75179...
GELU_MIN = float(_gelu64(torch.tensor(GELU_XMIN, dtype=torch.float64)))


class PremiseError(AssertionError):
    """The input handed to an `exact` stage is not on the lattice (the kernel's previous intermediate is already wrong)."""


class StageSet(rt.Feasible):
    """A feasible set for an output the kernel keeps as fp32 (h1, a1, the logits) or as T: 16-bit T additionally demands that the value IS a T value (an
    unrounded fp32 number between two neighbours is outside)."""

    def ok(self, out):
        out = out.detach().cpu()
        if self.lo is None:
            return (out.double() - self.v).abs() <= self.e
        o = out.double()
        hit = (o >= self.lo.double()) & (o <= self.hi.double()) if self.between else ((o == self.lo.double()) | (o == self.hi.double()))
        return hit & (out.to(self.dtype).double() == o)

    def rows(self, idx):
        pick = lambda t: None if t is None else t[idx]
        return StageSet(self.dtype, pick(self.lo), pick(self.hi), pick(self.v), pick(self.e), self.between)


def _ends(lo64, hi64, dtype, exact=False):
    if dtype == F32:
        v = 0.5 * (lo64 + hi64)
        return StageSet(dtype, v=v, e=0.5 * (hi64 - lo64) + (0.0 if exact else v.abs() * U32 + TINY32))  # exact: integers, no rounding anywhere: e = 0
    return StageSet(dtype, lo=rt.to_t(lo64, dtype), hi=rt.to_t(hi64, dtype), between=True)


def pre_interval(x, w, b, exact=False, x_lo=None, x_hi=None):
    """-> (lo, hi) fp64 [B, N]: where the fp32 pre-activation can lie.  x [B, K] fp64 (T values) or the interval x_lo / x_hi per element."""
    W = w.double()
    bd = torch.zeros(W.shape[0], dtype=torch.float64) if b is None else b.double()
    K = W.shape[1]
    if x_lo is None:
        lo = hi = x @ W.T + bd
        S = x.abs() @ W.abs().T + bd.abs()
    else:
        Wp, Wn = W.clamp(min=0), W.clamp(max=0)
        lo = x_lo @ Wp.T + x_hi @ Wn.T + bd
        hi = x_hi @ Wp.T + x_lo @ Wn.T + bd
        S = torch.maximum(x_lo.abs(), x_hi.abs()) @ W.abs().T + bd.abs()
    e = torch.zeros_like(S) if exact else (K + SLACK) * U32 * S
    return lo - e, hi + e


def dense_truth(x, w, b, dtype, gelu=True, exact=False, x_lo=None, x_hi=None) -> StageSet:
    lo, hi = pre_interval(x, w, b, exact, x_lo, x_hi)
    if dtype != F32:
        lo, hi = rt.to_t(lo, dtype).double(), rt.to_t(hi, dtype).double()
    if not gelu:
        return _ends(lo, hi, dtype, exact)
    if exact:  # lattice: the pre-activation is 0 or an integer k >= 8, and fp32 gelu_erf(k) == k (asserted by lattice_layer): the output is that integer
        if not bool(((lo == hi) & ((lo == 0) | (lo >= 8)) & (lo == lo.round())).all()):
            raise PremiseError("an exact stage needs integer pre-activations that are 0 or >= 8")
        return _ends(lo, hi, dtype, True)
    g0, g1 = _gelu64(lo), _gelu64(hi)
    straddle = (lo < GELU_XMIN) & (hi > GELU_XMIN)
    glo = torch.where(straddle, torch.full_like(g0, GELU_MIN), torch.minimum(g0, g1))
    ghi = torch.maximum(g0, g1)
    eg = rt.GELU_ABS * torch.maximum(lo.abs(), hi.abs()) + torch.maximum(g0.abs(), g1.abs()) * U32 + TINY32
    return _ends(glo - eg, ghi + eg, dtype)


def ln_interval(x, ln_w, ln_b, cls):
    """x [B, H] model dtype -> (lo, hi) fp64 of RNE_T(LN(x)) per element (rowwise_truth.ln_truth)."""
    F = rt.ln_truth(x, ln_w, ln_b, EPS, rt.RHO_LATTICE if cls == "lattice" else rt.RHO_GENERIC, exact_mean=cls == "lattice")
    if F.lo is None:
        return F.v - F.e, F.v + F.e
    return F.lo.double(), F.hi.double()


def stage1_truth(x, ln_w, ln_b, w1, b1, cls, exact=False) -> StageSet:
    if exact:  # the lattice LN output is one value per element (asserted against ln_truth)
        return dense_truth(lattice_ln_out(x, ln_w, ln_b), w1, b1, x.dtype, True, True)
    lo, hi = ln_interval(x, ln_w, ln_b, cls)
    return dense_truth(None, w1, b1, x.dtype, True, exact, lo, hi)


def pool_truth(hs, exact=False) -> StageSet:
    """hs [B, n, C] model dtype -> the set of z [B, n, C]."""
    dt = hs.dtype
    B, n, C = hs.shape
    half = C // 2
    g = hs[:, :, half:].double()
    tot, S = g.sum(1), g.abs().sum(1)
    e = torch.zeros_like(S) if exact else (n + SLACK) * U32 * S
    n_t = torch.tensor(float(n), dtype=torch.float64).to(F32).to(dt)
    if dt == F32:
        v = tot / float(n)
        gm = StageSet(dt, v=v, e=e / float(n) + v.abs() * 2 * U32 + TINY32)
        loc = hs[:, :, :half].double()
        full = lambda a, fill: torch.cat([fill, a[:, None, :].expand(B, n, half)], 2)
        return StageSet(dt, v=full(gm.v, loc), e=full(gm.e, torch.zeros_like(loc)))
    ends = [(rt.to_t(t, dt).float() / n_t.float()).to(dt) for t in (tot - e, tot + e)]
    full = lambda a: torch.cat([hs[:, :, :half], a[:, None, :].expand(B, n, half)], 2)
    return StageSet(dt, lo=full(torch.minimum(*ends)), hi=full(torch.maximum(*ends)), between=True)


def score64(l0, l1):
    m = torch.maximum(l0, l1)
    return (l0 - m) - torch.log(torch.exp(l0 - m) + torch.exp(l1 - m))


def score_fp32(l0, l1):
    """The kernel's expression in torch's fp32."""
    m = torch.maximum(l0, l1)
    return (l0 - m) - torch.log(torch.exp(l0 - m) + torch.exp(l1 - m))


def score_truth(logits, rho=None) -> StageSet:
    """logits [..., 2] model dtype (the kernel's own) -> the set of score [...]."""
    rho = RHO_SCORE if rho is None else rho
    dt = logits.dtype
    s = score64(logits[..., 0].double(), logits[..., 1].double())
    e = rho * (1.0 + s.abs())
    if dt == F32:
        return StageSet(dt, v=s, e=e + TINY32)
    return StageSet(dt, lo=rt.to_t(s - e, dt), hi=rt.to_t(s + e, dt), between=True)


def score_grid(dtype, n=2048):
    """n finite values of a 16-bit dtype spread over its bit patterns with |v| <= 2^14 (logits), both signs, plus 0 and the neighbours of +-1."""
    v = rt.all_values(dtype).float()
    v = v[torch.isfinite(v) & (v.abs() <= 2.0**14)]
    idx = torch.linspace(0, v.numel() - 1, n - 5).round().long()
    one = torch.ones((), dtype=dtype)
    extra = torch.tensor([0.0, 1.0, -1.0, float(one + torch.finfo(dtype).eps), float(-one - torch.finfo(dtype).eps)])
    return torch.cat([v[idx], extra])


def measure_rho_score(dtype, n=2048):
    """Largest |fp32 - fp64| / (1 + |s|) of score_fp32 over every pair of score_grid(dtype)."""
    g = score_grid(dtype, n)
    l0, l1 = g[:, None].expand(-1, g.numel()), g[None, :].expand(g.numel(), -1)
    s32, s64 = score_fp32(l0, l1).double(), score64(l0.double(), l1.double())
    return float(((s32 - s64).abs() / (1.0 + s64.abs())).max())


def decision_truth(F0: StageSet, F1: StageSet):
    """-> (determined bool [B], decision int [B]): where the feasible sets of the two logits are disjoint, l0 > l1 is decided."""
    if F0.lo is None:
        lo0, hi0, lo1, hi1 = F0.v - F0.e, F0.v + F0.e, F1.v - F1.e, F1.v + F1.e
    else:
        lo0, hi0, lo1, hi1 = F0.lo.double(), F0.hi.double(), F1.lo.double(), F1.hi.double()
    keep, evict = lo0 > hi1, hi0 <= lo1
    return keep | evict, keep.int()


# ------------------------------------------------------------------------------------------------------------------------------
# lattice weights: sparse integers, every pre-activation 0 or an integer in [8, LIMIT]
# ------------------------------------------------------------------------------------------------------------------------------
def stage1_priority(K, V):
    """Columns a sparse stage-1 weight occupies first: the two ends, the last 16-byte chunk, both sides of every 64-chunk lane pass (the kTp1MaxChunks
    boundary among them) and of every 256-vector pass of the LayerNorm loop."""
    seen, order = set(), []
    def add(k):
        if 0 <= k < K and k not in seen:
            seen.add(k)
            order.append(k)
    for k in (0, K - 1, K - V, V - 1, V):
        add(k)
    for step in (64 * V, 256 * V):
        for c in range(step, K, step):
            add(c - 1)
            add(c)
    for c in range(0, K, max(V, K // 64 // V * V)):
        add(c + 1)
    return order


def lattice_layer(xin, N, dtype, seed, nnz=4, priority=None, dead_every=7, gelu=True, limit=None):
    """xin [B, K] fp64 integers (the exact input of the layer) -> (w [N, K], b [N]) model dtype, out [B, N] fp64: the exact output.
    Neuron n takes up to `nnz` columns (from `priority`, cycled, so that every priority column meets a weight; else a permutation of all columns) with weights
    in +-{1, 2, 3}, and the bias that puts its smallest pre-activation over the rows at 8..15; columns, weights and that offset shrink until the largest
    stays within the limit.  Every dead_every-th neuron is all zero (pre-activation 0).  The premises are asserted."""
    g = torch.Generator().manual_seed(seed)
    B, K = xin.shape
    limit = LIMIT[dtype] if limit is None else min(limit, LIMIT[dtype])
    seq = [int(k) for k in torch.randperm(K, generator=g).tolist()] if priority is None else list(priority)
    w = torch.zeros(N, K, dtype=torch.float64)
    b = torch.zeros(N, dtype=torch.float64)
    pos = 0
    for n in range(N):
        if dead_every and n % dead_every == dead_every - 1:
            continue
        cols = list(dict.fromkeys(seq[(pos + j) % len(seq)] for j in range(nnz)))
        pos += nnz
        vals = torch.randint(1, 4, (len(cols),), generator=g).double() * (torch.randint(0, 2, (len(cols),), generator=g).double() * 2 - 1)
        base = 8 + int(torch.randint(0, 8, (1,), generator=g))
        lim = limit
        while True:
            s = xin[:, cols] @ vals
            bias = base - float(s.min())
            if float(s.max()) + bias <= lim and abs(bias) <= LIMIT[dtype]:
                break
            if len(cols) > 1:
                cols, vals = cols[:-1], vals[:-1]
            elif float(vals.abs().max()) > 1:
                vals = vals.sign()
            elif base > 8:
                base = 8
            elif float(vals[0]) < 0:
                vals = -vals
            else:
                assert lim < LIMIT[dtype], "a single column already leaves the lattice"
                lim = LIMIT[dtype]
        w[n, cols] = vals
        b[n] = bias
    pre = xin @ w.T + b
    assert bool(((pre == 0) | ((pre >= 8) & (pre <= LIMIT[dtype]))).all()) and torch.equal(pre, pre.round()), "pre-activations must be 0 or integers in [8, LIMIT]"
    assert float((xin.abs() @ w.abs().T + b.abs()).max()) < 2**24, "partial sums must be exact in fp32"
    assert torch.equal(w.to(dtype).double(), w) and torch.equal(b.to(dtype).double(), b)
    if gelu:  # fp32 gelu_erf(k) == k for integers k >= 6 and gelu(0) == 0 (asserted on torch's fp32 erf; the GPU test shows the kernel's)
        assert torch.equal(torch.nn.functional.gelu(pre.float()).double(), pre)
    return w.to(dtype), b.to(dtype), pre


def lattice_rows(H, B, dtype, seed, hot):
    """[B, H] model dtype.  Row 0 (and every row for fp32): a constant row, for which x - mean is exactly 0 and LN(x) = ln_b.  The others (16-bit): balanced
    +-1, mean 0 and variance 1 exactly, so that RNE_T(+-k rsqrt(1 + 1e-5) + b) = +-k + b for the integer ln_w = k, ln_b = b."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for r in range(B):
        if dtype == F32 or r % 3 == 0:
            rows.append(torch.full((H,), float(1 + r % 5), dtype=torch.float64))
            continue
        s = torch.cat([torch.ones(H // 2), -torch.ones(H - H // 2)]).double()[torch.randperm(H, generator=g)]
        rows.append(s)
    x = torch.stack(rows)
    assert H % 2 == 0
    return x.to(dtype)


def lattice_ln(H, dtype, seed, hot):
    """Integer ln_w (3..6 on the hot columns, up to 128 elsewhere) and ln_b in -2..2 (|ln_w| > |ln_b|: +-k + b is never 0, where LN would leave -k 5e-6)."""
    g = torch.Generator().manual_seed(seed + 50)
    w = torch.randint(3, 129, (H,), generator=g).double()
    w[hot] = torch.randint(3, 7, (len(hot),), generator=g).double()
    b = torch.randint(-2, 3, (H,), generator=g).double()
    return w.to(dtype), b.to(dtype)


def lattice_ln_out(x, ln_w, ln_b):
    """The exact LN output of lattice_rows under lattice_ln, asserted against ln_truth (both ends equal it)."""
    xd = x.double()
    const = (xd == xd[:, :1]).all(1, keepdim=True)
    xs = torch.where(const, ln_b.double()[None, :].expand_as(xd), xd * ln_w.double() + ln_b.double())
    lo, hi = ln_interval(x, ln_w, ln_b, "lattice")
    if x.dtype == F32:
        assert bool(((xs >= lo) & (xs <= hi) & (hi - lo <= 8 * U32 * xs.abs() + 1e-30)).all())
    else:
        assert torch.equal(lo, xs) and torch.equal(hi, xs), "the lattice LN output must be decided"
    return xs


# ------------------------------------------------------------------------------------------------------------------------------
# the greedy advance, restated
# ------------------------------------------------------------------------------------------------------------------------------
def advance_ref(logits, step=None, finished=None, out_ids=None, eos=(-1, -1, -1), pad_id=0, kv_full=None, kv_sparse=None, decision=None, min_new_tokens=0):
    """logits [B, V] (any float dtype, CPU).  -> dict of the tensors after the call (inputs are not modified).
    The token of a row is the lowest index among the maxima of its candidates, a candidate being an index that is not banned and whose logit is not NaN (a NaN
    compares false with everything, so it is never selected); a row without candidates yields 0.  The EOS ids are banned while step < min_new_tokens.
    eos[1], eos[2] count only when eos[0] >= 0."""
    B, V = logits.shape
    x = logits.float()
    e0 = int(eos[0])
    eset = [int(e) for e in eos] if e0 >= 0 else [-1, -1, -1]
    nxt = torch.zeros(B, dtype=torch.int64)
    out = {k: (None if t is None else t.clone()) for k, t in dict(step=step, finished=finished, out_ids=out_ids, kv_full=kv_full, kv_sparse=kv_sparse).items()}
    for b in range(B):
        st = int(step[b]) if step is not None else 0
        ban = e0 >= 0 and min_new_tokens > 0 and st < min_new_tokens
        cand = ~torch.isnan(x[b])
        if ban:
            for e in eset:
                if 0 <= e < V:
                    cand[e] = False
        if bool(cand.any()):
            vals = torch.where(cand, x[b], torch.full_like(x[b], float("-inf")))
            tok = int(torch.nonzero(cand & (vals == vals.max()))[0])
        else:
            tok = 0
        if finished is not None:
            if int(finished[b]):
                tok = pad_id
            elif e0 >= 0 and tok in eset:
                out["finished"][b] = 1
        nxt[b] = tok
        if out_ids is not None and step is not None:
            if st < out_ids.shape[1]:
                out["out_ids"][b, st] = tok
            out["step"][b] = st + 1
        if kv_full is not None:
            out["kv_full"][b] = int(kv_full[b]) + 1
        if kv_sparse is not None:
            out["kv_sparse"][b] = int(kv_sparse[b]) + (int(decision[b]) if decision is not None else 1)
    out["next_ids"] = nxt
    return out


ADVANCE_MUTANTS = ("highest_index_on_ties", "tail_skipped", "second_trip_skipped", "banned_id_wins", "write_at_out_cap")


def emulate_advance(logits, step, finished, out_ids, eos, pad_id, kv_full, kv_sparse, decision, min_new_tokens, vec_ok=True, mutant=None):
    """The kernel's structure (16-byte chunks dealt to 1024 threads, four per thread and trip, then the scalar tail) on the CPU, with one step altered.
    out_ids is emulated as the flat buffer the kernel indexes, one spare slot behind it."""
    B, V = logits.shape
    VE = rt.VEC[logits.dtype]
    x = logits.float()
    n_chunks = V // VE
    seen = torch.ones(V, dtype=torch.bool)
    if vec_ok:
        if mutant == "tail_skipped":
            seen[n_chunks * VE :] = False
        if mutant == "second_trip_skipped":
            seen[TRIP_CHUNKS * VE : n_chunks * VE] = False
    e0 = int(eos[0])
    eset = [int(e) for e in eos] if e0 >= 0 else [-1, -1, -1]
    cap = out_ids.shape[1]
    flat = torch.cat([out_ids.reshape(-1).clone(), torch.full((1,), -7, dtype=out_ids.dtype)])
    res = dict(step=step.clone(), finished=finished.clone(), kv_full=kv_full.clone(), kv_sparse=kv_sparse.clone(), next_ids=torch.zeros(B, dtype=torch.int64))
    for b in range(B):
        st = int(step[b])
        ban = e0 >= 0 and min_new_tokens > 0 and st < min_new_tokens and mutant != "banned_id_wins"
        cand = ~torch.isnan(x[b]) & seen
        if ban:
            for e in eset:
                if 0 <= e < V:
                    cand[e] = False
        tok = 0
        if bool(cand.any()):
            vals = torch.where(cand, x[b], torch.full_like(x[b], float("-inf")))
            hits = torch.nonzero(cand & (vals == vals.max()))
            tok = int(hits[-1] if mutant == "highest_index_on_ties" else hits[0])
        if int(finished[b]):
            tok = pad_id
        elif e0 >= 0 and tok in eset:
            res["finished"][b] = 1
        res["next_ids"][b] = tok
        if st < cap or (mutant == "write_at_out_cap" and st == cap):
            flat[b * cap + st] = tok
        res["step"][b] = st + 1
        res["kv_full"][b] = int(kv_full[b]) + 1
        res["kv_sparse"][b] = int(kv_sparse[b]) + int(decision[b])
    res["out_ids"] = flat[:-1].view(B, cap)
    res["spare"] = flat[-1:]
    return res


# ------------------------------------------------------------------------------------------------------------------------------
# the documented arithmetic in fp32, two summation orders, with the mutants
# ------------------------------------------------------------------------------------------------------------------------------
TP_MUTANTS = ("last_chunk_dropped", "neighbour_bias", "no_rounding_before_gelu", "ln_eps_lost", "ln_row_at_stride_h", "pass_reuses_weights", "decision_ge")
POOL_MUTANTS = ("unrounded_n", "unrounded_tot", "tokens_past_16_dropped")
HEAD_MUTANTS = ("score_from_unrounded_logits",)
INDEX_MUTANTS = ("img_start_of_row0",)
# restated thresholds; tests/test_predictor_truth_cpu.py asserts each against the value predictor_cases.branches_in_sources parses out of csrc/
K_TP1_MAX_CHUNKS = 10    # csrc/tp_body.h kTp1MaxChunks
TRIP_CHUNKS = 4 * 1024   # 16-byte chunks a trip of decode_advance_kernel's loop takes
FUSED_MAXC = (8, 10)     # gemv_gu_tp_kernel's two instantiations: MAXC = 8 while H / kVec <= 64 * 8


def _dot32(x32, w32, order):
    """x32 [B, K] @ w32 [N, K]^T in fp32: order 0 torch's matmul; order 1: 64 strided lanes of 8-element vectors accumulated in sequence, then a pairwise tree."""
    if order == 0:
        return x32 @ w32.T
    B, K = x32.shape
    pad = (-K) % 512
    xp = torch.cat([x32, torch.zeros(B, pad)], 1).view(B, -1, 64, 8)
    wp = torch.cat([w32, torch.zeros(w32.shape[0], pad)], 1).view(w32.shape[0], -1, 64, 8)
    lanes = torch.zeros(B, w32.shape[0], 64)
    for c in range(xp.shape[1]):
        for e in range(8):
            lanes = lanes + xp[:, None, c, :, e] * wp[None, :, c, :, e]
    while lanes.shape[-1] > 1:
        lanes = lanes[..., 0::2] + lanes[..., 1::2]
    return lanes[..., 0]


def _rt(t32, dt):
    return t32.to(dt).float()


def emulate_dense(x32, w, b, dt, gelu=True, order=0, mutant=None):
    w32, b32 = w.float(), b.float()
    if mutant == "neighbour_bias":
        b32 = b32[torch.arange(b32.numel()) ^ 1] if b32.numel() % 2 == 0 else b32.roll(1)
    if mutant == "pass_reuses_weights" and w32.shape[0] > 32:  # stage 2b, 8 waves x 4 neurons a pass: pass 1 computes with pass 0's rows
        w32 = w32.clone()
        w32[32:64] = w32[0:32]
    pre = _dot32(x32, w32, order) + b32
    if not gelu:
        return _rt(pre, dt)
    if mutant == "no_rounding_before_gelu":
        return _rt(torch.nn.functional.gelu(pre), dt)
    return _rt(torch.nn.functional.gelu(_rt(pre, dt)), dt)


def emulate_tp(x, x_stride_rows, W, order=0, mutant=None):
    """x: the buffer [B, stride] whose first H columns are the rows (stride >= H); W: dict ln_w ln_b l1_w l1_b .. l7_w l7_b (model dtype).
    -> dict h1, a1, a2, logits (fp32 tensors of T values), decision."""
    dt = W["l1_w"].dtype
    H = W["ln_w"].numel()
    B = x.shape[0]
    if mutant == "ln_row_at_stride_h":
        rows = x.reshape(-1)[: B * x.shape[1]]
        xr = torch.stack([rows[r * H : r * H + H] for r in range(B)])
    else:
        xr = x[:, :H]
    x32 = xr.float()
    mean = rt.fp32_sum_orders(x32)[order] / float(H)
    d = x32 - mean
    var = rt.fp32_sum_orders(d * d)[order] / float(H)
    r = torch.rsqrt(var) if mutant == "ln_eps_lost" else torch.rsqrt(var + EPS)
    xs = _rt(d * r * W["ln_w"].float() + W["ln_b"].float(), dt)
    w1 = W["l1_w"]
    if mutant == "last_chunk_dropped":  # the register prefetch taken although the row has more than 64 * kTp1MaxChunks vectors
        V = rt.VEC[dt]
        xs = xs.clone()
        xs[:, 64 * K_TP1_MAX_CHUNKS * V :] = 0.0
    m1 = mutant if mutant in ("neighbour_bias", "no_rounding_before_gelu") else None
    h1 = emulate_dense(xs, w1, W["l1_b"], dt, True, order, m1)
    a1 = emulate_dense(h1, W["l3_w"], W["l3_b"], dt, True, order, m1)
    a2 = emulate_dense(a1, W["l5_w"], W["l5_b"], dt, True, order, mutant if mutant in ("neighbour_bias", "no_rounding_before_gelu", "pass_reuses_weights") else None)
    lg = emulate_dense(a2, W["l7_w"], W["l7_b"], dt, False, order, "neighbour_bias" if mutant == "neighbour_bias" else None)
    dec = (lg[:, 0] >= lg[:, 1]) if mutant == "decision_ge" else (lg[:, 0] > lg[:, 1])
    return dict(h1=h1, a1=a1, a2=a2, logits=lg, decision=dec.int())


def emulate_pool(hs, order=0, mutant=None):
    dt = hs.dtype
    B, n, C = hs.shape
    half = C // 2
    g = hs[:, :, half:].float()
    if mutant == "tokens_past_16_dropped":
        g = g[:, : 16 * (n // 16)]
    if order == 0:
        tot = g.sum(1)
    else:  # 16 token groups in sequence, then the groups in sequence (the kernel's own shape; order 0 is torch's)
        pad = (-g.shape[1]) % 16
        gp = torch.cat([g, torch.zeros(B, pad, half)], 1).view(B, -1, 16, half)
        part = torch.zeros(B, 16, half)
        for i in range(gp.shape[1]):
            part = part + gp[:, i]
        tot = torch.zeros(B, half)
        for k in range(16):
            tot = tot + part[:, k]
    den = float(n) if mutant == "unrounded_n" else float(torch.tensor(float(n)).to(dt))
    num = tot if mutant == "unrounded_tot" else _rt(tot, dt)
    gm = (num / den).to(dt)
    return torch.cat([hs[:, :, :half], gm[:, None, :].expand(B, n, half)], 2)


def emulate_head(z2, w, b, order=0, mutant=None):
    """-> (logits [M, 2], score [M]) model dtype."""
    dt = z2.dtype
    pre = _dot32(z2.float(), w.float(), order) + b.float()
    lg = _rt(pre, dt)
    src = pre if mutant == "score_from_unrounded_logits" else lg
    return lg.to(dt), score_fp32(src[:, 0], src[:, 1]).to(dt)


def build_index(cu, img_start, B, n, mutant=None):
    """row_index [B n], cu_img [B + 1] as vp_build_index specifies them."""
    cu, st = cu.long(), img_start.long()
    rows = torch.cat([cu[b] + (st[0] if mutant == "img_start_of_row0" else st[b]) + torch.arange(n) for b in range(B)])
    return rows.int(), (torch.arange(B + 1) * n).int()


def vp_layout(B, n, H, D, FF, dtype):
    """csrc/predictors.hip vp_layout, restated: byte offsets of the workspace regions and the total."""
    es = 4 if dtype == F32 else 2
    M = B * n
    a256 = lambda v: (v + 255) & ~255
    out, o = {}, 0
    for name, size in (("x0", M * H * es), ("hs", M * D * es), ("y", M * D * es), ("qkv", M * 3 * D * es), ("ff", M * FF * es), ("z", M * D * es), ("z1", M * (D // 2) * es),
                       ("z2", M * (D // 4) * es), ("row_index", M * 4), ("cu_img", (B + 1) * 4)):
        out[name] = o
        o += a256(size)
    out["total"] = o
    return out
