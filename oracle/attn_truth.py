"""Attention test cases, their fp64 truth and a derived per-element error bound (CPU only, plain torch).

Used by tests/test_attn_truth_cpu.py (the bound discriminates: a tiled emulation of the documented arithmetic is inside it, small
mutants of that emulation are outside), tests/test_attn_routes_gpu.py (every HIP attention kernel against the truth) and
tools/attn_error_table.py (the measured table of docs/attention_error_budget.md).

Truth
-----
`truth(q, k, v, ...)`: attention in fp64 on the operands exactly as the kernel reads them (already rounded to bf16 / fp16 / fp32).  Masks:
none, causal, and "chunk on a cache" (query j sees keys <= kv_offset + j; causal is kv_offset = 0; a decode row is one query without a
mask over kv_len + extra keys).  GQA: query head h reads kv head h // (nH // nKV).  Per query row and head it returns

    O     = softmax(S) V                      the answer
    A     = softmax(S) |V|                    the magnitude the roundings act on (A >= |O|; equal without cancellation)
    S_abs = scale * max_j sum_i |q_i k_ij|    condition of the largest visible score
    n_vis                                     visible keys of the row
    l     = sum_j exp(s_j - max s)            (>= 1) and  V1 = sum_j |v_j| over the visible keys, for the fp16 term below

Bound
-----
    tol = c16 * ULP[dtype] * A  +  2 (n_vis + d + 8) 2^-24 (1 + S_abs) A  +  sub

Every coefficient has an origin; none was fitted to a kernel's output.

* ULP[dtype]: 2^-7 (bf16), 2^-10 (fp16), 2^-23 (fp32) -- spacing of the type in [1, 2), as in tests/test_kernels_gpu.py.  A value
  rounded to nearest moves by at most ULP/2 of its own magnitude.
* c16 = 1 for the 16-bit types, two roundings of ULP/2 each, both specified in include/dynllava.h ("P rounded to the dtype before P V",
  one output rounding): sum_j |dp_j| |v_j| <= ULP/2 * A and |dO| <= ULP/2 * |O| <= ULP/2 * A.  c16 = 0 for fp32 (neither happens).
* 2^-24: unit roundoff of the fp32 accumulators.  (n_vis + d + 8): a score is a d-term dot product, the row sum and each output element
  are n_vis-term sums -- first-order error k u of a k-term fp32 sum in any order (tiled, split over waves, merged partials) -- and 8
  covers the handful of single operations around them: scale, max subtraction, the exponential (v_exp_f32 / expf: <= 2 ulp), the rescale
  of the running sum and accumulator per tile, the reciprocal, the final multiply.  The factor 2: numerator and denominator each carry it.
* (1 + S_abs): the exponential turns an ABSOLUTE error of its argument into a RELATIVE error of p.  The argument s_j - m carries the dot
  product's error, at most d u * scale * sum_i |q_i k_ij| <= d u S_abs: the "1" is the relative part (sums), "S_abs" the part that
  scales with |s|.  This term is why rows with |s| in the hundreds (`big`) sit far below ratio 1: they guard overflow, not the last bit.
* sub (fp16 only) = 2^-25 * V1 / l + 2^-25.  Below fp16's normal range (2^-14) values round to a fixed quantum 2^-24, i.e. an absolute
  error of up to 2^-25 that ULP * A does not scale with: once per key for a flushed P (times |v_j|, divided by the row sum l), and once
  for an output element below 2^-14.  bf16 has fp32's exponent range: no such term.

Distributions (make_case), each seeded; `check_property` asserts the property that makes a distribution worth having.
Emulation (emulate) and its mutants (MUTANTS): see the functions.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

ULP = {torch.float32: 2.0**-23, torch.float16: 2.0**-10, torch.bfloat16: 2.0**-7}
DISTRIBUTIONS = ("gauss", "sink", "late_peak", "ramp", "plateau", "big", "v_outlier")
DECODE_ONLY = ("newtok", "newtok_mirror")
MUTANTS = ("mask_off_by_one_last_tile", "l_not_rescaled", "read_past_lk", "gqa_off_by_one_group", "max_not_carried")
TILE = 64


# ------------------------------------------------------------------------------------------------------------------------------
# truth and bound
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Truth:
    O: torch.Tensor      # [Lq, nH', d] fp64
    A: torch.Tensor      # [Lq, nH', d]
    S_abs: torch.Tensor  # [Lq, nH']
    n_vis: torch.Tensor  # [Lq] (int64)
    l: torch.Tensor      # [Lq, nH']
    V1: torch.Tensor     # [Lq, nH', d]
    s_max: float         # largest |score| over the visible pairs
    P0: torch.Tensor     # [Lq, nH'] softmax mass of key 0
    heads: list


def _visible(Lq, Lk, causal, kv_offset):
    """[Lq, Lk] bool: query j sees key i.  causal / chunk on a cache: i <= kv_offset + j."""
    if not causal:
        return torch.ones(Lq, Lk, dtype=torch.bool)
    return torch.arange(Lk)[None, :] <= (torch.arange(Lq)[:, None] + int(kv_offset))


def truth(q, k, v, causal=False, kv_offset=0, heads=None):
    """q [Lq, nH, d], k / v [Lk, nKV, d] (any float dtype; taken as they are).  heads: the query heads to evaluate (default all; long rows:
    a few).  The head axis of every result follows `heads`."""
    Lq, nH, d = q.shape
    Lk, nKV = k.shape[0], k.shape[1]
    assert nH % nKV == 0 and v.shape == k.shape
    n_rep = nH // nKV
    heads = list(range(nH)) if heads is None else list(heads)
    scale = 1.0 / math.sqrt(d)
    vis = _visible(Lq, Lk, causal, kv_offset)
    assert bool(vis.any(1).all()), "a query row without a visible key has no softmax"
    O, A, S_abs, l_, V1, P0 = [], [], [], [], [], []
    s_max = 0.0
    visd = vis.double()
    for h in heads:
        qh, kh, vh = q[:, h].double(), k[:, h // n_rep].double(), v[:, h // n_rep].double()
        s = (qh @ kh.T) * scale
        s_max = max(s_max, float(s[vis].abs().max()))
        sa = ((qh.abs() @ kh.abs().T) * scale).masked_fill(~vis, 0.0)
        s = s.masked_fill(~vis, -math.inf)
        e = torch.exp(s - s.max(1, keepdim=True).values)
        l = e.sum(1, keepdim=True)
        p = e / l
        O.append(p @ vh)
        A.append(p @ vh.abs())
        S_abs.append(sa.max(1).values)
        l_.append(l[:, 0])
        V1.append(visd @ vh.abs())
        P0.append(p[:, 0])
    st = lambda xs: torch.stack(xs, 1)
    return Truth(st(O), st(A), st(S_abs), vis.sum(1), st(l_), st(V1), s_max, st(P0), heads)


def bound(t: Truth, d: int, dtype) -> torch.Tensor:
    """The per-element tolerance of the module docstring, [Lq, nH', d]."""
    c16 = 0.0 if dtype == torch.float32 else 1.0
    n = t.n_vis.double()[:, None, None]
    tol = c16 * ULP[dtype] * t.A + 2.0 * (n + d + 8) * 2.0**-24 * (1.0 + t.S_abs[:, :, None]) * t.A
    if dtype == torch.float16:
        tol = tol + 2.0**-25 * t.V1 / t.l[:, :, None] + 2.0**-25
    return tol


def worst_ratio(out, t: Truth, d: int, dtype):
    """(max err / tol, max err in units of ULP * |truth element|, flat index of the worst element) for `out` [Lq, nH', d] (the heads of `t`).
    A NaN / Inf in `out` gives ratio inf."""
    err = (out.double() - t.O).abs()
    ratio = err / bound(t, d, dtype)
    ratio = torch.where(torch.isfinite(out.double()), ratio, torch.full_like(ratio, math.inf))
    ulps = err / (ULP[dtype] * t.O.abs().clamp_min(1e-300))
    ulps = torch.where(err == 0, torch.zeros_like(ulps), ulps)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), float(ulps[torch.isfinite(ulps)].max()) if bool(torch.isfinite(ulps).any()) else 0.0, i


# ------------------------------------------------------------------------------------------------------------------------------
# distributions
# ------------------------------------------------------------------------------------------------------------------------------
def _unit(d, g):
    u = torch.randn(d, generator=g)
    return u / u.norm()


def _rope_dir(w, rope, dtype):
    """Direction of the ROTATED query: the fused decode kernels rotate q (and the appended key) themselves, so slab keys are planted
    relative to apply_rope(w) at the new token's position, evaluated like the kernels do (every operation rounded to the dtype)."""
    if rope is None:
        return w
    from oracle.ref_cpu import apply_rope

    cos, sin, pos = rope
    x = w.to(dtype)[None, None, None, :]
    r, _ = apply_rope(x, x, cos.to(dtype), sin.to(dtype), torch.tensor([[int(pos)]]))
    r = r[0, 0, 0].float()
    return r / r.norm()


def make_case(name, Lq, Lk, d, dtype, seed, nH=1, nKV=1, peak_at=None, rope=None):
    """q [Lq, nH, d], k / v [Lk, nKV, d] in `dtype`.  Query j is aligned with key kv_offset + j where that matters (Lq <= Lk, the queries are the
    last Lq positions).  peak_at (late_peak): index of the dominant key, or (dominant, second), instead of the default (three before the end, inside the last 64-key tile; second: Lk // 2).
    rope = (cos, sin, pos): decode through a fused-RoPE kernel -- q and the LAST key (the appended token) are returned un-rotated, keys
    0 .. Lk-2 (the slab) are planted relative to the rotated query."""
    assert name in DISTRIBUTIONS + DECODE_ONLY and nH % nKV == 0 and 1 <= Lq <= Lk
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * DISTRIBUTIONS.index(name) if name in DISTRIBUTIONS else 1000003 * seed + 31)
    n_rep = nH // nKV
    q = torch.randn(Lq, nH, d, generator=g)
    k = torch.randn(Lk, nKV, d, generator=g)
    v = torch.randn(Lk, nKV, d, generator=g)
    sd = math.sqrt(d)
    n_slab = Lk - 1 if rope is not None else Lk  # keys that are stored rotated already
    for kvh in range(nKV):
        w = _unit(d, g)          # direction of this group's queries (and of an un-rotated appended key)
        wk = _rope_dir(w, rope, dtype)  # the same direction as the slab keys see it
        hs = slice(kvh * n_rep, (kvh + 1) * n_rep)
        kdir = lambda i: (wk if i < n_slab else w)
        if name == "sink":
            # key 0 = c w scores ln(Lk) + 5 for every query (their noise is made orthogonal to w; the other keys' scores: mean 0, std ~ 1.1 .. 1.5): it keeps
            # > 0.9 of every row's mass without reducing the others to nothing; every seventh key is anti-aligned, its p far below 2^-24 (flushed in fp16)
            qn = q[:, hs]
            q[:, hs] = qn - (qn @ w)[..., None] * w + 6.0 * w
            k[0, kvh] = (math.log(Lk) + 5.0) * sd / 6.0 * kdir(0)
            for i in range(3, Lk, 7):
                k[i, kvh] -= 12.0 * sd / 6.0 * kdir(i)
            v[0, kvh] *= 0.01
        elif name == "late_peak":
            j1, j2 = max(Lk - 4, ((Lk - 1) // TILE) * TILE), Lk // 2
            if peak_at is not None:
                j1, j2 = (int(peak_at), j2) if isinstance(peak_at, int) else (int(peak_at[0]), int(peak_at[1]))
            q[:, hs] += 4.0 * w
            k[j1, kvh] += 30.0 * kdir(j1)
            if j2 != j1:
                k[j2, kvh] += 20.0 * kdir(j2)
        elif name == "ramp":
            # k_j = t_j u, t_j rising linearly; even query rows look along +u (scores rise with the key index), odd ones along -u (they fall)
            sign = torch.where(torch.arange(Lq) % 2 == 0, 1.0, -1.0)[:, None, None]
            q[:, hs] = 0.1 * q[:, hs] + 4.0 * sign * w
            t = torch.linspace(-20.0, 20.0, Lk) if Lk > 1 else torch.zeros(1)
            kd = torch.stack([kdir(i) for i in range(Lk)]) if rope is not None else w[None].expand(Lk, d)
            k[:, kvh] = 0.1 * k[:, kvh] + t[:, None] * kd
        elif name == "plateau":
            # one key row repeated: every p of a query row is the SAME number, so its rounding error has one sign (no cancellation over keys);
            # one key (at a third of the row) scores higher; V positive, so that neither does the sum over V cancel
            base = k[0, kvh].clone()
            k[:, kvh] = base
            k[Lk // 3, kvh] = 1.5 * base
            v[:, kvh] = v[:, kvh].abs() + 1.0
        elif name == "big":
            pass  # (scaled below, both operands)
        elif name == "v_outlier":
            v[:, kvh, 3] *= 1000.0 if dtype != torch.float16 else 200.0
            v[::7, kvh, 5] = -v[::7, kvh, 5] * 50.0
        elif name in DECODE_ONLY:
            # the appended token (last key) dominates / is negligible
            q[:, hs] += 4.0 * w
            k[Lk - 1, kvh] += (30.0 if name == "newtok" else -30.0) * kdir(Lk - 1)
    if name == "big":
        q, k = q * 12.0, k * 12.0
    return q.to(dtype), k.to(dtype), v.to(dtype)


def check_property(name, q, k, v, causal=False, kv_offset=0, dtype=None):
    """Asserts the property of the distribution table on a generated case; returns a short description of what it found."""
    dtype = q.dtype if dtype is None else dtype
    t = truth(q, k, v, causal, kv_offset)
    Lq, Lk = q.shape[0], k.shape[0]
    if name == "sink":
        assert float(t.P0.min()) > 0.9, f"sink: key 0 holds only {float(t.P0.min()):.3f} of some row's mass"
        s = (q[-1, 0].double() @ k[:, 0].double().T) / math.sqrt(q.shape[2])
        p = torch.exp(s - s.max())
        n_flush = int((p < 2.0**-24).sum())
        assert Lk < 4 or n_flush > 0, "sink: no p below 2^-24"
        return f"min mass of key 0 {float(t.P0.min()):.3f}; {n_flush} of {Lk} p below 2^-24 in the last row"
    if name == "late_peak":
        # the running maximum of the last query row changes in the last 64-key tile
        n_rep = q.shape[1] // k.shape[1]
        last0 = ((Lk - 1) // TILE) * TILE
        moved = 0
        for h in range(q.shape[1]):
            sh = k[:, h // n_rep].double() @ q[-1, h].double()
            if last0 == 0 or float(sh[last0:].max()) > float(sh[:last0].max()):
                moved += 1
        assert moved == q.shape[1], f"late_peak: the maximum moves in the last tile for {moved} of {q.shape[1]} heads only"
        return f"running max moves in the last tile (keys {last0}..{Lk - 1}) for all {moved} heads"
    if name == "plateau":
        # the rounding error of P has one sign over the plateau keys of a row and is a visible fraction of an ulp for most rows
        if dtype == torch.float32:
            return "fp32: P is not rounded"
        s = (q[:, 0].float() @ k[:, 0].float().T) / math.sqrt(q.shape[2])
        s = s.masked_fill(~_visible(Lq, Lk, causal, kv_offset), -math.inf)
        p = torch.exp(s - s.max(1, keepdim=True).values)
        rel = ((p.to(dtype).float() - p) / p.clamp_min(1e-30)).masked_fill(p == 0, 0.0)
        keys = [i for i in range(Lk) if i != Lk // 3]
        rk = rel[:, keys]
        one_sign = ((rk >= 0).all(1) | (rk <= 0).all(1))
        assert bool(one_sign.all()), "plateau: the P rounding errors of a row differ in sign"
        if Lq < 16:  # (a decode row: no statistics over rows)
            return "P rounding error has one sign per row"
        below = p[:, keys].max(1).values < 1.0  # rows whose maximum is the higher key (where the plateau is the maximum its p is exactly 1)
        assert int(below.sum()) >= Lq // 8, "plateau: the higher key is (almost) never the maximum"
        frac = float((rk.abs().max(1).values > ULP[dtype] / 16)[below].float().mean())
        assert frac > 0.5, "plateau: P rounds (almost) exactly in most rows"
        return f"P rounding error has one sign per row; > ULP/16 in {frac:.2f} of the {int(below.sum())} rows under the higher key"
    if name == "big":
        fin = all(bool(torch.isfinite(x.float()).all()) for x in (q, k, v)) and bool(torch.isfinite(t.O).all())
        assert t.s_max > 500.0 and fin, f"big: max |s| = {t.s_max:.0f}, finite = {fin}"
        return f"max |s| = {t.s_max:.0f}, everything finite"
    return ""


# ------------------------------------------------------------------------------------------------------------------------------
# emulation of the documented arithmetic, and mutants of it
# ------------------------------------------------------------------------------------------------------------------------------
def emulate(q, k, v, causal=False, kv_offset=0, mutant=None, tile=TILE, pad_kv=None):
    """Tiled online softmax as include/dynllava.h documents it: key tiles of `tile`, fp32 scores and statistics (running max m, running sum l
    of the UNROUNDED p), P rounded to the 16-bit dtype before P V, fp32 accumulators rescaled when m moves, one output rounding.
    mutant: one of MUTANTS (a bug of the kind these kernels can have), None = correct.  pad_kv = (k_row, v_row) [nKV, d]: what lies in memory
    behind key Lk - 1 (only `read_past_lk` reads it; default: a copy of key 0, the next request's BOS token in a packed batch).
    `max_not_carried` takes each tile's own maximum as the new reference and rescales consistently: exact in real arithmetic, it overflows
    exp() once an earlier tile's maximum lies ~88 above a later one's -- the bug only `big` scores can show.  Returns [Lq, nH, d] in q.dtype."""
    assert mutant is None or mutant in MUTANTS
    dt = q.dtype
    Lq, nH, d = q.shape
    Lk, nKV = k.shape[0], k.shape[1]
    n_rep = nH // nKV
    scale = 1.0 / math.sqrt(d)
    if mutant == "read_past_lk" and Lk % tile != 0:
        if pad_kv is None:  # a packed batch: the next request's first token -- the same BOS token, hence the same key / value row as this one's
            pad_kv = (k[0], v[0])
        k = torch.cat([k, pad_kv[0][None].to(dt)])
        v = torch.cat([v, pad_kv[1][None].to(dt)])
    Lk_read = k.shape[0]
    qi = torch.arange(Lq)[:, None] + int(kv_offset)
    out = torch.empty(Lq, nH, d, dtype=dt)
    for h in range(nH):
        kvh = h // n_rep
        if mutant == "gqa_off_by_one_group":
            kvh = (kvh + 1) % nKV
        qh = q[:, h].float()
        m = torch.full((Lq, 1), -math.inf)
        l = torch.zeros(Lq, 1)
        acc = torch.zeros(Lq, d)
        for t0 in range(0, Lk_read, tile):
            t1 = min(t0 + tile, Lk_read)
            ks, vs = k[t0:t1, kvh].float(), v[t0:t1, kvh].float()
            s = (qh @ ks.T) * scale
            if causal:
                ki = torch.arange(t0, t1)[None, :]
                lim = qi + 1 if (mutant == "mask_off_by_one_last_tile" and t1 >= Lk) else qi
                s = s.masked_fill(ki > lim, -math.inf)
            mx = s.max(1, keepdim=True).values
            m_new = torch.where(torch.isinf(mx), m, mx) if (mutant == "max_not_carried" and t0 > 0) else torch.maximum(m, mx)
            m_ref = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)  # a row that has seen no key yet: exp(-inf - 0) = 0
            alpha = torch.exp(m - m_ref)
            p = torch.exp(s - m_ref)
            l = (l if mutant == "l_not_rescaled" else l * alpha) + p.sum(1, keepdim=True)
            acc = acc * alpha + p.to(dt).float() @ vs
            m = m_new
        out[:, h] = (acc / l).to(dt)
    return out


def plant_slab(name, q_rot, T, nKV, d, dtype, seed, peak_at=None):
    """Slab keys / values [T, nKV, d] for a decode step whose ROTATED queries q_rot [nH, d] already exist (dl_gemv_qkv_attn: q is the
    projection's output, it cannot be chosen): the distribution's keys are planted along each group's mean query direction, scaled by
    that group's mean projection so that a planted key scores what make_case's would.  gauss, sink, late_peak, v_outlier as there;
    newtok / newtok_mirror: every slab key scores ~ -15 / +15, so the appended token (the projection's own key, score ~ 0) dominates /
    is negligible."""
    assert name in ("gauss", "sink", "late_peak", "v_outlier") + DECODE_ONLY
    g = torch.Generator().manual_seed(1000003 * seed + 97)
    nH = q_rot.shape[0]
    n_rep = nH // nKV
    sd = math.sqrt(d)
    k = torch.randn(T, nKV, d, generator=g)
    v = torch.randn(T, nKV, d, generator=g)
    if T == 0:
        return k.to(dtype), v.to(dtype)
    for kvh in range(nKV):
        qg = q_rot[kvh * n_rep : (kvh + 1) * n_rep].float()
        u = qg.mean(0)
        u = u / u.norm()
        proj = float((qg @ u).mean())  # > 0: u is the mean direction
        unit = sd / proj * u           # a key `s * unit` scores s for the group's mean query
        if name == "sink":
            k[0, kvh] = (math.log(T + 1) + 5.0) * unit
            for i in range(3, T, 7):
                k[i, kvh] -= 12.0 * unit
            v[0, kvh] *= 0.01
        elif name == "late_peak":
            j1, j2 = max(T - 4, ((T - 1) // TILE) * TILE), T // 2
            if peak_at is not None:
                j1, j2 = (int(peak_at), j2) if isinstance(peak_at, int) else (int(peak_at[0]), int(peak_at[1]))
            k[j1, kvh] += 16.0 * unit
            if j2 != j1:
                k[j2, kvh] += 10.0 * unit
        elif name == "v_outlier":
            v[:, kvh, 3] *= 1000.0 if dtype != torch.float16 else 200.0
            v[::7, kvh, 5] = -v[::7, kvh, 5] * 50.0
        elif name in DECODE_ONLY:
            k[:, kvh] += (-15.0 if name == "newtok" else 15.0) * unit
    return k.to(dtype), v.to(dtype)
