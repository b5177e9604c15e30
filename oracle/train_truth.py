"""Policy attention and Gumbel hard keep (csrc/train_policy.hip): test inputs, fp64 truth, a derived per-element error bound, a tiled
emulation of the documented arithmetic and mutants of it (CPU only, plain torch).

Used by tests/test_train_truth_cpu.py (the emulation is inside the bound, every mutant is outside it somewhere), by oracle/train_cases.py
and tests/test_train_policy_gpu.py (the HIP kernels against the truth) and written up in docs/train_policy_error_budget.md.

Truth
-----
`truth(case)`: fp64 on the operands exactly as the kernels read them (bf16 / f16 q, k, v, dO and bias; fp32 policy), from the formulas in
the header of train_policy.hip:

    s_ij = scale q_i.k_j + bias_ij   (-inf where masked)        m_i = max_j s_ij        e_ij = exp(s_ij - m_i)
    pe_ij = e_ij p'_ij  (p'_ij = policy_j, p'_ii = 1)           Dn_i = sum_j pe_ij + eps     A_ij = (pe_ij + eps/N) / Dn_i  (every j < L)
    o = A v      delta_i = dO_i.o_i     dA_ij = dO_i.v_j     dE_ij = (dA_ij - delta_i) / Dn_i     dS_ij = dE_ij pe_ij
    dV = A^T dO      dQ = scale dS k      dK = scale dS^T q      dpolicy_j = sum_h sum_{i != j} dE_ij e_ij

with m_i a CONSTANT in the backward (what the kernels specify).  `autograd_grads(case)` is the second gradient set: full fp64 autograd of
`ref64`, an fp64 restatement of oracle.ref_cpu.sdpa_with_policy (which casts to fp32 inside; the CPU test pins the two together).

Bound (one per output tensor; U = spacing of the dtype in [1, 2), u = 2^-24, |x| elementwise)
-----
    "active" entries of a row: not masked with -inf and within 104 of the row maximum -- beyond that gap exp() is below 2^-149, exactly 0 in
    fp32 whatever the score's own error, so no rounding of such an entry reaches an output (a key masked with a FINITE finfo.min is not
    active unless the whole row is masked).  n_vis, S_abs and V1 below run over the active entries.
    rel_i   = 2 (n_vis_i + d + 8) u (1 + S_abs_i) + E_add_i
              fp32 error of a pe_ij or of Dn_i relative to itself: sums of n_vis terms, d-term dot products whose absolute error d u S_abs
              (S_abs_i = scale max_j sum_c |q_ic k_jc|) the exponential turns into a relative one, 8 single operations.  With a bias,
              E_add_i = u (2 |m_i| + span_i), span_i = the largest gap m_i - x_ij of an active entry: the fp32 add x_ij = s_ij + bias_ij
              carries u |x_ij| <= u (|m_i| + gap_ij) and the maximum itself u |m_i|.  A row whose maximum is an ordinary score: ~1e-6; a
              row fully masked with f16's finfo.min (m_i ~ -65504): 0.0078; 0 where the maximum absorbs its score in fp64 as well
              (|bias| >= 2^60 (1 + S_abs): bf16's finfo.min).
    out     : U Aabs + rel Aabs [+ 2^-25 V1 / Dn + 2^-25]             Aabs = A |v|, V1_i = sum_{j active} |v_j|
              P rounded to the dtype before P V and the output rounding (U/2 each), fp32; f16: an unnormalised pe below 2^-14 rounds
              to the fixed quantum 2^-24, an absolute error that the division by Dn_i carries.
    delta   : err_delta_i = sum_c |dO_ic| tol_out_ic + (d + 2) u sum_c |dO_ic| Aabs_ic     (delta is formed from the kernel's own rounded o)
    dE      : |dE|_ij := (|dA_ij| + sum_c |dO_ic o_ic|) / Dn_i   -- the cancellation in dA - delta is charged --
              err_dE_ij = (err_delta_i + d u sum_c |dO_ic v_jc|) / Dn_i + (2 rel_i + 4 u) |dE|_ij
    dS      : R_ij = (U/2) |dE|_ij pe_ij + err_dE_ij pe_ij [+ 2^-25 active_ij]     (dS^T rounded to the dtype before the second MFMA)
    dq      : scale R |k| + (n_vis + 8) u scale (|dE| pe) |k| + (U/2) |dq| [+ 2^-25]
    dk      : scale R^T |q| + (L + 8) u scale (|dE| pe)^T |q| + (U/2) |dk| [+ 2^-25]
    dv      : ((U/2 + 2 rel + (L + 12) u) A [+ 2^-25 active])^T |dO| + (U/2) |dv| [+ 2^-25]     (A^T = pe / Dn rounded to the dtype)
    dpolicy : sum_h sum_{i != j} e_ij (err_dE_ij + (L + H + 8) u |dE|_ij) [+ (U/2) |dpolicy| when the wrapper rounds it to the policy's dtype]
    every tolerance also carries fp32's underflow: a flushed e_ij or product is an absolute error of 2^-126 (times |dE|_ij, |v_j| / Dn_i or
    |dO_i| / Dn_i as the contraction has it) -- visible only where `big` scores put whole rows below 1e-38.
No constant was fitted to a kernel.  A tolerance of exactly 0 (a key no other row sees has dpolicy_j = 0 exactly) demands exactly 0.
A dpolicy beyond the dtype's largest finite value (f16: `big`, `leak_rows`) is +-inf once the wrapper rounds it; that is what is accepted.

Gumbel keep: `gumbel_truth`, see there.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

from oracle import attn_truth as at

ULP = at.ULP
TILE = 64
EPS = 1e-6
INPUTS = at.DISTRIBUTIONS + ("leak_rows",)
POLICIES = ("pattern", "ones", "zeros", "edges", "frac")
OUTPUTS = ("out", "dq", "dk", "dv", "dpolicy")
MUTANTS = ("leak_dropped", "self_first_tile_only", "dpolicy_with_diagonal", "policy_one_late_last_tile", "causal_skip_one_wave", "first_qtile_one_late_128",
           "stats_from_head0", "bias_row_stride_ignored", "l_not_rescaled")
# inputs on which the gradient through max_j is asserted to be below the bound (recorded, not asserted, on the others): their row maximum is
# a kept key or the row's own key in (almost) every row, so Dn_i >= 1 and the term eps (delta_i - dO_i . mean_j v_j) / Dn_i is O(eps) with
# |delta_i| = O(1).  Not `v_outlier` (|v| up to 1000 scales delta_i alike: measured 2x the dk bound), `late_peak` / `big` (dropped keys lead rows)
MAXGRAD_BELOW_BOUND = ("gauss", "sink", "ramp", "plateau")


@dataclass
class Case:
    q: torch.Tensor        # [B,H,L,d] model dtype (any strides)
    k: torch.Tensor
    v: torch.Tensor
    do: torch.Tensor
    policy: torch.Tensor   # fp32 [B,L]
    bias: torch.Tensor = None  # model dtype [B or 1,1,L,L] (any strides) or None
    causal: bool = False
    eps: float = EPS
    n_eps: int = 0         # N of eps / N (0: L)
    name: str = ""
    leak_keys: list = field(default_factory=list)

    @property
    def shape(self):
        return tuple(self.q.shape)

    @property
    def scale(self):
        return 1.0 / math.sqrt(self.q.shape[-1])

    @property
    def N(self):
        return self.n_eps or self.q.shape[2]


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def leak_key_positions(L):
    """Index 0 of a key tile, index 63 of a key tile, and one inside the last (partial) tile -- as far as L has them."""
    last0 = ((L - 1) // TILE) * TILE
    cand = [0, 63, last0 + (L - 1 - last0) // 2]
    return sorted({j for j in cand if j < L - 1})


def make_policy(kind, B, L, seed, leak_keys=()):
    g = torch.Generator().manual_seed(7001 + 13 * seed + L)
    if kind == "pattern":  # tests/test_train_ops_gpu.py's
        p = (torch.rand(B, L, generator=g) > 0.4).float()
        p[:, : max(1, L // 4)] = 1.0
        p[:, L // 2] = 0.37
    elif kind == "ones":
        p = torch.ones(B, L)
    elif kind == "zeros":
        p = torch.zeros(B, L)
    elif kind == "edges":
        p = torch.ones(B, L)
        for j in (0, 15, 16, 63, 64, 127, 128, L - 1):
            if j < L:
                p[:, j] = 0.0
    elif kind == "frac":
        p = torch.rand(B, L, generator=g).clamp(2.0**-10, 1.0 - 2.0**-10)
    else:
        raise ValueError(kind)
    for j in leak_keys:
        p[:, j] = 0.0
    return p


def make_inputs(name, B, H, L, d, dtype, seed=0, policy="pattern"):
    """q, k, v, dO as [B,L,H,d] storage viewed [B,H,L,d] (the attention module's layout) and the fp32 policy.  The distributions of
    attn_truth.make_case, one request per batch row; `leak_rows`: dropped keys (leak_key_positions) whose score leads every other visible key
    of two rows in three by ~30 > ln(1 / eps): those rows' Dn_i falls to ~eps and the eps / N leak IS the row."""
    assert name in INPUTS
    qs, ks, vs = [], [], []
    leak = leak_key_positions(L) if name == "leak_rows" else []
    for b in range(B):
        q, k, v = at.make_case("gauss" if name == "leak_rows" else name, L, L, d, torch.float32, seed=seed * 131 + b, nH=H, nKV=H)
        if name == "v_outlier" and dtype == torch.float16:
            q, k, v = at.make_case(name, L, L, d, dtype, seed=seed * 131 + b, nH=H, nKV=H)
        if name == "leak_rows":
            g = torch.Generator().manual_seed(977 * seed + b)
            rows = torch.arange(L) % 3 != 0
            for h in range(H):
                w = torch.randn(d, generator=g)
                w = w / w.norm()
                qb = q[rows, h]
                q[rows, h] = qb - (qb @ w)[:, None] * w + 6.0 * w  # boosted rows: exactly 6 along w
                for j in leak:
                    k[j, h] += 5.0 * math.sqrt(d) * w               # score 30 for a boosted row, 5 N(0,1) for the others
        qs.append(q), ks.append(k), vs.append(v)
    g = torch.Generator().manual_seed(424243 + seed)
    do = torch.randn(B, L, H, d, generator=g)
    q, k, v = (torch.stack(x) for x in (qs, ks, vs))
    q, k, v, do = (t.to(dtype).transpose(1, 2) for t in (q, k, v, do))
    return q, k, v, do, make_policy(policy, B, L, seed, leak), leak


def make_bias(kind, B, L, dtype, seed=0):
    """The additive mask of a mask kind, [B or 1,1,L,L] in the model dtype (bool for "bool"); None for "causal" / "none".
    additive / bool: causal, right padding of the later batch rows (tests/test_train_ops_gpu.py's); soft: causal + random values in [-2, 0];
    batch1: causal, shape[0] == 1; keypad: [B,1,1,L] key padding expanded (row stride 0), no causal part; leftpad: causal + left padding
    with finfo.min as transformers builds it -- the padded query rows are fully masked."""
    if kind in ("causal", "none"):
        return None
    neg = torch.finfo(dtype).min
    future = torch.ones(L, L, dtype=torch.bool).tril().logical_not()[None, None]
    if kind == "keypad":
        m = torch.zeros(B, 1, 1, L, dtype=dtype)
        if L > 1:
            m[B - 1, :, :, L - max(1, L // 4):] = neg
        return m.expand(B, 1, L, L)
    m = torch.zeros(1 if kind == "batch1" else B, 1, L, L, dtype=dtype)
    m.masked_fill_(future, neg)
    if kind in ("additive", "bool") and B > 1 and L > 5:
        m[1:, :, :, L - 5:] = neg
    if kind == "soft":
        g = torch.Generator().manual_seed(31 + seed)
        m = torch.where(m == 0, (-2.0 * torch.rand(B, 1, L, L, generator=g)).to(dtype), m)
    if kind == "leftpad" and L > 1:
        pad = max(1, L // 5)
        m[B - 1, :, :, :pad] = neg
        m[B - 1, :, :pad, :] = neg
    if kind == "bool":
        return m == 0
    return m


def make_case(name, B, H, L, d, dtype, kind="causal", policy="pattern", seed=0, n_eps=0):
    q, k, v, do, pol, leak = make_inputs(name, B, H, L, d, dtype, seed, policy)
    pol = pol.to(dtype).float()  # the module hands the policy over in the model dtype
    bias = make_bias(kind, B, L, dtype, seed)
    if bias is not None and bias.dtype == torch.bool:  # as the wrapper converts it
        bias = torch.zeros(bias.shape, dtype=dtype).masked_fill_(bias.logical_not(), float("-inf"))
    return Case(q, k, v, do, pol, bias, kind == "causal", EPS, n_eps, name, leak)


# ------------------------------------------------------------------------------------------------------------------------------
# truth and bound
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Truth:
    out: torch.Tensor
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor
    dpolicy: torch.Tensor  # [B,L]
    Dn: torch.Tensor       # [B,H,L]
    aux: dict


GAP_MAX = 104.0  # exp(-104) < 2^-149: beyond this gap to the row maximum fp32 holds e_ij = 0 exactly, whatever the score's own error


def _scores(c: Case):
    """fp64 s [B,H,L,L] (-inf where masked), the ACTIVE entries (not masked and within GAP_MAX of the row maximum: the only ones whose
    e_ij is not exactly 0 in fp32 -- a key masked with a finite finfo.min is not active unless the whole row is), S_abs [B,H,L], E_add [B,H,L]."""
    B, H, L, d = c.shape
    q, k = c.q.double(), c.k.double()
    s = (q @ k.transpose(-1, -2)) * c.scale
    sabs = (q.abs() @ k.abs().transpose(-1, -2)) * c.scale
    vis = torch.ones(L, L, dtype=torch.bool).expand(B, H, L, L)
    absorbed = torch.zeros(B, H, L, L, dtype=torch.bool)
    if c.causal:
        vis = vis & torch.ones(L, L, dtype=torch.bool).tril()
    if c.bias is not None:
        b = c.bias.double().expand(B, 1, L, L)
        vis = vis & ~torch.isneginf(b)
        absorbed = b.abs() >= 2.0**60 * (1.0 + sabs)
        s = s + b
    s = s.masked_fill(~vis, -math.inf)
    assert bool(vis.any(-1).all()), "a query row without a visible key has no softmax (the reference returns NaN)"
    m, jmax = s.max(-1, keepdim=True)
    gap = m - s
    act = vis & (gap <= GAP_MAX)
    e_add = torch.zeros(B, H, L, dtype=torch.float64)
    if c.bias is not None:
        # the fp32 add of the bias: x_ij = s_ij + bias_ij carries u |x_ij| <= u (|m_i| + gap_ij), m_i = x_i,argmax carries u |m_i|, so the
        # argument of an active entry's exponential carries u (2 |m_i| + gap_ij); nothing where the row maximum absorbs its score in fp64 too
        span = gap.masked_fill(~act, 0.0).amax(-1)
        e_add = 2.0**-24 * (2.0 * m[..., 0].abs() + span)
        e_add = torch.where(absorbed.gather(-1, jmax)[..., 0], torch.zeros_like(e_add), e_add)
    return s, vis, act, sabs.masked_fill(~act, 0.0).amax(-1), e_add


def truth(c: Case) -> Truth:
    B, H, L, d = c.shape
    s, vis, act, S_abs, E_add = _scores(c)
    v, do, q, k = c.v.double(), c.do.double(), c.q.double(), c.k.double()
    e = torch.exp(s - s.amax(-1, keepdim=True))
    eye = torch.eye(L, dtype=torch.float64)
    pol = c.policy.double()[:, None, None, :]
    pp = pol + (1.0 - pol) * eye
    pe = e * pp
    Dn = pe.sum(-1) + c.eps
    cl = c.eps / c.N
    A = (pe + cl) / Dn[..., None]
    o = A @ v
    dA = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1)
    dE = (dA - delta[..., None]) / Dn[..., None]
    dS = dE * pe
    dq = c.scale * (dS @ k)
    dk = c.scale * (dS.transpose(-1, -2) @ q)
    dv = A.transpose(-1, -2) @ do
    dpol = (dE * e * (1.0 - eye)).sum(dim=(1, 2))
    aux = dict(vis=vis, act=act, S_abs=S_abs, E_add=E_add, e=e, pe=pe, A=A, dA=dA, o=o)
    return Truth(o, dq, dk, dv, dpol, Dn, aux)


def bound(t: Truth, c: Case, dpolicy_rounded=True, H_total=None) -> dict:
    """The per-element tolerances of the module docstring, keyed by OUTPUTS.  H_total: the launch's head count when `c` is a slice of it."""
    B, H, L, d = c.shape
    H = H_total or H
    dtype = c.q.dtype
    U, u = ULP[dtype], 2.0**-24
    f16 = dtype == torch.float16
    a = t.aux
    vis, act, e, pe, A = a["vis"].double(), a["act"].double(), a["e"], a["pe"], a["A"]  # vis: not -inf (the underflow terms); act: see _scores
    v, do, q, k = (x.double().abs() for x in (c.v, c.do, c.q, c.k))
    n_vis = act.sum(-1)
    Dn = t.Dn[..., None]
    rel = (2.0 * (n_vis + d + 8) * u * (1.0 + a["S_abs"]) + a["E_add"])[..., None]
    Aabs = A @ v
    sub = 2.0**-25 if f16 else 0.0
    fl = 2.0**-126  # fp32 underflow: an exponential or a product below the smallest normal is flushed to zero
    tol_o = (U + rel) * Aabs + (sub * (act @ v) + fl * (vis @ v)) / Dn + sub + fl
    err_delta = (do * tol_o).sum(-1, keepdim=True) + (d + 2) * u * (do * Aabs).sum(-1, keepdim=True)
    absdE = (a["dA"].abs() + (do * a["o"].abs()).sum(-1, keepdim=True)) / Dn
    err_dE = (err_delta + d * u * (do @ v.transpose(-1, -2))) / Dn + (2.0 * rel + 4 * u) * absdE
    absdS = absdE * pe
    R = 0.5 * U * absdS + err_dE * pe + sub * act + fl * (absdE + 1.0) * vis
    tol_dq = c.scale * (R @ k) + (n_vis[..., None] + 8) * u * c.scale * (absdS @ k) + 0.5 * U * t.dq.abs() + sub + fl
    tol_dk = c.scale * (R.transpose(-1, -2) @ q) + (L + 8) * u * c.scale * (absdS.transpose(-1, -2) @ q) + 0.5 * U * t.dk.abs() + sub + fl
    RA = (0.5 * U + 2.0 * rel + (L + 12) * u) * A + sub * act + fl * (1.0 + 1.0 / Dn) * vis
    tol_dv = RA.transpose(-1, -2) @ do + 0.5 * U * t.dv.abs() + sub + fl
    off = 1.0 - torch.eye(L, dtype=torch.float64)
    tol_dp = (off * (e * (err_dE + (L + H + 8) * u * absdE) + fl * (absdE + 1.0) * vis)).sum(dim=(1, 2))
    if dpolicy_rounded:
        tol_dp = tol_dp + 0.5 * U * t.dpolicy.abs() + sub
    return dict(out=tol_o, dq=tol_dq, dk=tol_dk, dv=tol_dv, dpolicy=tol_dp)


def _worst(g, ref, tol, dtype, rounded_dtype=None):
    """(max err / tol, that element's error in ULP of the element, its index) of one tensor; NaN / Inf gives ratio inf -- except, for a
    tensor rounded to `rounded_dtype` whose truth is beyond that dtype's largest finite value, the +-inf that rounding gives."""
    g, ref = g.double(), ref.double()
    assert g.shape == ref.shape, (g.shape, ref.shape)
    err = (g - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(err, math.inf))
    if rounded_dtype is not None and rounded_dtype != torch.float32:
        ok = torch.isinf(g) & (ref.abs() + tol >= torch.finfo(rounded_dtype).max) & (torch.sign(g) == torch.sign(ref))
        ratio = torch.where(ok, torch.zeros_like(ratio), ratio)
        err = torch.where(ok, torch.zeros_like(err), err)
    i = int(ratio.argmax())
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))
    e_i, r_i = float(err.flatten()[i]), float(ref.flatten()[i].abs())
    ulps = 0.0 if e_i == 0 else (math.inf if r_i == 0 else e_i / (ULP[dtype] * r_i))  # (of an element that is exactly 0: inf)
    return float(ratio.flatten()[i]), ulps, idx


def worst_ratios(got: dict, t: Truth, tol: dict, dtype, dpolicy_rounded=True) -> dict:
    """{output: (max err / tol, that element's error in ULP of the element, its index)}."""
    return {n: _worst(got[n], getattr(t, n), tol[n], dtype, dtype if (n == "dpolicy" and dpolicy_rounded) else None) for n in OUTPUTS}


def evaluate(c: Case, got: dict, dpolicy_rounded=True, head_chunk=16) -> dict:
    """worst_ratios of a whole launch, evaluated one batch row and `head_chunk` heads at a time (the fp64 [L,L] intermediates of a
    [2,32,520,520] launch do not fit otherwise); dpolicy's truth and tolerance are summed over the head chunks before the comparison."""
    B, H, L, d = c.shape
    dtype = c.q.dtype
    worst = {n: (0.0, 0.0, ()) for n in OUTPUTS}
    dp_t, dp_tol = torch.zeros(B, L, dtype=torch.float64), torch.zeros(B, L, dtype=torch.float64)
    for b in range(B):
        bias = None if c.bias is None else c.bias[(b if c.bias.shape[0] > 1 else 0):][:1]
        for h0 in range(0, H, head_chunk):
            hs = slice(h0, min(H, h0 + head_chunk))
            sub = Case(c.q[b:b + 1, hs], c.k[b:b + 1, hs], c.v[b:b + 1, hs], c.do[b:b + 1, hs], c.policy[b:b + 1], bias, c.causal, c.eps, c.N, c.name)
            t = truth(sub)
            tol = bound(t, sub, dpolicy_rounded=False, H_total=H)
            dp_t[b] += t.dpolicy[0]
            dp_tol[b] += tol["dpolicy"][0]
            for n in OUTPUTS[:4]:
                r = _worst(got[n][b:b + 1, hs], getattr(t, n), tol[n], dtype)
                if r[0] >= worst[n][0]:
                    worst[n] = (r[0], r[1], (b, h0 + r[2][1]) + r[2][2:])
    if dpolicy_rounded:
        dp_tol = dp_tol + 0.5 * ULP[dtype] * dp_t.abs() + (2.0**-25 if dtype == torch.float16 else 0.0)
    worst["dpolicy"] = _worst(got["dpolicy"], dp_t, dp_tol, dtype if dpolicy_rounded else torch.float32, dtype if dpolicy_rounded else None)
    return worst


def format_ratios(res: dict) -> str:
    return "; ".join(f"{n} {r:.3f} ({ul:.2g} ulp at {list(idx)})" for n, (r, ul, idx) in res.items())


def ref64(q, k, v, policy, bias, causal, eps, N, detach_max=False):
    """oracle.ref_cpu.sdpa_with_policy restated in fp64 (the restated reference exponentiates in fp32); N: the N of eps / N."""
    B, H, L, d = q.shape
    s = (q @ k.transpose(-1, -2)) / math.sqrt(d)
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).tril().logical_not(), -math.inf)
    if bias is not None:
        s = s + bias
    pol = policy.reshape(B, 1, 1, L)
    pp = pol + (1.0 - pol) * torch.eye(L, dtype=s.dtype)
    m = s.amax(-1, keepdim=True)
    a = torch.exp(s - (m.detach() if detach_max else m)) * pp
    a = (a + eps / N) / (a.sum(-1, keepdim=True) + eps)
    return a @ v


def autograd_grads(c: Case, detach_max=False):
    """(out, dq, dk, dv, dpolicy) by fp64 autograd of ref64 -- the full gradient, the one through max_j included, unless detach_max."""
    q, k, v, pol = (x.double().clone().requires_grad_(True) for x in (c.q, c.k, c.v, c.policy))
    o = ref64(q, k, v, pol, None if c.bias is None else c.bias.double(), c.causal, c.eps, c.N, detach_max)
    o.backward(c.do.double())
    return dict(out=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dpolicy=pol.grad)


def check_property(c: Case, t: Truth = None) -> str:
    """The property that makes an input worth having (attn_truth.check_property for its distributions, request 0 head 0)."""
    B, H, L, d = c.shape
    if c.name == "leak_rows":
        t = truth(c) if t is None else t
        lo, hi = int((t.Dn < 10 * c.eps).sum()), int((t.Dn > 1).sum())
        if L >= 2 * TILE:
            assert lo > 0 and hi > 0, f"leak_rows: {lo} rows with Dn < 10 eps, {hi} with Dn > 1"
        assert all(float(c.policy[:, j].abs().max()) == 0 for j in c.leak_keys)
        return f"{lo} rows with Dn < 10 eps (min {float(t.Dn.min()):.7e}), {hi} rows with Dn > 1, of {t.Dn.numel()}"
    if c.bias is not None or L < 2:
        return ""
    return at.check_property(c.name, c.q[0].transpose(0, 1), c.k[0].transpose(0, 1), c.v[0].transpose(0, 1), causal=c.causal, dtype=c.q.dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# emulation of the documented arithmetic, and mutants of it
# ------------------------------------------------------------------------------------------------------------------------------
def emulate(c: Case, mutant=None, bwd_keys=64, dpolicy_rounded=True) -> dict:
    """The kernels' documented arithmetic in fp32: 64-key tiles with an online max m and sum l of the UNROUNDED pe, P rounded to the dtype
    before P V, the leak added as (acc + c_leak sum_j v_j) / Dn, o rounded; delta from the rounded o; the backward recomputes e from the
    saved m, rounds A^T = pe / Dn and dS^T to the dtype, adds c_leak sum_i dO_i / Dn_i to dV, sums dpolicy over the heads in fp32.
    bwd_keys: keys per workgroup of the key-side backward (64: four waves, 128: eight) -- it decides which (query tile, wave) pairs a
    causal launch visits, which is where the geometry mutants live.  mutant: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    assert bwd_keys in (64, 128)
    B, H, L, d = c.shape
    dt = c.q.dtype
    rd = lambda x: x.to(dt).float()
    q, k, v, do = (x.float() for x in (c.q, c.k, c.v, c.do))
    scale, eps = torch.tensor(c.scale, dtype=torch.float32), torch.tensor(c.eps, dtype=torch.float32)
    c_leak = (eps / float(c.N)) if mutant != "leak_dropped" else torch.tensor(0.0)
    qi, kj = torch.arange(L)[:, None], torch.arange(L)[None, :]
    pol = c.policy.float()
    if mutant == "policy_one_late_last_tile" and L % TILE:
        last0 = (L // TILE) * TILE
        pol = torch.cat([pol[:, :last0], pol[:, last0 + 1:], torch.zeros(B, 1)], 1)
    self_ok = (qi == kj) & ((kj < TILE) if mutant == "self_first_tile_only" else True)
    pp = torch.where(self_ok, torch.ones(()), pol[:, None, None, :].expand(B, H, L, L))
    s = (q @ k.transpose(-1, -2)) * scale
    if c.bias is not None:
        b = c.bias.float().expand(B, 1, L, L)
        if mutant == "bias_row_stride_ignored":
            b = b[:, :, :1, :].expand(B, 1, L, L)
        s = s + b
    valid = torch.ones(L, L, dtype=torch.bool)
    if c.causal:
        valid = kj <= qi
    s = s.masked_fill(~valid, -math.inf)
    # causal launches skip what lies wholly in a wave's future; the mutants skip (or start) one step too far
    fwd_visit = torch.ones(L, L, dtype=torch.bool)
    kv_visit = torch.ones(L, L, dtype=torch.bool)
    if c.causal and mutant == "causal_skip_one_wave":
        fwd_visit = (kj // TILE) * TILE <= (qi // 16) * 16 - 16 + 15
        kv_visit = (kj // 16) * 16 + 16 <= (qi // TILE) * TILE + TILE - 1
    if c.causal and mutant == "first_qtile_one_late_128" and bwd_keys == 128:
        kv_visit = (qi // TILE) >= ((kj // 128) * 128) // TILE + 1
    # ---- forward, tile by tile
    m = torch.full((B, H, L, 1), -math.inf)
    l = torch.zeros(B, H, L, 1)
    acc = torch.zeros(B, H, L, d)
    for t0 in range(0, L, TILE):
        t1 = min(t0 + TILE, L)
        st = s[..., t0:t1].masked_fill(~fwd_visit[:, t0:t1], -math.inf)
        mn = torch.maximum(m, st.amax(-1, keepdim=True))
        ms = torch.where(torch.isneginf(mn), torch.zeros_like(mn), mn)
        alpha = torch.exp(m - ms)
        p = torch.exp(st - ms) * pp[..., t0:t1]
        l = (l if mutant == "l_not_rescaled" else l * alpha) + p.sum(-1, keepdim=True)
        acc = acc * alpha + rd(p) @ v[..., t0:t1, :]
        m = mn
    Dn = l + eps
    sumv = v.sum(-2, keepdim=True)
    o = rd((acc + c_leak * sumv) * (1.0 / Dn))
    # ---- backward
    delta = (do * o).sum(-1, keepdim=True)
    Mx, Dnb = (m, Dn) if mutant != "stats_from_head0" else (m[:, :1].expand_as(m), Dn[:, :1].expand_as(Dn))
    di = 1.0 / Dnb
    e = torch.where(valid, torch.exp(s - Mx), torch.zeros(()))
    pe = e * pp
    dE = ((do @ v.transpose(-1, -2)) - delta) * di
    dS = rd(dE * pe)
    dq = rd((dS * fwd_visit) @ k * scale)
    dSk = dS * kv_visit
    dk = rd(dSk.transpose(-1, -2) @ q * scale)
    gsum = (do * di).sum(-2, keepdim=True)
    dv = rd((rd(pe * di) * kv_visit).transpose(-1, -2) @ do + c_leak * gsum)
    keep = torch.ones(L, L) if mutant == "dpolicy_with_diagonal" else (qi != kj).float()
    dpol = (dE * e * keep * kv_visit).sum(-2).sum(1)
    if dpolicy_rounded:
        dpol = rd(dpol)
    return dict(out=o, dq=dq, dk=dk, dv=dv, dpolicy=dpol)


# ------------------------------------------------------------------------------------------------------------------------------
# Gumbel hard keep
# ------------------------------------------------------------------------------------------------------------------------------
def gumbel_inputs(n, dtype, seed=0):
    """logp, noise [n,2], prev, dkeep [n] in `dtype`: random log-probabilities and Gumbel noise with, planted round-robin, exact ties
    logp0 + g0 == logp1 + g1, one class at -inf, the noise at both extremes of -log(Exp) (Exp -> tiny: large positive; Exp large: negative),
    and zeros in prev."""
    g = torch.Generator().manual_seed(9000 + n)
    lp = torch.log_softmax(torch.randn(n, 2, generator=g), -1)
    noise = -torch.empty(n, 2).exponential_(generator=g).log()
    prev = (torch.rand(n, generator=g) > 0.25).float()
    dkeep = torch.randn(n, generator=g)
    for i in range(n):
        kind = i % 8
        if kind == 1:    # exact tie
            lp[i, 1], noise[i, 1] = lp[i, 0], noise[i, 0]
        elif kind == 2:  # tie of different summands (exact in every dtype: small dyadic numbers)
            lp[i], noise[i] = torch.tensor([-0.5, -1.5]), torch.tensor([0.25, 1.25])
        elif kind == 3:
            lp[i, i // 8 % 2] = -math.inf
        elif kind == 4:
            noise[i, 0] = -math.log(1.2e-38)   # the smallest normal fp32 draw
        elif kind == 5:
            noise[i, 1] = -math.log(88.0)      # a far tail of Exp(1)
    return lp.to(dtype), noise.to(dtype), prev.to(dtype), dkeep.to(dtype)


def gumbel_truth(lp, noise, prev, dkeep, tau):
    """fp64 of the unrounded expression y = (logp + g) / tau, s = softmax(y), on the operands as given (U: spacing of the dtype in [1, 2)).
    Decision (class 0 wins; a tie takes class 0).  The kernel, like the eager ops, rounds the sum to the dtype, the quotient by tau to
    the dtype, and the softmax to the dtype, and decides on the rounded softmax:
      slack_y = U (1 + U) (|y0| + |y1|)        each y_c moves by at most U/2 of the sum (divided by tau) plus U/2 of itself
      the decision is DETERMINED where tanh((margin - slack_y) / 2) > U + 8 * 2^-24, margin = |y0 - y1|: s_max - s_min = tanh(margin / 2), and
      the two roundings of the softmax move each side by at most U/2 (s <= 1); elsewhere either class is allowed.
    keep lies within one ULP of {0, prev}: ret0 = (hard - s0) + s0, two roundings of at most U/2 each around 1, exactly 0 otherwise.
    dprev = dkeep * ret0: tol = 1.5 U (1 + U) |dkeep| around dkeep * {0, 1}  (ret0's U, the store's U/2).
    dlogp_c = dy0 s_0 ((c == 0) - s_c) / tau with dy0 = dkeep * prev, relative to G = |dy0| max(s0, s1) / tau (NOT to |dlogp_c|: 1 - s0 is
    formed from the rounded s0, an absolute error of U/2 s0):  tol = (2.5 U + 2 slack_y + 8 * 2^-24) G  -- the four roundings of
    tp_gumbel_bwd_kernel (dy0; the product; the quotient by tau, whose store is exact) and the saved y_soft's own (as the factor and inside
    dot), U/2 each; |d s_c| <= s_c slack_y from the rounded y, entering twice; fp32 operations.  f16: + 2^-25 (1 + |dy0| / tau), the fixed
    quantum of a subnormal s_c or result."""
    dt = lp.dtype
    U = ULP[dt]
    y = (lp.double() + noise.double()) / tau
    finite = torch.isfinite(y)
    ya = torch.where(finite, y.abs(), torch.zeros_like(y))
    slack = U * (1.0 + U) * (ya[:, 0] + ya[:, 1])
    margin = torch.where(finite.all(1), (y[:, 0] - y[:, 1]).abs(), torch.full_like(slack, math.inf))
    determined = torch.tanh((margin - slack).clamp_min(0.0) / 2) > U + 8 * 2.0**-24
    dec0 = y[:, 0] >= y[:, 1]
    s = torch.softmax(y, -1)
    p, dk = prev.double(), dkeep.double()
    dy0 = dk * p
    dlogp = torch.stack([s[:, 0] * (dy0 - dy0 * s[:, 0]), s[:, 1] * (0.0 - dy0 * s[:, 0])], 1) / tau
    G = (dy0.abs() * s.amax(-1) / tau)[:, None]
    sub = 2.0**-25 if dt == torch.float16 else 0.0
    tol_dlogp = (2.5 * U + 2.0 * slack[:, None] + 8 * 2.0**-24) * G + sub * (1.0 + dy0.abs()[:, None] / tau)
    tol_dprev = 1.5 * U * (1.0 + U) * dk.abs() + sub
    return dict(dec0=dec0, determined=determined, margin=margin, slack=slack, dlogp=dlogp, tol_dlogp=tol_dlogp.expand(-1, 2), tol_dprev=tol_dprev, s=s)
