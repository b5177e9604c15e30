"""Truth, hard rows and the acceptance criterion for the row-wise family: every launch that normalises a row or applies an activation (csrc/elementwise.hip,
csrc/gemv_prologue.h, the activation epilogues).  docs/rowwise_exactness.md has the construction and the measured figures.

The kernels are specified by their rounding points (include/dynllava.h, oracle/ref_cpu.py):

  RMSNorm     r = rsqrt(mean(x^2) + eps) in fp32;  out = RNE_T(w * RNE_T(x * r))          (the cast first, then the weight: an exact fp32 product, one rounding)
  LayerNorm   out = RNE_T((x - mu) * r * w + b) evaluated in fp32
  silu_mul    out = RNE_T(RNE_T(g / (1 + exp(-g))) * u)
  quick_gelu  out = RNE_T(x * RNE_T(sigmoid(RNE_T(1.702 x))))

The only freedom a correct kernel has is the fp32 value of its statistic (summation order, rsqrtf, expf, the divide).  So the expectation is not a tolerance
but, per element, the SET of values the specification produces when that fp32 quantity lies within a relative rho of its fp64 truth.  Every step after the
statistic is monotone in it, so the set is spanned by its two ends: `decided` elements (both ends round alike) must equal that value, the others must
equal one of the two.  For fp32 the interval itself is kept, |out - v| <= e.

rho:  lattice rows have statistics that are exact in fp32 in any order (sums of small integers times one power of two), so rho covers only `/ H`, `+ eps`
and rsqrtf: RHO_LATTICE = 2^-22, four fp32 ulps.  Generic rows depend on the summation order: RHO_GENERIC is four times the largest deviation measured on the
CPU over the whole case table in two fp32 orders that belong to no kernel (measure_rho_rms / measure_rho_ln; tests/test_rowwise_truth_cpu.py re-derives it).  RHO_ACT and
GELU_ABS are measured the same way against torch's fp32 exp / erf."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from oracle import linear_truth as lt

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
U32 = 2.0**-24                 # half an fp32 ulp, relative: the error of one fp32 rounding
TINY32 = 2.0**-149             # the fp32 subnormal quantum: the absolute error of one fp32 rounding near zero
FLT_MAX = 3.4028234663852886e38
RHO_LATTICE = 2.0**-22
# measured on the CPU (docs/rowwise_exactness.md, "Measured"): 4 x the largest deviation, rounded up to two digits, floored at 2^-22
RHO_GENERIC = 8.6e-7           # 4 x 2.14e-7 (LayerNorm r, fp16, H = 16384 after a residual add)
RHO_ACT = 5.6e-7               # 4 x 1.38e-7 (fp16 gates)
GELU_ABS = 1.2e-6              # absolute, in units of |x|: erff carries an absolute error
VEC = {BF16: 8, F16: 8, F32: 4}  # elements of a 16-byte vector


def eps32(eps):
    return float(torch.tensor(eps, dtype=F32).double())


def to_t(t64, dtype):
    """fp64 -> fp32 -> dtype, both RNE: what a kernel does with an fp32 expression, and monotone."""
    return t64.to(F32).to(dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# the criterion
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Feasible:
    """16-bit: the two ends lo / hi (either order).  fp32: v +- e.  NaN in lo means the specification gives NaN there."""
    dtype: torch.dtype
    lo: torch.Tensor = None
    hi: torch.Tensor = None
    v: torch.Tensor = None
    e: torch.Tensor = None
    between: bool = False  # an absolute error that can span more than two 16-bit values (GELU's tail): lo <= out <= hi

    @property
    def shape(self):
        return self.lo.shape if self.lo is not None else self.v.shape

    def ok(self, out):
        out = out.detach().cpu()
        if self.lo is None:
            return (out.double() - self.v).abs() <= self.e
        nan = torch.isnan(self.lo)
        hit = ((out >= self.lo) & (out <= self.hi)) if self.between else ((out == self.lo) | (out == self.hi))
        return torch.where(nan, torch.isnan(out), hit)

    def undecided(self):
        """Share of elements whose two ends differ (fp32: 0 by definition -- the interval is the criterion)."""
        if self.lo is None:
            return 0.0
        return float(((self.lo != self.hi) & ~torch.isnan(self.lo)).double().mean())

    def rows(self, idx):
        pick = lambda t: None if t is None else t[idx]
        return Feasible(self.dtype, pick(self.lo), pick(self.hi), pick(self.v), pick(self.e), self.between)


def stack(fs):
    cat = lambda k: None if getattr(fs[0], k) is None else torch.cat([getattr(f, k) for f in fs], 0)
    return Feasible(fs[0].dtype, cat("lo"), cat("hi"), cat("v"), cat("e"), fs[0].between)


def rms_truth(h, w, eps, rho) -> Feasible:
    """h [R, H] (the residual stream after the add, model dtype), w [H]."""
    dt = h.dtype
    x = h.double()
    r = 1.0 / torch.sqrt(x.pow(2).mean(-1, keepdim=True) + eps32(eps))
    wd = w.double()
    if dt == F32:
        v = wd * x * r
        return Feasible(dt, v=v, e=v.abs() * (rho + 3 * U32) + 2 * TINY32)
    ends = [to_t(wd * to_t(x * (r * s), dt).double(), dt) for s in (1.0 - rho, 1.0 + rho)]
    return Feasible(dt, lo=ends[0], hi=ends[1])


def ln_truth(h, w, b, eps, rho, exact_mean=False) -> Feasible:
    """exact_mean: a lattice row, whose fp32 mean is the true one in any order (asserted by the generator)."""
    dt = h.dtype
    x = h.double()
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    r = 1.0 / torch.sqrt(d.pow(2).mean(-1, keepdim=True) + eps32(eps))
    wd, bd = w.double(), b.double()
    v = d * r * wd + bd
    dmu = 0.0 if exact_mean else rho * x.abs().mean(-1, keepdim=True)
    # rho on r; the mean's error; the roundings of x - mean, * r, * w (each relative to its own intermediate) and of the sum
    e = (d.abs() * r * wd.abs()) * (rho + 3 * U32) + dmu * r * wd.abs() + v.abs() * U32 + 2 * TINY32
    e = e * (1 + 2.0**-10)  # second-order terms
    if dt == F32:
        return Feasible(dt, v=v, e=e)
    return Feasible(dt, lo=to_t(v - e, dt), hi=to_t(v + e, dt), between=True)


def exp_overflows(g64):
    """-> (overflow, edge): expf(-g) is +inf in fp32 / within 2^-20 of the threshold, where one ulp of expf decides (no 16-bit value lies there)."""
    with_edge = torch.exp(-g64.clamp(min=-745.0))
    return with_edge > FLT_MAX * (1 + 2.0**-20), (with_edge > FLT_MAX * (1 - 2.0**-20)) & (with_edge <= FLT_MAX * (1 + 2.0**-20))


def silu64(g64):
    return g64 * torch.sigmoid(g64)


def _act_ends(s64, dtype, rho):
    return [to_t(s64 * (1.0 - rho), dtype), to_t(s64 * (1.0 + rho), dtype)]


def silu_mul_truth(g, u, rho=None) -> Feasible:
    """g, u: model dtype, same shape.  Where the fp32 expression itself overflows (expf(-g) = inf, g < -88.72) the specified value is g / inf = -0."""
    rho = RHO_ACT if rho is None else rho
    dt = g.dtype
    g64, u64 = g.double(), u.double()
    over, edge = exp_overflows(g64)
    s = torch.where(over, torch.zeros_like(g64), silu64(g64))
    finite = torch.isfinite(g64)
    if dt == F32:
        v = s * u64
        e = v.abs() * (rho + 2 * U32) + TINY32 * (1 + u64.abs())
        e = torch.where(edge, e + (silu64(g64) * u64).abs(), e)
        return Feasible(dt, v=torch.where(finite, v, torch.zeros_like(v)), e=torch.where(finite, e, torch.full_like(e, float("inf"))))
    assert not bool(edge.any())
    lo, hi = [to_t(a.double() * u64, dt) for a in _act_ends(s, dt, rho)]
    return Feasible(dt, lo=lo, hi=hi)


def quick_gelu_truth(x, rho=None) -> Feasible:
    rho = RHO_ACT if rho is None else rho
    dt = x.dtype
    x64 = x.double()
    c = float(torch.tensor(1.702, dtype=F32).double())
    t = to_t(x64 * c, dt).double()  # RNE_T(1.702f * x): the fp32 product of two fp32 values, rounded to fp32 and then to T -- no freedom
    over, edge = exp_overflows(t)
    sg = torch.where(over, torch.zeros_like(t), torch.sigmoid(t))
    if dt == F32:
        v = x64 * sg
        e = v.abs() * (rho + 2 * U32) + TINY32 * (1 + x64.abs())
        e = torch.where(edge, e + (x64 * torch.sigmoid(t)).abs(), e)
        fin = torch.isfinite(x64)
        return Feasible(dt, v=torch.where(fin, v, torch.zeros_like(v)), e=torch.where(fin, e, torch.full_like(e, float("inf"))))
    assert not bool(edge.any())
    lo, hi = [to_t(x64 * a.double(), dt) for a in _act_ends(sg, dt, rho)]
    return Feasible(dt, lo=lo, hi=hi)


def gelu_truth(x, bound=None) -> Feasible:
    """x Phi(x) in fp64; |error| <= bound |x| absolute (erff's error is absolute), then one rounding."""
    bound = GELU_ABS if bound is None else bound
    dt = x.dtype
    x64 = x.double()
    v = 0.5 * x64 * (1.0 + torch.erf(x64 / math.sqrt(2.0)))
    e = bound * x64.abs() + v.abs() * U32 + TINY32
    if dt == F32:
        return Feasible(dt, v=v, e=e)
    return Feasible(dt, lo=to_t(v - e, dt), hi=to_t(v + e, dt), between=True)


# ------------------------------------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------------------------------------
def norm_weight(H, seed=0):
    """k / 128, k in [128, 256): a full 8-bit mantissa in every dtype."""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(128, 256, (H,), generator=g).double() / 128


def norm_bias(H, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randint(-64, 64, (H,), generator=g).double() / 128


RMS_LATTICE_KINDS = ("int", "int_small", "int_outlier", "zero", "last_only")
RMS_GENERIC_KINDS = ("randn3", "outlier", "small", "tiny")
LN_LATTICE_KINDS = ("balanced", "balanced_small", "constant", "int_outlier")
LN_GENERIC_KINDS = ("randn3", "outlier", "small", "tiny", "offset")
OFFSET = {BF16: (32.0, 1.0), F16: (64.0, 1.0), F32: (1000.0, 1.0)}  # mu, sigma: bf16's grid at mu has a quarter-sigma spacing (fp16: 1 / 16)


def _ints(H, g):
    s = torch.randint(0, 2, (H,), generator=g).double() * 2 - 1
    return s * torch.randint(1, 4, (H,), generator=g).double()


def rms_lattice_rows(H, dtype, seed=0):
    """[5, H] fp64, all exactly `dtype` values; the sums of squares are exact in fp32 in any order (asserted)."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for kind in RMS_LATTICE_KINDS:
        x = _ints(H, g)
        if kind == "int_small":
            x = x * 2.0**-10  # mean square <= 9 x 2^-20 < eps: losing eps shows in every element
        elif kind == "int_outlier":
            x[-1] = 1024.0
        elif kind == "zero":
            x = torch.zeros(H, dtype=torch.float64)
        elif kind == "last_only":  # a dropped tail shows through rstd = rsqrt(eps)
            x = torch.zeros(H, dtype=torch.float64)
            x[-1] = 3.0
        rows.append(x)
    x = torch.stack(rows)
    assert_sums_exact(x.pow(2))
    assert torch.equal(x.to(dtype).double(), x)
    return x


def assert_sums_exact(t):
    """Every row of t is integers times one power of two with sum |t| < 2^24 quanta: any fp32 summation order gives the true sum."""
    for row in t:
        nz = row[row != 0].abs()
        if nz.numel() == 0:
            continue
        q = 2.0 ** math.floor(math.log2(float(nz.min())))
        while not bool((row / q == (row / q).round()).all()):
            q /= 2
            assert q > 2.0**-60
        assert float((row / q).abs().sum()) < 2**24, "partial sums may round"


def ln_lattice_rows(H, dtype, seed=0):
    """[4, H]: integer rows whose mean is exactly 1/4 (H % 4 == 0), one scaled by 2^-10, the constant row 3 (the output is b), one with a 1024 outlier and mean 1/4."""
    assert H % 4 == 0
    g = torch.Generator().manual_seed(seed)
    rows = []
    for kind in LN_LATTICE_KINDS:
        if kind == "constant":
            rows.append(torch.full((H,), 3.0, dtype=torch.float64))
            continue
        x = _ints(H, g)
        if kind == "int_outlier" and H > 1024:
            x[-1] = 128.0  # (x - 1/4)^2 in sixteenths stays below 2^24 over the row
        # move single elements by +-1 (staying in [-3, 3]) until the sum is H / 4
        want = H // 4
        diff = int(want - x.sum())
        i = 0
        while diff != 0:
            step = 1 if diff > 0 else -1
            if abs(x[i] + step) <= 3 and i != H - 1:
                x[i] += step
                diff -= step
            i = (i + 1) % H
        if kind == "balanced_small":
            x = x * 2.0**-10
        rows.append(x)
    x = torch.stack(rows)
    mu = x.mean(-1, keepdim=True)
    assert torch.equal(mu.float().double(), mu)
    assert_sums_exact(x)
    assert_sums_exact((x - mu).pow(2))
    assert torch.equal(x.to(dtype).double(), x)
    return x


def generic_rows(H, dtype, kinds, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    rows = []
    for kind in kinds:
        x = torch.randn(H, generator=g, dtype=torch.float64)
        if kind == "randn3":
            x = 3 * x
        elif kind == "outlier":
            x[0], x[H - 1], x[H // 2] = 2000.0, -1500.0, 900.0
        elif kind == "small":
            x = 1e-3 * x
        elif kind == "tiny":
            x = 2.0**-16 * x  # fp16: subnormal outputs
        elif kind == "offset":
            mu, sigma = OFFSET[dtype]
            x = mu + sigma * x
        rows.append(x)
    return torch.stack(rows).to(dtype).double()


def split_add(x, dtype, seed=0, scale_rows=None):
    """h0, delta (model dtype values, fp64) with RNE_T(h0 + delta) == x exactly: delta in {-2..2} x the row's quantum where x is an integer multiple of
    it, 0 elsewhere (generic rows get a generic delta in make_add_generic)."""
    g = torch.Generator().manual_seed(300 + seed)
    q = torch.ones(x.shape[0], 1, dtype=torch.float64) if scale_rows is None else scale_rows
    d = torch.randint(-2, 3, x.shape, generator=g).double() * q
    big = x.abs() > 64 * q
    d = torch.where(big, x / 2, d)  # an outlier is split in halves (its neighbours on the 16-bit grid are too coarse for +-1)
    h0 = x - d
    assert torch.equal(h0.to(dtype).double(), h0) and torch.equal(d.to(dtype).double(), d)
    assert torch.equal(to_t(h0 + d, dtype).double(), x)
    return h0, d


def split_parts(delta, n, seed=0, quantum=None):
    """delta [R, H] -> fp32 parts [n, R, H] of integers (times the row's quantum) whose sum in slice order is exactly delta."""
    g = torch.Generator().manual_seed(400 + seed)
    q = torch.ones(delta.shape[0], 1, dtype=torch.float64) if quantum is None else quantum
    p = torch.randint(-4, 5, (n,) + tuple(delta.shape), generator=g).double() * q
    p[-1] = delta - p[:-1].sum(0)
    acc = torch.zeros(delta.shape, dtype=F32)
    for s in range(n):
        acc = acc + p[s].float()
    assert torch.equal(acc.double(), delta) and torch.equal(p.float().double(), p)
    return p.float()


def row_quantum(x):
    """[R, 1]: the power of two every element of the row is an integer multiple of (1 for a zero row)."""
    out = []
    for row in x:
        q = 1.0
        while not bool((row / q == (row / q).round()).all()):
            q /= 2
        out.append(q)
    return torch.tensor(out, dtype=torch.float64)[:, None]


# ------------------------------------------------------------------------------------------------------------------------------
# the specified arithmetic in fp32 (oracle/ref_cpu.py's expressions), with the mutants
# ------------------------------------------------------------------------------------------------------------------------------
def fp32_sum_orders(t32):
    """Row sums of t32 [R, H] in two fp32 orders that belong to no kernel: torch.sum, and 256 strided lanes followed by a pairwise tree."""
    R, H = t32.shape
    pad = (-H) % 256
    z = torch.cat([t32, torch.zeros(R, pad, dtype=F32)], 1).view(R, -1, 256)
    lanes = torch.zeros(R, 256, dtype=F32)
    for i in range(z.shape[1]):
        lanes = lanes + z[:, i]
    while lanes.shape[1] > 1:
        lanes = lanes[:, 0::2] + lanes[:, 1::2]
    return [t32.sum(-1, keepdim=True), lanes]


def rstd_rms_fp32(h, eps, order):
    x = h.float()
    return torch.rsqrt(fp32_sum_orders(x * x)[order] / float(h.shape[-1]) + eps)


def stats_ln_fp32(h, eps, order):
    x = h.float()
    H = float(h.shape[-1])
    mean = fp32_sum_orders(x)[order] / H
    d = x - mean
    return mean, torch.rsqrt(fp32_sum_orders(d * d)[order] / H + eps)


RMS_MUTANTS = ("weight_before_cast", "truncated_store", "rstd_16bit", "padded_count", "eps_lost", "eps_outside_root", "last_vector_dropped", "reread_vector0_counted")
PARTS_MUTANTS = ("slice_dropped_at_batch", "slice_twice_at_batch")
LN_MUTANTS = ("one_pass_variance", "extra_rounding_before_affine", "truncated_store", "padded_count", "eps_lost", "last_vector_dropped", "reread_vector0_counted")
ACT_MUTANTS = ("silu_no_inner_rounding", "fast_silu_unguarded", "truncated_store")
PASS_VECS = 256  # a pass of the block-per-row kernels: 256 lanes x one 16-byte vector


def _trunc(t32, dt):
    return lt.truncate(t32.double(), dt) if dt != F32 else t32


def emulate_rmsnorm(h, w, eps, mutant=None, order=0):
    """oracle/ref_cpu.py's RMSNorm on h [R, H] (model dtype), the sum taken in fp32 order `order`; `mutant` alters one step."""
    dt, H, V = h.dtype, h.shape[-1], VEC[h.dtype]
    x = h.float()
    sq = x * x
    count = float(H)
    if mutant == "last_vector_dropped":
        sq = sq[:, : H - V]
    ss = fp32_sum_orders(sq)[order]
    if mutant == "padded_count":
        count = float(-(-H // (PASS_VECS * V)) * PASS_VECS * V)
    if mutant == "reread_vector0_counted":  # the lanes of the last pass that hold no vector re-read vector 0 and add it
        ss = ss + float((-(H // V)) % PASS_VECS) * sq[:, :V].sum(-1, keepdim=True)
    ms = ss / count
    if mutant == "eps_lost":
        r = torch.rsqrt(ms)
    elif mutant == "eps_outside_root":
        r = 1.0 / (torch.sqrt(ms) + eps)
    else:
        r = torch.rsqrt(ms + eps)
    if mutant == "rstd_16bit" and dt != F32:
        r = r.to(dt).float()
    elif mutant == "rstd_16bit":
        r = r.to(BF16).float()
    if mutant == "weight_before_cast":
        return (w.float() * (x * r)).to(dt)
    out = w.float() * (x * r).to(dt).float()
    return _trunc(out, dt) if mutant == "truncated_store" else out.to(dt)


def emulate_add_parts(h0, parts, mutant=None, batch=8):
    """h = RNE_T(h0 + RNE_T(sum of parts in slice order)); the mutants lose / repeat the first slice of the second batch."""
    dt = h0.dtype
    acc = torch.zeros(h0.shape, dtype=F32)
    for s in range(parts.shape[0]):
        if mutant == "slice_dropped_at_batch" and s == batch:
            continue
        acc = acc + parts[s]
        if mutant == "slice_twice_at_batch" and s == batch:
            acc = acc + parts[s]
    return (h0.float() + acc.to(dt).float()).to(dt)


def emulate_layernorm(h, w, b, eps, mutant=None, order=0):
    dt, H, V = h.dtype, h.shape[-1], VEC[h.dtype]
    x = h.float()
    count = float(H)
    if mutant == "padded_count":
        count = float(-(-H // (64 * V)) * 64 * V)  # a pass of the wave-per-row kernel
    xs = x[:, : H - V] if mutant == "last_vector_dropped" else x
    s = fp32_sum_orders(xs)[order]
    pad = float((-(H // V)) % 64)
    if mutant == "reread_vector0_counted":
        s = s + pad * x[:, :V].sum(-1, keepdim=True)
    mean = s / count
    if mutant == "one_pass_variance":
        var = fp32_sum_orders(x * x)[order] / count - mean * mean
    else:
        d = xs - mean
        q = fp32_sum_orders(d * d)[order]
        if mutant == "reread_vector0_counted":
            q = q + pad * ((x[:, :V] - mean) ** 2).sum(-1, keepdim=True)
        var = q / count
    r = torch.rsqrt(var) if mutant == "eps_lost" else torch.rsqrt(var + eps)
    if mutant == "extra_rounding_before_affine":
        out = ((x - mean) * r).to(dt).float() * w.float() + b.float()
    else:
        out = (x - mean) * r * w.float() + b.float()
    return _trunc(out, dt) if mutant == "truncated_store" else out.to(dt)


def emulate_silu_mul(g, u, mutant=None):
    dt = g.dtype
    s = torch.nn.functional.silu(g.float())
    if mutant == "fast_silu_unguarded":
        s = s * (1.0 + 2.0**-20)
    if mutant == "silu_no_inner_rounding":
        return (s * u.float()).to(dt)
    out = s.to(dt).float() * u.float()
    return _trunc(out, dt) if mutant == "truncated_store" else out.to(dt)


def emulate_quick_gelu(x):
    dt = x.dtype
    xf = x.float()
    return (xf * torch.sigmoid((1.702 * xf).to(dt).float()).to(dt).float()).to(dt)


# ------------------------------------------------------------------------------------------------------------------------------
# every 16-bit input
# ------------------------------------------------------------------------------------------------------------------------------
def all_values(dtype):
    """All 65 536 bit patterns of a 16-bit dtype, in bit order."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def up_values(dtype):
    one = torch.ones((), dtype=dtype)
    ulp = float(torch.finfo(dtype).eps)
    return torch.tensor([1.0, -1.0, 1.0 + ulp, 3.0, 0.333, 100.0, 2.0**-14, 0.0], dtype=torch.float64).to(dtype) * one


def fp32_gates():
    """2^20 gates in [-110, 110], then +-2^k for k down to -140 (fp32 subnormals), padded to a multiple of 8."""
    sweep = torch.linspace(-110.0, 110.0, 2**20, dtype=torch.float64).float()
    k = torch.arange(-140, 7, dtype=torch.float64)
    pw = torch.cat([2.0**k, -(2.0**k)]).float()
    g = torch.cat([sweep, pw])
    return torch.cat([g, torch.zeros((-g.numel()) % 8, dtype=F32)])


# ------------------------------------------------------------------------------------------------------------------------------
# measuring rho
# ------------------------------------------------------------------------------------------------------------------------------
def measure_rho_rms(rows):
    """Largest |r32 / r* - 1| over the rows (model-dtype tensor [R, H]) and the two orders."""
    x = rows.double()
    r = 1.0 / torch.sqrt(x.pow(2).mean(-1, keepdim=True) + eps32(1e-5))
    return max(float((rstd_rms_fp32(rows, 1e-5, o).double() / r - 1).abs().max()) for o in (0, 1))


def measure_rho_ln(rows):
    """-> (deviation of r, deviation of the mean in units of mean|x|)."""
    x = rows.double()
    mu = x.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps32(1e-5))
    dr = dm = 0.0
    for o in (0, 1):
        m32, r32 = stats_ln_fp32(rows, 1e-5, o)
        dr = max(dr, float((r32.double() / r - 1).abs().max()))
        dm = max(dm, float(((m32.double() - mu).abs() / x.abs().mean(-1, keepdim=True).clamp_min(1e-300)).max()))
    return dr, dm


def measure_rho_act(dtype):
    """Largest relative deviation of torch's fp32 g / (1 + exp(-g)) and 1 / (1 + exp(-t)) from fp64 over every finite value of a 16-bit dtype (outside
    the overflow zone and fp32-subnormal results)."""
    g = all_values(dtype)
    g = g[torch.isfinite(g.float())].float()
    g64 = g.double()
    over, _ = exp_overflows(g64)
    worst = 0.0
    for f32, f64 in ((g / (1.0 + torch.exp(-g)), silu64(g64)), (1.0 / (1.0 + torch.exp(-g)), torch.sigmoid(g64))):
        keep = ~over & (f64.abs() > 2.0**-120)
        worst = max(worst, float((f32.double()[keep] / f64[keep] - 1).abs().max()))
    return worst


def measure_gelu_abs(dtype):
    """Largest |torch fp32 GELU - x Phi(x)| / |x| over every finite non-zero value of a 16-bit dtype."""
    x = all_values(dtype)
    x = x[torch.isfinite(x.float()) & (x.float() != 0) & (x.float().abs() <= 65504.0)].float()  # (torch's CPU kernel overflows above 1.7e38)
    x64 = x.double()
    v = 0.5 * x64 * (1.0 + torch.erf(x64 / math.sqrt(2.0)))
    return float(((torch.nn.functional.gelu(x).double() - v).abs() / x64.abs()).max())
