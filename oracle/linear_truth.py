"""Integer-lattice inputs for the GEMM / GEMV kernels, their fp64 truth and the one bit pattern the header allows (CPU only, plain torch).

Used by tests/test_linear_truth_cpu.py (an emulation of the specified arithmetic returns `expected` exactly, small mutants of it do not, and
the same mutants pass the tolerances of the older tests on gaussian inputs) and by oracle/linear_cases.py / tests/test_linear_exact_gpu.py
(every kernel instantiation of the linear family against `expected` with torch.equal).  docs/linear_exactness.md is the write-up.

Why there is exactly one answer
-------------------------------
include/dynllava.h promises "fp32 accumulation, one rounding" for dl_linear, dl_linear_splitk, dl_gemv, dl_gemm_smallm, dl_linear_packed,
dl_linear_tiles, dl_gemv_mx8 and dl_gemm_mx8.  Every operand here is a small integer times a power of two, so
  * every product x w is exact in fp32 (two short significands);
  * with q the smallest non-zero |x w| of a case, every partial sum of any subset of the terms, in any order, is an integer multiple of q
    below 2^24 q (premise (i): sum_k |x||w| < 2^24 q for every output) -- exactly representable in fp32.  However a kernel tiles, splits,
    interleaves or reduces K, its fp32 accumulators hold exact values, and the fp32 partial sums of a k range equal the truth of that range;
  * "one rounding" is then RNE(truth) bit for bit, and the tolerance is zero.  No constant is fitted.

Families (make_case; each asserts its premises (i)-(iv) in check_premises)
--------------------------------------------------------------------------
small_a   sparse x in {-1, 0, 1}, dense w in {+-1, +-2}; small_b: dense x in {+-1, +-2}, sparse w in {-1, 0, 1}.  Every output is an integer of
          at most 256 (bf16) / 2048 (fp16) / 2^24 (fp32): exactly representable, so one missing, doubled or misplaced term changes the output bits.
          The non-zeros of the sparse operand are dealt to its rows in priority order: k = 0, k = K - 1 and both sides of every cut point the caller
          names (k-slice / k-range bounds), then both sides of every multiple of 256, 128, 64, 32 and 8, then the rest -- so the boundaries are
          occupied first when the row budget cannot cover all of K.  Between small_a and small_b every x and every w element meets a non-zero partner.
wide      dense x in {+-1, +-2}, dense w in {+-1, +-2, +-3}, one outlier activation channel x[:, c] = 1024 (w[:, c] in {+-2, +-3}): sums of a few
          thousand, most of them not representable in 16 bits, some exact ties.  Makes every rounding visible.  (fp32 outputs: nothing rounds,
          expected = truth; the family still checks every term.)  The prologue cases, whose x cannot carry it, put the large factor into a weight
          column instead.
outlier   small_a with x[:, c] = +-1024 and the weight column c thinned to one row in eight: those outputs are rounded, their neighbours stay in the
          exactly-representable regime (exact_mask) beside an operand 1024 times larger.
blockscale (MXFP8) any of the above with every 32-block of every weight row multiplied by its own 2^e, e over 9 binades [-4, 4], different between
          neighbouring blocks and neighbouring rows; every value is e4m3fn x E8M0 (the host quantiser round-trips the matrix, asserted).

Prologues / epilogues kept exact by construction: integer bias and residual (expected = RNE(resid + RNE(truth + bias)), the rounding points of
dl_linear / dl_linear_packed / dl_linear_tiles); ADDNORM with h + delta in {+-1} (mean square 1, hn rsqrt(1 + eps) rounds to +-1 in 16 bits) and norm
weights in {0, +-1, +-2}; SILUMUL with gates in {0, 16, 32} (silu(g) rounds to g in 16 bits, asserted against oracle/ref_cpu.py's expression); SiLU-pair
epilogues with four hot columns a row whose gate weights cancel to {0, 16, 32} (a short reduction, exact outputs: the full-K reduction and a rounding store of
those instantiations are NOT exercised).  GELU / QuickGELU epilogues are left to the older tests.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

LIMIT = {torch.bfloat16: 256, torch.float16: 2048, torch.float32: 2**24}  # integers up to here are exactly representable
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11, torch.float32: 24}
FAMILIES = ("small_a", "small_b", "wide", "outlier")
OUTLIER = 1024.0
E_RANGE = (-4, 4)  # blockscale: 9 binades


# ------------------------------------------------------------------------------------------------------------------------------
# rounding, representability
# ------------------------------------------------------------------------------------------------------------------------------
def rne(t64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp64 -> dtype with ONE round-to-nearest-even.  torch converts fp64 -> 16 bits through fp32; the lattice values are exact in fp32 (asserted), so
    the fp32 -> 16-bit conversion is the only rounding."""
    f = t64.to(torch.float32)
    assert torch.equal(f.double(), t64), "truth is not exact in fp32: premise (i) is violated"
    return f.to(dtype)


def _scaled_sig(t64, bits):
    m, _ = torch.frexp(t64.abs())  # |t| = m 2^e, m in [0.5, 1)
    return m * float(2**bits)


def representable(t64, dtype):
    """Elementwise: t64 is exactly a `dtype` value (normal range; the lattice stays far from the subnormals and from overflow)."""
    s = _scaled_sig(t64, SIG_BITS[dtype])
    return s == s.round()


def is_tie(t64, dtype):
    """Elementwise: t64 lies exactly halfway between two neighbouring `dtype` values."""
    s = _scaled_sig(t64, SIG_BITS[dtype] + 1)
    return (s == s.round()) & (s.round() % 2 == 1)


def truncate(t64, dtype):
    """fp64 -> dtype rounded toward zero (the truncation mutant)."""
    r = rne(t64, dtype).double()
    over = r.abs() > t64.abs()
    bits = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}[dtype]
    down = (rne(t64, dtype).view(bits) - 1).view(dtype)  # one step toward zero in sign-magnitude
    return torch.where(over, down, rne(t64, dtype))


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class LinearCase:
    family: str
    dtype: torch.dtype
    x: torch.Tensor                  # [M, K] model dtype, as the kernel reads it
    w: torch.Tensor                  # [N, K] model dtype (for MXFP8: the exactly quantisable matrix)
    bias: torch.Tensor | None = None   # [N] model dtype, integers
    resid: torch.Tensor | None = None  # [M, N] model dtype, integers
    exact_mask: torch.Tensor | None = None  # [M, N] bool: outputs meant to be exactly representable (regime "mixed")
    regime: str | None = None  # what check_premises asserts of the outputs: "exact" (ii), "mixed" (ii on exact_mask), "rounding" (iii), None (only (i) / (iv))
    cuts: tuple = ()
    extra: dict = field(default_factory=dict)  # prologue operands (h_in, delta, norm_w, gate_up, ...)

    @property
    def truth(self) -> torch.Tensor:
        return self.x.double() @ self.w.double().T

    def part_truth(self, k0: int, k1: int) -> torch.Tensor:
        """fp64 truth of the k range [k0, k1): what an fp32 partial-sum buffer of that range must hold, exactly."""
        return self.x[:, k0:k1].double() @ self.w[:, k0:k1].double().T

    def expected(self, dtype: torch.dtype | None = None) -> torch.Tensor:
        """RNE(truth) (fp32: the truth); with bias / residual RNE(resid + RNE(truth + bias)), the rounding points the header states."""
        dt = self.dtype if dtype is None else dtype
        t = self.truth
        if self.bias is not None:
            t = t + self.bias.double()[None, :]
        y = rne(t, dt)
        if self.resid is not None:
            y = rne(self.resid.double() + y.double(), dt)
        return y

    def expected_parts(self, bounds) -> torch.Tensor:
        """fp32 [len(bounds), M, N]: the exact truth of every k range."""
        return torch.stack([rne(self.part_truth(k0, k1), torch.float32) for k0, k1 in bounds])


def _priority(K, cuts, g):
    """All k in [0, K) in the order the sparse operand occupies them (see the module docstring)."""
    seen, order = set(), []

    def add(k):
        if 0 <= k < K and k not in seen:
            seen.add(k)
            order.append(k)

    add(0)
    add(K - 1)
    for c in sorted(set(int(c) for c in cuts)):
        add(c - 1)
        add(c)
    for step in (256, 128, 64, 32, 8):
        for c in range(step, K, step):
            add(c - 1)
            add(c)
    rest = [k for k in torch.randperm(K, generator=g).tolist() if k not in seen]
    return order + rest


def _sparse(R, K, per_row, cuts, g, values=(-1.0, 1.0)):
    """[R, K] with per_row non-zeros a row, dealt round-robin in priority order: the union over the rows covers the first R * per_row priorities."""
    prio = _priority(K, cuts, g)
    out = torch.zeros(R, K, dtype=torch.float64)
    vals = torch.tensor(values, dtype=torch.float64)
    start = int(torch.randint(0, R, (1,), generator=g))
    for r in range(R):
        ks = [prio[i % K] for i in range((r + start) % R, R * per_row, R)][:per_row]
        ks = sorted(set(ks))
        out[r, ks] = vals[torch.randint(0, len(vals), (len(ks),), generator=g)]
    return out


def _dense(R, K, values, g):
    vals = torch.tensor(values, dtype=torch.float64)
    return vals[torch.randint(0, len(vals), (R, K), generator=g)]


def _budget(dtype, x_abs, w_abs, K, rows):
    """Non-zeros per row of the sparse operand: enough to cover K over `rows` rows where sum |x||w| <= LIMIT allows it, else the guaranteed maximum."""
    cap = max(1, int(LIMIT[dtype] // (x_abs * w_abs)))
    need = -(-K // rows)
    return min(K, need if need <= cap else cap), need <= cap


def make_case(family, M, N, K, dtype, seed=0, cuts=(), bias=False, resid=False, force_cover=False) -> LinearCase:
    """A seeded case of `family` at [M, K] x [N, K].
    force_cover (small_b at a K too long for the guaranteed budget): deal enough non-zeros to cover K anyway; representability is then asserted,
    not guaranteed (random signs keep |sum| far below the limit)."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(1000 * seed + {"small_a": 1, "small_b": 2, "wide": 3, "outlier": 4}[family])
    exact = None
    if family in ("small_a", "outlier"):
        per, _ = _budget(dtype, 1, 2, K, M)
        x = _sparse(M, K, per, cuts, g)
        w = _dense(N, K, (-2.0, -1.0, 1.0, 2.0), g)
        if family == "outlier":
            c = int(torch.randint(0, K, (1,), generator=g))
            x[:, c] = OUTLIER * _dense(M, 1, (-1.0, 1.0), g)[:, 0]
            thin = torch.zeros(N, dtype=torch.bool)
            thin[int(torch.randint(0, min(8, N), (1,), generator=g)) :: 8] = True
            w[:, c] = torch.where(thin, w[:, c], torch.zeros(N, dtype=torch.float64))
            # the budget above is spent by the other channels: keep it (one more unit term at most for the rows that see the outlier)
            exact = (~thin)[None, :].expand(M, N).clone()
    elif family == "small_b":
        per, ok = _budget(dtype, 2, 1, K, N)
        if not ok and force_cover:
            per = -(-K // N)
        x = _dense(M, K, (-2.0, -1.0, 1.0, 2.0), g)
        w = _sparse(N, K, per, cuts, g)
    else:  # wide
        x = _dense(M, K, (-2.0, -1.0, 1.0, 2.0), g)
        w = _dense(N, K, (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0), g)
        c = int(torch.randint(0, K, (1,), generator=g))
        big = _dense(N, 1, (-3.0, -2.0, 2.0, 3.0), g)[:, 0]
        x[:, c] = OUTLIER
        w[:, c] = big
    regime = {"small_a": "exact", "small_b": "exact", "outlier": "mixed", "wide": "rounding"}[family]
    case = LinearCase(family, dtype, x.to(dtype), w.to(dtype), exact_mask=exact, cuts=tuple(cuts), regime=regime)
    assert torch.equal(case.x.double(), x) and torch.equal(case.w.double(), w), "operands must be exact in the model dtype"
    if bias:
        case.bias = torch.randint(-3, 4, (N,), generator=g).to(dtype)
    if resid:
        case.resid = torch.randint(-4, 5, (M, N), generator=g).to(dtype)
    return case


def blockscale(case: LinearCase, seed=0) -> LinearCase:
    """The case with every 32-block of every weight row multiplied by its own 2^e: e = E_RANGE[0] + (3 n + 5 b + seed) mod 9 -- neighbouring blocks
    differ by 5 (mod 9), neighbouring rows by 3 (mod 9), never by 0."""
    N, K = case.w.shape
    assert K % 32 == 0
    n = torch.arange(N)[:, None]
    b = torch.arange(K // 32)[None, :]
    span = E_RANGE[1] - E_RANGE[0] + 1
    e = E_RANGE[0] + (3 * n + 5 * b + seed) % span
    w = (case.w.double().view(N, K // 32, 32) * torch.pow(2.0, e.double())[..., None]).view(N, K)
    # a base whose sums need rounding keeps that premise; a scaled small base has no regime of its own (it is neither all exact nor asserted to round)
    out = LinearCase("blockscale/" + case.family, case.dtype, case.x, w.to(case.dtype), cuts=case.cuts, extra={**case.extra, "e": e},
                     regime="rounding" if case.regime == "rounding" else None)
    assert torch.equal(out.w.double(), w)
    return out


def check_blockscale(case: LinearCase):
    """blockscale premises: >= 8 binades, neighbours differ, and mxfp8.py's host quantiser round-trips the matrix unchanged."""
    from dynamic_llava_amd import mxfp8

    e = case.extra["e"]
    assert int(e.max() - e.min()) + 1 >= 8
    assert bool((e[:, 1:] != e[:, :-1]).all()) and bool((e[1:] != e[:-1]).all())
    q, sc = mxfp8.quantize_mx8(case.w, case.dtype)
    assert torch.equal(mxfp8.dequantize_mx8(q, sc, torch.float32).double(), case.w.double()), "not exactly e4m3fn x E8M0"
    return q, sc


def check_premises(case: LinearCase, others=(), cover=True):
    """Asserts (i)-(iv) of the module docstring -- conditions on the reference alone.  `others`: further cases used with the same table entry, whose
    coverage counts together with this one's (small_a + small_b).  Returns the measured facts for the tables of the document."""
    x, w, dt = case.x.double(), case.w.double(), case.dtype
    t = case.truth
    xa, wa = x.abs(), w.abs()
    q = float(xa[xa > 0].min()) * float(wa[wa > 0].min())  # a lower bound of the smallest non-zero product; every operand is a multiple of its own minimum
    assert torch.equal((xa / float(xa[xa > 0].min())).round(), xa / float(xa[xa > 0].min())) and torch.equal((wa / float(wa[wa > 0].min())).round(), wa / float(wa[wa > 0].min()))
    assert float((xa @ wa.T).max()) < 2.0**24 * q, "(i) sum |x||w| must stay below 2^24 units"
    facts = {"unit": q, "max_abs_sum": float((xa @ wa.T).max())}
    rep = representable(t, dt)
    if dt != torch.float32:
        assert case.regime in ("exact", "mixed", "rounding", None)
        if case.regime == "exact":
            assert bool(rep.all()), "(ii) every output of a small case must be exactly representable"
        elif case.regime == "mixed":
            assert bool(rep[case.exact_mask].all()) and bool(case.exact_mask.any()) and not bool(case.exact_mask.all()), "(ii) outlier: the unaffected outputs"
        elif case.regime == "rounding":
            assert float((~rep).float().mean()) >= 0.25, f"(iii) only {float((~rep).float().mean()):.2f} of the outputs need rounding"
            assert bool(is_tie(t, dt).any()), "(iii) no exact tie"
    facts["not_representable"] = float((~rep).float().mean())
    facts["ties"] = int(is_tie(t, dt).sum())
    if cover:
        allc = (case,) + tuple(others)
        k_cov = torch.zeros(x.shape[1], dtype=torch.bool)
        for c in allc:
            k_cov |= (c.x != 0).any(0) & (c.w != 0).any(0)
        assert bool(k_cov.all()), f"(iv) {int((~k_cov).sum())} k never meet a non-zero product"
        for c in allc:
            assert bool((c.x != 0).any(1).all()) and bool((c.w != 0).any(1).all()), "(iv) every row of X and of W takes part"
    return facts


# ------------------------------------------------------------------------------------------------------------------------------
# prologue cases (dl_gemv / dl_gemv_mx8)
# ------------------------------------------------------------------------------------------------------------------------------
def silu_is_identity_on(values, dtype) -> bool:
    """cast(silu(g)) == g for every g in values, by oracle/ref_cpu.py's expression (fp32 silu of the rounded gate, rounded to the dtype)."""
    g = torch.tensor(values, dtype=dtype)
    return torch.equal(torch.nn.functional.silu(g.float()).to(dtype), g)


def make_addnorm_case(family, B, N, K, dtype, seed=0, with_delta=True, cuts=()) -> LinearCase:
    """DL_GEMV_ADDNORM: h_in = +-3 and delta = -+2 (or h_in = +-1 without delta), so hn = +-1, mean(hn^2) = 1 and cast(hn rsqrt(1 + eps)) = hn in 16 bits;
    x = norm_w * hn with norm_w in {0, +-1, +-2} (small: sparse, the zeros) or {+-1, +-2} (wide: dense, the factor 1024 in the weight column)."""
    assert dtype != torch.float32, "rsqrt(1 + eps) does not round to 1 in fp32: left to the tolerance tests"
    g = torch.Generator().manual_seed(7000 + seed)
    sign = _dense(B, K, (-1.0, 1.0), g)
    if family == "small":
        per, _ = _budget(dtype, 2, 2, K, 1)
        nw = _sparse(1, K, per, cuts, g, values=(-2.0, -1.0, 1.0, 2.0))[0]
        w = _dense(N, K, (-2.0, -1.0, 1.0, 2.0), g)
        fam, regime = "addnorm/small", "exact"  # representable outputs; the zero columns of norm_w are the sparse case
    else:
        nw = _dense(1, K, (-2.0, -1.0, 1.0, 2.0), g)[0]
        w = _dense(N, K, (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0), g)
        w[:, int(torch.randint(0, K, (1,), generator=g))] = OUTLIER * _dense(N, 1, (-3.0, -2.0, 2.0, 3.0), g)[:, 0]
        fam, regime = "addnorm/wide", "rounding"
    x = sign * nw[None, :]
    case = LinearCase(fam, dtype, x.to(dtype), w.to(dtype), cuts=tuple(cuts), regime=regime)
    case.extra = {
        "h_in": (3.0 * sign if with_delta else sign).to(dtype),
        "delta": (-2.0 * sign).to(dtype) if with_delta else None,
        "norm_w": nw.to(dtype),
        "h_out": sign.to(dtype),
        "eps": 1e-5,
    }
    assert abs(1.0 / (1.0 + 1e-5) ** 0.5 - 1.0) < 2.0 ** -(SIG_BITS[dtype] + 2), "hn rsqrt(1 + eps) must round back to hn"
    return case


def make_silumul_case(family, B, N, K, dtype, seed=0, cuts=()) -> LinearCase:
    """DL_GEMV_SILUMUL: gate_up [B, 2K] with gates in {0, 16, 32} and up in {+-1, +-2}: x = cast(cast(silu(g)) u) = g u exactly (16-bit dtypes).
    Every x is a multiple of 16, so integer weights would only give multiples of 16 -- all representable up to 16 * 2048.  wide therefore takes its
    weights in sixteenths, {+-1, +-2, +-3} / 16, and puts the large factor into one weight column, 64 * {+-2, +-3}: the products are integers, the
    sums reach several thousand (|x w| <= 64 * 192 = 12288, inside fp16's range) and most of them need rounding."""
    assert dtype != torch.float32 and silu_is_identity_on((0.0, 16.0, 32.0), dtype)
    g = torch.Generator().manual_seed(8000 + seed)
    up = _dense(B, K, (-2.0, -1.0, 1.0, 2.0), g)
    if family == "small":  # |x| <= 64, |w| <= 2, outputs multiples of 16: at most LIMIT * 16 / 128 non-zero gates a row
        per = max(1, min(K, LIMIT[dtype] * 16 // 128))
        gate = _sparse(B, K, per, cuts, g, values=(16.0, 32.0))
        w = _dense(N, K, (-2.0, -1.0, 1.0, 2.0), g)
        fam, regime = "silumul/small", "exact"
    else:
        gate = _dense(B, K, (16.0, 32.0), g)
        w = _dense(N, K, (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0), g) / 16.0
        w[:, int(torch.randint(0, K, (1,), generator=g))] = OUTLIER / 16.0 * _dense(N, 1, (-3.0, -2.0, 2.0, 3.0), g)[:, 0]
        fam, regime = "silumul/wide", "rounding"
    case = LinearCase(fam, dtype, (gate * up).to(dtype), w.to(dtype), cuts=tuple(cuts), regime=regime)
    assert torch.equal(case.w.double(), w)
    case.extra = {"gate_up": torch.cat([gate, up], 1).to(dtype)}
    return case


def make_silu_pair_case(B, I, K, dtype, seed=0, ks=None, hot=4, shared=False, x_hot=1.0):
    """SiLU-pair epilogues (dl_gemv OUT_SILU_PAIR, dl_linear_packed DL_LP_SILU_PAIR, dl_silu_mul_parts): x is x_hot on `hot` columns of a row and 0 elsewhere;
    the rows' hot sets are disjoint (shared=True: one set for all rows -- ADDNORM, whose norm weights all rows share) and are dealt from `ks` first (k = 0,
    K - 1, the k-range bounds), then at random.  On a hot set the gate weights of a neuron are multiples of 16 / x_hot: all but the last in {-16, 0, 16},
    the last chosen so that the gate sum is a target in {0, 16, 32}, where cast(silu(g)) = g; up weights are small integers.  So a gate sum is a
    several-term reduction with cancellation, y = cast(gate * up) is exact, and a term taken from a neighbouring column (arbitrary weights there) shows.
    Returns (x [B, K], w [2I, K] = [gate; up], expected [B, I])."""
    assert dtype != torch.float32 and silu_is_identity_on((0.0, 16.0, 32.0), dtype)
    g = torch.Generator().manual_seed(9000 + seed)
    first = list(dict.fromkeys(k for k in (ks if ks is not None else [0, K - 1]) if 0 <= k < K))
    prio = first + [k for k in torch.randperm(K, generator=g).tolist() if k not in set(first)]
    n_sets = 1 if shared else B
    hot = max(1, min(hot, K // n_sets))
    sets = [prio[s_::n_sets][:hot] for s_ in range(n_sets)]
    x = torch.zeros(B, K, dtype=torch.float64)
    wg = _dense(I, K, (0.0, 16.0, 32.0), g)
    wu = _dense(I, K, (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0), g)
    for s_, cols in enumerate(sets):
        x[(slice(None) if shared else s_), cols] = x_hot
        free = _dense(I, len(cols) - 1, (-16.0, 0.0, 16.0), g)
        target = _dense(I, 1, (0.0, 16.0, 32.0), g)
        wg[:, cols] = torch.cat([free, target - free.sum(1, keepdim=True)], 1)
    w = torch.cat([wg / x_hot, wu], 0)
    t = x @ w.T
    assert bool(((t[:, :I] == 0) | (t[:, :I] == 16) | (t[:, :I] == 32)).all())
    assert bool(representable(t[:, :I] * t[:, I:], dtype).all()) and bool(representable(t[:, I:], dtype).all())
    y = rne(t[:, :I] * t[:, I:], dtype)
    assert torch.equal(w.to(dtype).double(), w)
    return x.to(dtype), w.to(dtype), y


# ------------------------------------------------------------------------------------------------------------------------------
# emulation of the specified arithmetic, and its mutants
# ------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("truncate_output", "partials_rounded_to_dtype", "running_sum_in_dtype", "last_k_dropped_in_strip", "weights_8_early", "scale_of_block_b+1",
           "scale_of_block_b-1", "pad_row_reads_next_row", "row_paired_with_m+1", "row_paired_with_m-1")
ORDERS = ("forward", "reverse", "tree")


def _add_in_order(parts, order):
    """fp32 sum of a list of fp32 tensors in the given order (each + is one fp32 operation)."""
    parts = list(parts)
    if order == "reverse":
        parts = parts[::-1]
    if order == "tree":
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        return parts[0]
    acc = parts[0].clone()
    for p in parts[1:]:
        acc = acc + p
    return acc


def emulate(x, w, out_dtype, n_slices=1, lanes=1, order="forward", mutant=None, scale_e=None, row_tile=16, guard_rows=0):
    """The specified arithmetic on x [M, K], w [N, K]: K cut into n_slices contiguous slices, every slice into `lanes` interleaved lanes of 8-element
    chunks; each (slice, lane) is one fp32 accumulator (an fp32 matmul over its k set); a slice's lanes, then the slices, are added in `order`; ONE
    rounding to out_dtype.  scale_e [N, K/32] (MXFP8): w holds the unit-scale code values, each 32-block's fp32 partial is multiplied by 2^e.
    guard_rows: the output gets that many rows behind M, NaN as in the GPU test's guard band (a correct kernel never writes them).
    mutant: one of MUTANTS."""
    M, K = x.shape
    N = w.shape[0]
    xf, wf = x.float(), w.float()
    if mutant == "weights_8_early":  # the last 8 weights of each row are read 8 elements early
        wf = wf.clone()
        wf[:, K - 8 :] = wf[:, K - 16 : K - 8]
    if scale_e is not None:
        e = scale_e
        if mutant == "scale_of_block_b+1":
            e = torch.cat([e[:, 1:], e[:, -1:]], 1)
        if mutant == "scale_of_block_b-1":
            e = torch.cat([e[:, :1], e[:, :-1]], 1)
        sc = torch.pow(2.0, e.float())  # [N, K/32]
    chunk = torch.arange(K) // 8
    bounds = [(K // 8 * s // n_slices * 8, K // 8 * (s + 1) // n_slices * 8) for s in range(n_slices)]
    slice_sums = []
    for k0, k1 in bounds:
        lane_sums = []
        for ln in range(lanes):
            sel = ((chunk % lanes) == ln) & (torch.arange(K) >= k0) & (torch.arange(K) < k1)
            if scale_e is None:
                acc = xf[:, sel] @ wf[:, sel].T
            else:  # one fp32 partial per 32-block, scaled, added to the accumulator in k order
                acc = torch.zeros(M, N)
                for b in range(k0 // 32, -(-k1 // 32)):
                    sb = sel.clone()
                    sb[: b * 32] = False
                    sb[(b + 1) * 32 :] = False
                    if bool(sb.any()):
                        acc = acc + (xf[:, sb] @ wf[:, sb].T) * sc[None, :, b]
            lane_sums.append(acc)
        s_sum = _add_in_order(lane_sums, order)
        if mutant == "last_k_dropped_in_strip" and k1 == K:  # the last k term is missing in one 1 x 16 output strip
            m_, n0 = int(torch.nonzero(xf[:, K - 1])[-1]) if bool((xf[:, K - 1] != 0).any()) else M - 1, max(0, N - 16)
            last = xf[m_, K - 1] * wf[n0 : n0 + 16, K - 1] * (sc[n0 : n0 + 16, (K - 1) // 32] if scale_e is not None else 1.0)
            s_sum = s_sum.clone()
            s_sum[m_, n0 : n0 + 16] -= last
        if mutant == "partials_rounded_to_dtype":
            s_sum = s_sum.to(out_dtype).float()
        slice_sums.append(s_sum)
    if mutant == "running_sum_in_dtype":
        acc = slice_sums[0].to(out_dtype)
        for p in slice_sums[1:]:
            acc = (acc.float() + p).to(out_dtype)
        total = acc.float()
    else:
        total = _add_in_order(slice_sums, order)
    y = truncate(total.double(), out_dtype) if mutant == "truncate_output" else total.to(out_dtype)
    t0 = (M - 1) // row_tile * row_tile  # first row of the last row tile
    if mutant in ("row_paired_with_m+1", "row_paired_with_m-1") and M - t0 > 1:
        y = y.clone()
        y[t0:M] = torch.roll(y[t0:M], 1 if mutant == "row_paired_with_m+1" else -1, 0)
    if guard_rows:
        pad = torch.full((guard_rows, N), float("nan"), dtype=out_dtype)
        if mutant == "pad_row_reads_next_row":  # rows of the last tile beyond M are computed from a real row and stored
            pad = pad.clone()
            n_pad = min(guard_rows, -M % row_tile)
            pad[:n_pad] = y[M - 1 : M].expand(n_pad, N)
        y = torch.cat([y, pad], 0)
    return y


def same_values(a, b) -> bool:
    """torch.equal as values (+-0 equal, NaN equal only to NaN in the same place: the guard band)."""
    if a.shape != b.shape:
        return False
    an, bn = torch.isnan(a.float()), torch.isnan(b.float())
    return bool((an == bn).all()) and bool((a.float()[~an] == b.float()[~bn]).all())


def count_diff(a, b) -> int:
    an, bn = torch.isnan(a.float()), torch.isnan(b.float())
    return int(((a.float() != b.float()) & ~(an & bn)).sum())


# the tolerances of the older GPU tests, restated (tests/test_kernels_gpu.py): what a mutant has to get past there
ULP = {torch.float32: 2.0**-23, torch.float16: 2.0**-10, torch.bfloat16: 2.0**-7}


def old_linear_packed_ratio(y, ref64, dtype, K) -> float:
    """max |err| over the bound of test_linear_packed_vs_fp32_every_layout: (0.5 ulp + 3e-5 sqrt(K / 1024 + 1)) max(1, max |ref|) 1.01.  < 1 passes."""
    import math

    tol = (0.5 * ULP[dtype] + 3e-5 * math.sqrt(K / 1024 + 1)) * max(1.0, float(ref64.abs().max())) * 1.01
    return float((y.double() - ref64).abs().max()) / tol


def old_close_ulp_bad(y, ref, dtype, n_ulp=1.0, atol=1e-3) -> int:
    """Elements outside _close_ulp(n_ulp, atol): |a - b| <= n_ulp ulp max(|a|, |b|) + atol.  0 passes."""
    a, b = y.float(), ref.float()
    tol = n_ulp * ULP[dtype] * torch.maximum(a.abs(), b.abs()) + atol
    return int(((a - b).abs() > tol).sum())
