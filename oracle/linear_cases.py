"""The table behind tests/test_linear_exact_gpu.py: one entry per kernel instantiation the linear family can launch, and the code that drives it.

Every entry names the template instantiation(s) it reaches -- by a restatement, in the *_inst functions below, of the dispatch code of csrc/linear.hip
(linear_launch, dl_linear_splitk), csrc/gemv.hip (gemv_variant / gemv_launch), csrc/gemm_smallm.hip (dl_gemm_smallm), csrc/linear_packed.hip (lp_nu /
lp_tpw / lp_epi), csrc/linear_tiles.hip (lt_shape), csrc/gemv_mx8.hip (gemv_mx8_launch) and csrc/gemm_mx8.hip (dl_gemm_mx8).  ALL_INSTANTIATIONS lists
what those functions can reach in a release build; OMITTED gives the one-line reason for each one the table leaves out; the closing test asserts
table + omitted == all.

A launch is checked by Runner.check: the output (and every fp32 partial-sum buffer) lies inside a NaN guard band, X / Y rows are strided where the ABI
takes a stride, the result must equal `expected` as values (+-0 equal, NaN never), the band must still be NaN, and a second identical launch must
return the same bits.  Inputs and expectations: oracle/linear_truth.py (one expected tensor per (family, shape, dtype), shared by every kernel, split
and layout that computes it)."""
from __future__ import annotations

from functools import lru_cache

import torch

from oracle import linear_truth as lt

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DT = {BF16: "bf16", F16: "f16", F32: "f32"}
HALF = (BF16, F16)
FAMS = lt.FAMILIES


# ------------------------------------------------------------------------------------------------------------------------------
# cases (cached: built and checked once per process)
# ------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def case(family, M, N, K, dtype, cuts=(), bias=False, resid=False):
    """A case whose premises hold (the seed is advanced until the reference alone satisfies them -- wide needs a tie among as few as N outputs)."""
    last = None
    for seed in range(16):
        try:
            c = lt.make_case(family, M, N, K, dtype, seed=seed, cuts=cuts, bias=bias, resid=resid, force_cover=True)
            partner = ()
            if family in ("small_a", "outlier"):
                partner = (lt.make_case("small_b", M, N, K, dtype, seed=seed, cuts=cuts, force_cover=True),)
            elif family == "small_b":
                partner = (lt.make_case("small_a", M, N, K, dtype, seed=seed, cuts=cuts),)
            lt.check_premises(c, others=partner)
            return c
        except AssertionError as e:  # premise not met at this seed
            last = e
    raise AssertionError(f"no seed satisfies the premises of {family} at {M}x{N}x{K} {dtype}: {last}")


def _first_seed(make, cover):
    last = None
    for seed in range(16):
        try:
            c = make(seed)
            lt.check_premises(c, cover=cover)
            return c
        except AssertionError as e:  # premise not met at this seed (a tie among as few as 40 outputs)
            last = e
    raise AssertionError(f"no seed satisfies the premises: {last}")


@lru_cache(maxsize=None)
def mx_case(base, M, N, K, dtype, cuts=()):
    """blockscale on a base case; the seed is advanced until the scaled case satisfies its own premises too (wide: a tie among the scaled sums)."""
    def make(seed):
        c = lt.blockscale(lt.make_case(base, M, N, K, dtype, seed=seed, cuts=cuts, force_cover=True))
        c.extra["q"], c.extra["scale"] = lt.check_blockscale(c)
        return c

    return _first_seed(make, base in ("wide", "small_b"))


@lru_cache(maxsize=None)
def addnorm_case(family, B, N, K, dtype, with_delta=True):
    return _first_seed(lambda seed: lt.make_addnorm_case(family, B, N, K, dtype, seed=16 * B + seed, with_delta=with_delta), family == "wide")


@lru_cache(maxsize=None)
def mx_addnorm_case(family, B, N, K, dtype, with_delta=True):
    """blockscale on an ADDNORM case (the activations and the prologue operands are untouched)."""
    def make(seed):
        b = lt.blockscale(lt.make_addnorm_case(family, B, N, K, dtype, seed=16 * B + seed, with_delta=with_delta))
        lt.check_blockscale(b)
        return b

    return _first_seed(make, family == "wide")


@lru_cache(maxsize=None)
def silumul_case(family, B, N, K, dtype):
    return _first_seed(lambda seed: lt.make_silumul_case(family, B, N, K, dtype, seed=16 * B + seed), family == "wide")


def split_bounds(K, step, n, trim256=0):
    """k ranges of a kernel that deals ceil(K / step) steps to n ranges: range r = steps [S r / n, S (r + 1) / n) (dl_linear_splitk, dl_gemm_smallm,
    dl_gemm_mx8, dl_linear_tiles); dl_linear_packed's in-launch hand-over shortens all but the last by trim256 / 256."""
    S = -(-K // step)
    b = [S if r >= n else S * r * (256 - trim256) // (256 * n) for r in range(n + 1)]
    return [(min(b[r] * step, K), min(b[r + 1] * step, K)) for r in range(n)]


def cuts_of(bounds):
    return tuple(sorted({k for k0, k1 in bounds for k in (k0, k1) if 0 < k}))[:-1] if bounds else ()


# ------------------------------------------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------------------------------------------
class Runner:
    def __init__(self, ops, device="cuda"):
        self.ops, self.dev, self.bad, self.n, self.bands = ops, device, [], 0, []

    def d(self, t):
        return None if t is None else t.to(self.dev)

    def strided(self, t, pad=8):
        """t [R, C] on the device as a view of a wider NaN-filled buffer (row stride C + pad)."""
        buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=self.dev)
        buf[:, : t.shape[1]] = t.to(self.dev)
        return buf[:, : t.shape[1]]

    def out2d(self, M, N, dtype):
        ld = -(-N // 8) * 8 + 8
        buf = torch.full((M + 2, ld), float("nan"), dtype=dtype, device=self.dev)
        return buf, buf[1 : M + 1, :N]

    def flat(self, shape, dtype=F32):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 128,), float("nan"), dtype=dtype, device=self.dev)
        return buf, buf[64 : 64 + n].view(*shape)

    def check(self, tag, fn, exp, contiguous=False):
        """fn(view) launches into `view` (a [M, N] strided view, or a contiguous tensor of exp's shape); see the module docstring."""
        exp_d = exp.to(self.dev)
        res = []
        for _ in range(2):
            buf, view = self.flat(tuple(exp.shape), exp.dtype) if contiguous else self.out2d(exp.shape[0], exp.shape[1], exp.dtype)
            fn(view)
            res.append((buf, view))
        self.n += 1
        (b0, v0), (b1, v1) = res
        eq = v0 == exp_d
        g = b0.clone()
        if contiguous:
            g[64 : 64 + exp.numel()] = float("nan")
        else:
            g[1 : exp.shape[0] + 1, : exp.shape[1]] = float("nan")
        ok = torch.stack([eq.all(), torch.isnan(g).all(), (v0 == v1).all() | ~eq.all()])
        ok = ok.tolist()
        if not all(ok):
            idx = torch.nonzero(~eq)
            self.bad.append(dict(tag=tag, differing=int((~eq).sum()), of=exp.numel(), first=idx[:6].tolist(), got=v0[~eq][:6].float().tolist(),
                                 want=exp_d[~eq][:6].float().tolist(), guard_intact=ok[1], second_launch_same=ok[2]))
        return v0

    def workspace(self, n, tag):
        """fp32 workspace of n elements inside a NaN band (16-byte aligned interior); finish() asserts the band is still NaN."""
        buf = torch.full((n + 128,), float("nan"), dtype=F32, device=self.dev)
        self.bands.append((tag, buf, 64, 64 + n, None))
        return buf[64 : 64 + n]

    def workspace_bytes(self, n, tag):
        """Zeroed byte workspace (dl_linear_packed's hand-over buffer: 256-byte aligned, zeroed once) inside a band of 0xA5 bytes."""
        buf = torch.full((n + 768,), 0xA5, dtype=torch.uint8, device=self.dev)
        lo = 256 + (-buf.data_ptr()) % 256
        buf[lo : lo + n] = 0
        self.bands.append((tag, buf, lo, lo + n, 0xA5))
        return buf[lo : lo + n]

    def finish(self):
        """Every workspace band handed out is untouched."""
        for tag, buf, lo, hi, fill in self.bands:
            self.n += 1
            band = torch.cat([buf[:lo], buf[hi:]])
            ok = bool(torch.isnan(band).all()) if fill is None else bool((band == fill).all())
            if not ok:
                self.bad.append(dict(tag=f"{tag}: workspace guard band written", guard_intact=False, differing=0, second_launch_same=True))
        self.bands = []

    def same(self, tag, a, b):
        self.n += 1
        if not bool((a == b.to(a.device)).all()):
            self.bad.append(dict(tag=tag, differing=int((a != b.to(a.device)).sum()), of=a.numel()))


# ------------------------------------------------------------------------------------------------------------------------------
# dl_linear
# ------------------------------------------------------------------------------------------------------------------------------
def linear_inst(dtype, K):
    return "linear_simple_kernel<f32>" if dtype == F32 else f"linear_mfma_kernel<{DT[dtype]},{128 if K >= 1024 else 64}>"


# (M, N, K): ragged in M and N (64 x 64 tiles, more than one block either way), K no multiple of the k tile (128 / 64); K >= 1024 and K < 1024
LINEAR_SHAPES = [(70, 136, 1032), (70, 136, 520), (64, 64, 1024)]
LINEAR_TABLE = [dict(id=f"linear-{M}x{N}x{K}-{DT[dt]}", shape=(M, N, K), dtype=dt, inst={linear_inst(dt, K)}) for (M, N, K) in LINEAR_SHAPES for dt in (BF16, F16, F32)]


def run_linear(R, e):
    M, N, K = e["shape"]
    dt = e["dtype"]
    for fam in FAMS:
        for flags, bias in ((0, False), (0, True), (2, False), (2, True)):
            c = case(fam, M, N, K, dt, (), bias, flags == 2)
            x, w = R.strided(c.x), R.d(c.w)
            b = R.d(c.bias)
            r = R.strided(c.resid, 16) if c.resid is not None else None
            R.check(f"{e['id']} {fam} flags {flags} bias {bias}", lambda y: R.ops.linear(x, w, bias=b, flags=flags, residual=r, out=y), c.expected())


# ------------------------------------------------------------------------------------------------------------------------------
# dl_linear_splitk
# ------------------------------------------------------------------------------------------------------------------------------
def splitk_inst(dtype, M):
    return f"linear_splitk_wide_kernel<{DT[dtype]},64,{4 if M <= 128 else 6}>" if M <= 192 else f"linear_splitk_kernel<{DT[dtype]},128>"


SPLITK_TABLE = [dict(id=f"splitk-M{M}-{DT[dt]}", shape=(M, 132, 1032), dtype=dt, inst={splitk_inst(dt, M)}) for M in (100, 170, 200) for dt in HALF]


def run_splitk(R, e):
    M, N, K = e["shape"]
    dt = e["dtype"]
    step = 64 if M <= 192 else 128
    for ns in (1, 3, 8):
        bounds = split_bounds(K, step, ns)
        for fam in FAMS:
            c = case(fam, M, N, K, dt, cuts_of(split_bounds(K, step, 8)))
            x, w = R.strided(c.x), R.d(c.w)
            exp = c.expected_parts(bounds)
            assert torch.equal(exp.double().sum(0), c.truth)  # the sum of the parts is exact
            R.check(f"{e['id']} {fam} n_slices {ns}", lambda p: R.ops.linear_splitk(x, w, p.view(-1), ns), exp, contiguous=True)


# ------------------------------------------------------------------------------------------------------------------------------
# dl_gemv
# ------------------------------------------------------------------------------------------------------------------------------
PLAIN, ADDNORM, SILUMUL, PAIR = 0, 1, 2, 16
MODE_NAME = {0: "PLAIN", 1: "ADDNORM", 2: "SILUMUL"}


def gemv_inst(dtype, B, mode, K):
    pro, pair = mode & 3, bool(mode & PAIR)
    T = DT[dtype]
    if pair:
        return f"gemv_kernel<{T},{B},{pro},pair,2,4>"
    if B == 1 and pro == 0 and dtype != F32:
        if K // 8 <= 512:
            return f"gemv_b1_plain_kernel<{T},1>"
        if K // 8 <= 1024:
            return f"gemv_b1_plain_kernel<{T},2>"
        if K // 8 <= 2048:
            return f"gemv_b1_plain_halves_kernel<{T},{12 if ((K // 8 + 1) // 2 + 63) // 64 <= 12 else 16}>"
    if B == 1 and pro == 0:
        return f"gemv_kernel<{T},1,0,plain,1,8>"
    return f"gemv_kernel<{T},{B},{pro},plain,2,4>"


def _gemv_entries():
    out = []
    for dt in (BF16, F16, F32):
        for B in range(1, 9):
            for mode in (PLAIN, ADDNORM, SILUMUL, PLAIN | PAIR, ADDNORM | PAIR, SILUMUL | PAIR):
                if dt == F32 and mode != PLAIN:
                    continue
                Ks = [512]
                if B == 1 and mode == PLAIN and dt != F32:
                    Ks = [512, 4104, 8200, 12296, 16392]  # x in registers (8 / 16 chunks a lane), wave-pair halves (12 / 16 chunks, ragged), the generic kernel
                for K in Ks:
                    N = 40 if K == 512 else 64
                    out.append(dict(id=f"gemv-{DT[dt]}-B{B}-{MODE_NAME[mode & 3]}{'-pair' if mode & PAIR else ''}-K{K}", B=B, mode=mode, shape=(B, N, K), dtype=dt,
                                    inst={gemv_inst(dt, B, mode, K)}))
    return out


GEMV_TABLE = _gemv_entries()
GRID_CAPS = (0, 3)  # the tuned default; three workgroups, so that every workgroup loops over several neuron groups


def _pair_operands(R, B, I, K, dt, mode):
    """Activations for the SiLU-pair epilogue in each prologue (lt.make_silu_pair_case: four hot columns a row, gate sums on {0, 16, 32})."""
    pro = mode & 3
    kw = {}
    if pro == PLAIN:
        x, w, y = lt.make_silu_pair_case(B, I, K, dt, seed=B)
        kw["x"] = R.strided(x)
    elif pro == ADDNORM:  # norm_w is shared by the rows: one hot set, h + delta = +1 there, norm_w = 1 there and 0 elsewhere
        x, w, y = lt.make_silu_pair_case(B, I, K, dt, seed=B, ks=[K - 1, 0, 255, 256], shared=True)
        g = torch.Generator().manual_seed(B)
        sign = torch.where(torch.rand(B, K, generator=g) < 0.5, -1.0, 1.0)
        sign[x != 0] = 1.0
        kw.update(h_in=R.d((3 * sign).to(dt)), delta=R.d((-2 * sign).to(dt)), norm_w=R.d(x[0].clone()), eps=1e-5, h_out=torch.full((B, K), float("nan"), dtype=dt, device=R.dev))
        kw["_h_out"] = sign.to(dt)
    else:  # SILUMUL: gate 16 (silu(16) = 16) and up 1 in the hot columns, gate 0 elsewhere; the gate weights are sixteenths of PLAIN's
        x, w, y = lt.make_silu_pair_case(B, I, K, dt, seed=B, x_hot=16.0)
        kw["x"] = R.strided(torch.cat([x, torch.ones_like(x)], 1))
    return kw, R.d(w), y


def run_gemv(R, e, mx8=False):
    B, N, K = e["shape"]
    dt, mode = e["dtype"], e["mode"]
    pro = mode & 3
    ops = R.ops

    def launch(wd, kw, cap):
        hidden = {k: v for k, v in kw.items() if not k.startswith("_")}
        if mx8:
            return lambda y: ops.gemv_mx8(wd[0], wd[1], y, mode=mode, grid_cap=cap, **hidden)
        return lambda y: ops.gemv(wd, y, mode=mode, grid_cap=cap, **hidden)

    def weights(c_w):
        if not mx8:
            return R.d(c_w)
        q, sc = ops.quantize_mx8(R.d(c_w), model_dtype=dt)
        from dynamic_llava_amd import mxfp8

        qh, sh = mxfp8.quantize_mx8(c_w, dt)
        assert torch.equal(mxfp8.dequantize_mx8(qh, sh, torch.float32).double(), c_w.double()), "the weights must be exactly e4m3fn x E8M0"
        R.same(f"{e['id']} dl_quantize_mx8 codes", q, qh)
        R.same(f"{e['id']} dl_quantize_mx8 scales", sc, sh)
        return q, sc

    if mode & PAIR:
        kw, w, y = _pair_operands(R, B, N // 2, K, dt, mode)
        wd = weights(w.cpu()) if mx8 else w
        for cap in GRID_CAPS:
            R.check(f"{e['id']} hot-columns cap {cap}", launch(wd, kw, cap), y)
            if "_h_out" in kw:
                R.same(f"{e['id']} h_out", kw["h_out"], kw["_h_out"])
        return
    if pro == PLAIN:
        fams = FAMS if not mx8 else ("small_a", "small_b", "wide")
        cs = [(f, mx_case(f, B, N, K, dt) if mx8 else case(f, B, N, K, dt)) for f in fams]
    elif pro == ADDNORM:
        cs = [(f"addnorm-{f}{'' if wd_ else '-nodelta'}", (mx_addnorm_case if mx8 else addnorm_case)(f, B, N, K, dt, wd_)) for f in ("small", "wide") for wd_ in ((True, False) if f == "wide" else (True,))]
    else:
        cs = [(f"silumul-{f}", silumul_case(f, B, N, K, dt)) for f in ("small", "wide")]
    for name, c in cs:
        wd = weights(c.w)
        if pro == PLAIN:
            kw = dict(x=R.strided(c.x))
        elif pro == ADDNORM:
            ex = c.extra
            kw = dict(h_in=R.d(ex["h_in"]), delta=R.d(ex["delta"]), norm_w=R.d(ex["norm_w"]), eps=ex["eps"],
                      h_out=torch.full((B, K), float("nan"), dtype=dt, device=R.dev) if ex["delta"] is not None else None)
        else:
            kw = dict(x=R.strided(c.extra["gate_up"]))
        for cap in GRID_CAPS:
            R.check(f"{e['id']} {name} cap {cap}", launch(wd, kw, cap), c.expected())
            if pro == ADDNORM and c.extra["delta"] is not None:
                R.same(f"{e['id']} {name} h_out", kw["h_out"], c.extra["h_out"])


# ------------------------------------------------------------------------------------------------------------------------------
# dl_gemv_mx8
# ------------------------------------------------------------------------------------------------------------------------------
def gemv_mx8_inst(dtype, B, mode):
    return f"gemv_mx8_kernel<{DT[dtype]},{B},{mode & 3},{'pair' if mode & PAIR else 'plain'},2,4>"


GEMV_MX8_TABLE = [
    dict(id=f"gemv_mx8-{DT[dt]}-B{B}-{MODE_NAME[mode & 3]}{'-pair' if mode & PAIR else ''}-K{K}", B=B, mode=mode, shape=(B, 40, K), dtype=dt, inst={gemv_mx8_inst(dt, B, mode)})
    for dt in (BF16, F16, F32)
    for B in range(1, 9)
    for mode in (PLAIN, ADDNORM, ADDNORM | PAIR)
    for K in ((512, 2048) if (B <= 3 and mode == PLAIN) else (512,))
    if dt != F32 or mode == PLAIN
]


# ------------------------------------------------------------------------------------------------------------------------------
# dl_gemm_smallm (+ dl_add_rmsnorm_parts / dl_silu_mul_parts on its partial sums)
# ------------------------------------------------------------------------------------------------------------------------------
def smallm_inst(dtype, M, variant, wg_waves):
    nb = 1 if M <= 16 else 2
    if variant == 1:
        return f"gemm_smallm_kernel<{DT[dtype]},{nb},{4 if wg_waves == 4 else 8}>"
    return f"gemm_smallm_staged_kernel<{DT[dtype]},{nb},{256 if variant == 2 else 128},{8 if variant == 2 else 16}>"


SMALLM_TABLE = [
    dict(id=f"smallm-{DT[dt]}-M{M}-v{v}w{ww}", shape=(M, 136, 1024), dtype=dt, variant=v, wg_waves=ww, inst={smallm_inst(dt, M, v, ww)})
    for dt in HALF
    for (v, ww) in ((1, 4), (1, 8), (2, 0), (3, 0))
    for M in (5, 16, 17, 32)
] + [  # 32 rows of K = 11008 do not fit LDS in one slice: the slicing the kernel forces
    dict(id=f"smallm-{DT[dt]}-M32-K11008-v{v}", shape=(32, 64, 11008), dtype=dt, variant=v, wg_waves=0, inst={smallm_inst(dt, 32, v, 0)}, lds_forced=True)
    for dt in HALF
    for v in (1, 2)
]


def run_smallm(R, e):
    M, N, K = e["shape"]
    dt, v, ww = e["dtype"], e["variant"], e["wg_waves"]
    ops, lib = R.ops, R.ops.lib()
    forced = e.get("lds_forced", False)
    wants = (1,) if forced else (0, 1, 3)
    eff = {ns: int(lib.dl_gemm_smallm_slices(M, N, K, ns, v)) for ns in wants}
    if forced:
        assert eff[1] > 1, "the shape must force the slicing"
    cuts = tuple(sorted({k for s in eff.values() for k in cuts_of(split_bounds(K, 256, s))}))
    for fam in FAMS:
        c = case(fam, M, N, K, dt, cuts)
        x, w = R.strided(c.x), R.d(c.w)
        for ns in wants:
            ws = R.workspace(max(eff[ns] * M * N, 4), f"{e['id']} {fam} n_slices {ns}")
            R.check(f"{e['id']} {fam} n_slices {ns} (effective {eff[ns]})", lambda y: ops.gemm_smallm(x, w, out=y, workspace=ws, n_slices=ns, wg_waves=ww, variant=v), c.expected())
        if ww != 4:  # the partial-sum form (defer_reduce takes no wg_waves) and its consumer: h integer, h + RNE(sum of the parts)
            ns = wants[-1]
            exp = c.expected_parts(split_bounds(K, 256, eff[ns]))
            parts = R.check(f"{e['id']} {fam} parts n_slices {ns}", lambda p: ops.gemm_smallm_parts(x, w, p.view(-1), n_slices=ns, variant=v), exp, contiguous=True)
            if N % 8 == 0:
                g = torch.Generator().manual_seed(M)
                h0 = torch.randint(-4, 5, (M, N), generator=g).to(dt)
                want = lt.rne(h0.double() + c.expected().double(), dt)

                def add(hbuf):
                    hbuf.copy_(h0.to(R.dev))
                    ops.add_rmsnorm_parts(hbuf, parts, None)

                R.check(f"{e['id']} {fam} add_rmsnorm_parts", add, want, contiguous=True)
    if ww != 4 and not forced:  # gate|up partial sums through dl_silu_mul_parts: four hot columns a row, gate sums on {0, 16, 32}
        I = 64
        x1, w1, y1 = lt.make_silu_pair_case(M, I, K, dt, seed=M, ks=[0, K - 1, 255, 256, 511, 512, 767, 768])
        ws = R.workspace(int(lib.dl_gemm_smallm_slices(M, 2 * I, K, 3, v)) * M * 2 * I, f"{e['id']} silu_mul_parts")
        parts, _ = ops.gemm_smallm_parts(R.strided(x1), R.d(w1), ws, n_slices=3, variant=v)
        parts = parts.contiguous()
        R.check(f"{e['id']} silu_mul_parts", lambda y: ops.silu_mul_parts(parts, y), y1, contiguous=True)


# ------------------------------------------------------------------------------------------------------------------------------
# dl_gemm_mx8
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_MX8_TABLE = [dict(id=f"gemm_mx8-{DT[dt]}-M{M}", shape=(M, 132, 2048), dtype=dt, inst={f"gemm_mx8_kernel<{DT[dt]},{1 if M <= 16 else 2}>"}) for dt in HALF for M in (4, 16, 17, 32)]


def run_gemm_mx8(R, e):
    M, N, K = e["shape"]
    dt = e["dtype"]
    ops, lib = R.ops, R.ops.lib()
    from dynamic_llava_amd import mxfp8

    wants = (0, 1, 64)  # automatic, one slice, the most dl_gemm_mx8_slices allows (K / 256)
    eff = {ns: int(lib.dl_gemm_mx8_slices(M, N, K, ns)) for ns in wants}
    assert eff[64] == K // 256 and eff[1] == (1 if M <= 16 else 2)  # (two row tiles of K = 2048 do not fit LDS beside the staging: the forced slicing)
    cuts = tuple(range(256, K, 256))
    for base in ("small_a", "small_b", "wide"):
        c = mx_case(base, M, N, K, dt, cuts)
        x = R.strided(c.x)
        q, sc = ops.quantize_mx8(R.d(c.w), model_dtype=dt)
        R.same(f"{e['id']} {base} dl_quantize_mx8 codes", q, c.extra["q"])
        R.same(f"{e['id']} {base} dl_quantize_mx8 scales", sc, c.extra["scale"])
        for ns in wants:
            ws = R.workspace(eff[ns] * M * N + 4, f"{e['id']} {base} n_slices {ns}")
            R.check(f"{e['id']} blockscale/{base} n_slices {ns} (effective {eff[ns]})", lambda y: ops.gemm_mx8(x, q, sc, out=y, workspace=ws, n_slices=ns), c.expected())
            exp = c.expected_parts(mxfp8.gemm_mx8_slice_bounds(K, eff[ns]))
            R.check(f"{e['id']} blockscale/{base} parts n_slices {ns}", lambda p: ops.gemm_mx8_parts(x, q, sc, p.view(-1), n_slices=ns), exp, contiguous=True)


# ------------------------------------------------------------------------------------------------------------------------------
# dl_linear_packed
# ------------------------------------------------------------------------------------------------------------------------------
LP_STORE, LP_SILU_PAIR, LP_RESID, LP_PARTS = 0, 1, 2, 3
LP_EPI_NAME = {0: "STORE", 1: "SILU_PAIR", 2: "RESID", 3: "PARTS"}
LP_UNITS = (1, 2, 3, 4, 6, 8)


def lp_inst(dtype, nu, M, epi):
    return f"linear_packed_kernel<{DT[dtype]},NU{nu},TPW{-(-(-(-M // 16)) // 4)},{LP_EPI_NAME[epi]}>"


# rows -> tiles per consumer wave 1 (M <= 64), 2, 3, 4; 1 / 16 / 17: a single row, a full tile, one row into the second tile
LP_ROWS = (1, 16, 17, 100, 170, 256)
# (k_split, K): K = 1024 is 16 steps of 64 k; eight ranges need K = 2048 so that the shortened hand-over ranges (split_bounds) all hold a step
LP_SPLITS = {1: (1, 1024), 2: (2, 1024), 3: (3, 1024), 4: (1, 1024), 6: (8, 2048), 8: (2, 1024)}  # by units per workgroup: every unit count also runs k_split 1
LP_TABLE = [
    dict(id=f"linear_packed-{DT[dt]}-NU{nu}-M{M}-{LP_EPI_NAME[epi]}", dtype=dt, nu=nu, M=M, epi=epi, inst={lp_inst(dt, nu, M, epi)})
    for dt in HALF
    for nu in LP_UNITS
    for M in LP_ROWS
    for epi in (LP_STORE, LP_SILU_PAIR, LP_RESID, LP_PARTS)
    if not (epi == LP_SILU_PAIR and nu % 2)
]


def run_linear_packed(R, e):
    dt, nu, M, epi = e["dtype"], e["nu"], e["M"], e["epi"]
    ops = R.ops
    N = 224 if epi == LP_SILU_PAIR else 208  # 14 / 13 units of 16 neurons: a ragged last workgroup for 3, 4, 6, 8 (and 2: 13) units per workgroup
    for ks, K in {(1, 1024), LP_SPLITS[nu]}:
        trim = 24 if (ks > 1 and epi != LP_PARTS) else 0
        bounds = split_bounds(K, 64, ks, trim)
        assert all(k1 > k0 for k0, k1 in bounds)
        need = int(ops.lib().dl_linear_packed_workspace_bytes(M, N, K, epi, nu, ks)) if epi != LP_PARTS else 0
        assert need >= 0
        ws = R.workspace_bytes(need, f"{e['id']} k_split {ks}") if need else None
        err = torch.zeros(1, dtype=torch.int32, device=R.dev)
        if epi == LP_SILU_PAIR:
            hot = [0, K - 1] + [k for k0, k1 in bounds for k in (k0, k1 - 1)] + [31, 32, 63, 64]
            x1, w1, y1 = lt.make_silu_pair_case(M, N // 2, K, dt, seed=M, ks=hot)
            todo = [("hot-columns", x1, ops.pack_weight_tiles(R.d(w1), gate_up_pairs=True), y1, None)]
        else:
            todo = []
            for fam in FAMS:
                c = case(fam, M, N, K, dt, cuts_of(bounds), False, epi == LP_RESID)
                todo.append((fam, c.x, ops.pack_weight_tiles(R.d(c.w)), c.expected_parts(bounds) if epi == LP_PARTS else c.expected(), c.resid))
        for fam, x, wp, exp, resid in todo:
            xs, xp = R.strided(x), ops.pack_x_tiles(R.d(x))
            r = R.strided(resid, 16) if resid is not None else None
            for layout, xin, mk in (("row-major", xs, None), ("fragment-order", xp, (M, K))):
                tag = f"{e['id']} {fam} k_split {ks} K {K} X {layout}"
                if epi == LP_PARTS:
                    R.check(tag, lambda p: ops.linear_packed(xin, wp, N, out=p, epilogue=epi, units_per_workgroup=nu, k_split=ks, x_packed_mk=mk), exp, contiguous=True)
                else:
                    R.check(tag, lambda y: ops.linear_packed(xin, wp, N, out=y, epilogue=epi, resid=r, units_per_workgroup=nu, k_split=ks, workspace=ws, err=err, x_packed_mk=mk), exp)
        R.same(f"{e['id']} err_flag", err, torch.zeros(1, dtype=torch.int32))
        if ws is not None:
            R.same(f"{e['id']} flag words zero after the launches", ws[:256], torch.zeros(256, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------------------------
# dl_linear_tiles
# ------------------------------------------------------------------------------------------------------------------------------
LT_BIAS, LT_PARTS = 0, 3
LT_SHAPES = [542, 20542, 532, 20532, 522, 512, 521, 20521, 541, 20541, 1042, 1032, 1041]  # lt_shape's LT_CASE list (release build)
LT_PARTS_ONLY = [142, 20142, 242, 20242, 342, 442, 642, 742, 842, 20842]                 # its LT_CASE_PARTS list


def lt_inst(dtype, shape, epi):
    dw = 5 if shape >= 20000 else 3
    s = shape % 10000
    return f"linear_tiles_kernel<{DT[dtype]},TM{s // 100},WN{(s // 10) % 10},NUW{s % 10},{'BIAS' if epi == LT_BIAS else 'PARTS'},DW{dw}>"


LT_TABLE = [dict(id=f"linear_tiles-{DT[dt]}-{s}-{'BIAS' if epi == LT_BIAS else 'PARTS'}", dtype=dt, tile_shape=s, epi=epi, inst={lt_inst(dt, s, epi)})
            for dt in HALF for s in LT_SHAPES + LT_PARTS_ONLY for epi in (LT_BIAS, LT_PARTS) if epi == LT_PARTS or s in LT_SHAPES]


def unpack_rows(yp, M, N):
    """dl_linear_tiles' fragment order [step = n / 64][tile = row / 16][half][lane = 16 ((n % 32) / 8) + row % 16][8] -> [M, N]."""
    tiles = -(-M // 16)
    return yp[: N // 64 * tiles * 1024].view(N // 64, tiles, 2, 4, 16, 8).permute(1, 4, 0, 2, 3, 5).reshape(tiles * 16, N)[:M]


def run_linear_tiles(R, e):
    dt, shape, epi = e["dtype"], e["tile_shape"], e["epi"]
    ops = R.ops
    tm = shape % 10000 // 100
    M = 330 if tm == 10 else 170  # 160-row tiles: three row blocks, the last ragged; else 11 row tiles: ragged for every TM but 1
    N, K = 208, 512               # 13 units: a ragged last column block for every WN x NUW
    for ks in ((1,) if epi == LT_BIAS else (1, 3)):
        bounds = split_bounds(K, 64, ks)
        for fam in FAMS:
            for bias in ((False, True) if epi == LT_BIAS else (False,)):
                c = case(fam, M, N, K, dt, cuts_of(split_bounds(K, 64, 3)), bias, False)
                wp = ops.pack_weight_tiles(R.d(c.w))
                b = R.d(c.bias)
                xs, xp = R.strided(c.x), ops.pack_x_rows(R.d(c.x))
                for layout, xin, mk in (("row-major", xs, None), ("fragment-order", xp, (M, K))):
                    tag = f"{e['id']} {fam} k_split {ks} bias {bias} X {layout}"
                    if epi == LT_PARTS:
                        R.check(tag, lambda p: ops.linear_tiles(xin, wp, N, out=p, epilogue=epi, x_packed_mk=mk, tile_shape=shape, k_split=ks), c.expected_parts(bounds), contiguous=True)
                    else:
                        R.check(tag, lambda y: ops.linear_tiles(xin, wp, N, bias=b, out=y, epilogue=epi, x_packed_mk=mk, tile_shape=shape), c.expected())
    if epi == LT_BIAS:  # fragment-order Y (N % 64 == 0): the rows of the last tile past M may hold anything, so only [:M] is compared
        Np = 192
        c = case("wide", M, Np, K, dt, (), True, False)
        yp = ops.linear_tiles(R.strided(c.x), ops.pack_weight_tiles(R.d(c.w)), Np, bias=R.d(c.bias), epilogue=epi, y_packed=True, tile_shape=shape)
        R.same(f"{e['id']} wide fragment-order Y", unpack_rows(yp, M, Np), c.expected())


# ------------------------------------------------------------------------------------------------------------------------------
# the instantiations the dispatch code can reach (release build), and the ones this table leaves out
# ------------------------------------------------------------------------------------------------------------------------------
def all_instantiations():
    out = set()
    for dt in (BF16, F16, F32):
        T = DT[dt]
        # csrc/linear.hip linear_launch / dl_linear_splitk
        out |= {"linear_simple_kernel<f32>"} if dt == F32 else {f"linear_mfma_kernel<{T},128>", f"linear_mfma_kernel<{T},64>", f"linear_splitk_wide_kernel<{T},64,4>",
                                                                  f"linear_splitk_wide_kernel<{T},64,6>", f"linear_splitk_kernel<{T},128>"}
        # csrc/gemv.hip dl_gemv -> gemv_launch<T, B> -> gemv_variant<T, B, MODE>
        for B in range(1, 9):
            for pro in (0, 1, 2):
                out.add(f"gemv_kernel<{T},{B},{pro},pair,2,4>")
                out.add(f"gemv_kernel<{T},1,0,plain,1,8>" if (B == 1 and pro == 0) else f"gemv_kernel<{T},{B},{pro},plain,2,4>")
            # csrc/gemv_mx8.hip dl_gemv_mx8 -> gemv_mx8_launch<T, B>
            out |= {f"gemv_mx8_kernel<{T},{B},0,plain,2,4>", f"gemv_mx8_kernel<{T},{B},1,plain,2,4>", f"gemv_mx8_kernel<{T},{B},1,pair,2,4>"}
        if dt == F32:
            continue
        out |= {f"gemv_b1_plain_kernel<{T},1>", f"gemv_b1_plain_kernel<{T},2>", f"gemv_b1_plain_halves_kernel<{T},12>", f"gemv_b1_plain_halves_kernel<{T},16>"}
        for nb in (1, 2):  # csrc/gemm_smallm.hip dl_gemm_smallm, csrc/gemm_mx8.hip dl_gemm_mx8
            out |= {f"gemm_smallm_kernel<{T},{nb},4>", f"gemm_smallm_kernel<{T},{nb},8>", f"gemm_smallm_staged_kernel<{T},{nb},256,8>", f"gemm_smallm_staged_kernel<{T},{nb},128,16>",
                    f"gemm_mx8_kernel<{T},{nb}>"}
        for nu in LP_UNITS:  # csrc/linear_packed.hip lp_nu -> lp_tpw -> lp_epi
            for tpw in (1, 2, 3, 4):
                for epi in (0, 1, 2, 3):
                    if not (epi == 1 and nu % 2):
                        out.add(f"linear_packed_kernel<{T},NU{nu},TPW{tpw},{LP_EPI_NAME[epi]}>")
        for s in LT_SHAPES:  # csrc/linear_tiles.hip lt_shape -> lt_epi
            for epi in ("BIAS", "QGELU", "GELU", "PARTS"):
                out.add(lt_inst(dt, s, 0).replace("BIAS", epi))
        for s in LT_PARTS_ONLY:
            out.add(lt_inst(dt, s, 3))
    return out


def omitted():
    """instantiation -> the one-line reason it has no entry.  Empty: the fp32 prologues and SiLU-pair epilogues of dl_gemv / dl_gemv_mx8 (their results are
    no lattice values) and the GELU / QuickGELU epilogues of dl_linear_tiles are driven by oracle/rowwise_cases.py under its feasible-set criterion."""
    return {}


def driven():
    """Every instantiation of all_instantiations() that a table drives: the tables below, and those of oracle/rowwise_cases.py that reach this family."""
    from oracle import rowwise_cases as rc

    out = set()
    for table, _ in TABLES.values():
        for e in table:
            out |= e["inst"]
    return out | (rc.driven() & all_instantiations())


TABLES = {
    "linear": (LINEAR_TABLE, run_linear),
    "splitk": (SPLITK_TABLE, run_splitk),
    "gemv": (GEMV_TABLE, run_gemv),
    "gemv_mx8": (GEMV_MX8_TABLE, lambda R, e: run_gemv(R, e, mx8=True)),
    "smallm": (SMALLM_TABLE, run_smallm),
    "gemm_mx8": (GEMM_MX8_TABLE, run_gemm_mx8),
    "linear_packed": (LP_TABLE, run_linear_packed),
    "linear_tiles": (LT_TABLE, run_linear_tiles),
}


# ------------------------------------------------------------------------------------------------------------------------------
# the table without a GPU: the specified arithmetic behind hip_ops' signatures (tests/test_linear_truth_cpu.py dry-runs the runners on it)
# ------------------------------------------------------------------------------------------------------------------------------
class ReferenceOps:
    """fp64 products, one rounding, the header's rounding points and k ranges -- on the CPU, with the argument lists of dynamic_llava_amd.hip_ops.  The packing
    calls are the identity (the layouts are the kernels' business); the host queries go to the library."""

    def __init__(self, real_ops):
        self.real = real_ops

    def lib(self):
        return self.real.lib()

    @staticmethod
    def _mm(x, w, k0=0, k1=None):
        return x[:, k0:k1].double() @ w[:, k0:k1].double().T

    @staticmethod
    def _silu_pair(t, dt):
        I = t.shape[1] // 2
        return (torch.nn.functional.silu(t[:, :I].float()).to(dt).float() * t[:, I:].float()).to(dt)

    def _parts(self, x, w, bounds):
        return torch.stack([self._mm(x, w, k0, k1).float() for k0, k1 in bounds])

    def linear(self, a, w, bias=None, flags=0, residual=None, out=None):
        t = self._mm(a, w) + (0 if bias is None else bias.double())
        y = lt.rne(t, a.dtype)
        out.copy_(lt.rne(residual.double() + y.double(), a.dtype) if flags & 2 else y)

    def linear_splitk(self, a, w, parts, n_slices):
        M, K = a.shape
        parts[: n_slices * M * w.shape[0]].view(n_slices, M, -1).copy_(self._parts(a, w, split_bounds(K, 64 if M <= 192 else 128, n_slices)))

    def gemv(self, w, y, x=None, mode=0, h_in=None, h_out=None, delta=None, norm_w=None, eps=0.0, grid_cap=0):
        dt = y.dtype
        if mode & 3 == ADDNORM:
            hn = h_in if delta is None else (h_in.float() + delta.float()).to(dt)
            if delta is not None:
                h_out.copy_(hn)
            x = norm_w * (hn.float() * torch.rsqrt(hn.float().pow(2).mean(-1, keepdim=True) + eps)).to(dt)
        elif mode & 3 == SILUMUL:
            x = self._silu_pair(x, dt)
        t = lt.rne(self._mm(x, w), dt)
        y.copy_(self._silu_pair(t, dt) if mode & PAIR else t)

    def quantize_mx8(self, w, model_dtype=None):
        from dynamic_llava_amd import mxfp8

        return mxfp8.quantize_mx8(w, model_dtype)

    @staticmethod
    def _deq(q, sc):
        from dynamic_llava_amd import mxfp8

        return mxfp8.dequantize_mx8(q, sc, torch.float32)

    def gemv_mx8(self, q, sc, y, **kw):
        self.gemv(self._deq(q, sc), y, **kw)

    def gemm_smallm(self, x, w, out=None, workspace=None, n_slices=0, wg_waves=0, variant=0):
        out.copy_(lt.rne(self._mm(x, w), x.dtype))

    def gemm_smallm_parts(self, x, w, ws, n_slices=0, variant=0):
        M, K = x.shape
        s = int(self.lib().dl_gemm_smallm_slices(M, w.shape[0], K, n_slices, variant))
        v = ws[: s * M * w.shape[0]].view(s, M, -1)
        v.copy_(self._parts(x, w, split_bounds(K, 256, s)))
        return v, s

    def add_rmsnorm_parts(self, h, parts, w=None, eps=1e-6, out=None):
        h.copy_(lt.rne(h.double() + lt.rne(parts.double().sum(0), h.dtype).double(), h.dtype))

    def silu_mul_parts(self, parts, out):
        out.copy_(self._silu_pair(lt.rne(parts.double().sum(0), out.dtype), out.dtype))

    def gemm_mx8(self, x, q, sc, out=None, workspace=None, n_slices=0):
        out.copy_(lt.rne(self._mm(x, self._deq(q, sc)), x.dtype))

    def gemm_mx8_parts(self, x, q, sc, ws, n_slices=0):
        M, K = x.shape
        s = int(self.lib().dl_gemm_mx8_slices(M, q.shape[0], K, n_slices))
        v = ws[: s * M * q.shape[0]].view(s, M, -1)
        v.copy_(self._parts(x, self._deq(q, sc), split_bounds(K, 256, s)))
        return v, s

    def pack_weight_tiles(self, w, gate_up_pairs=False):
        return w

    def pack_x_tiles(self, x):
        return x

    def pack_x_rows(self, x):
        return x

    def linear_packed(self, x, wp, N, out=None, epilogue=0, resid=None, units_per_workgroup=0, k_split=1, workspace=None, err=None, x_packed_mk=None):
        dt = x.dtype
        if epilogue == LP_PARTS:
            out.copy_(self._parts(x, wp, split_bounds(x.shape[1], 64, k_split)))
            return out
        t = lt.rne(self._mm(x, wp), dt)
        if epilogue == LP_SILU_PAIR:
            t = self._silu_pair(t, dt)
        out.copy_(lt.rne(resid.double() + t.double(), dt) if epilogue == LP_RESID else t)
        return out

    def linear_tiles(self, x, wp, N, bias=None, out=None, epilogue=0, x_packed_mk=None, y_packed=False, tile_shape=0, k_split=1):
        dt = x.dtype
        M, K = x.shape
        if epilogue == LT_PARTS:
            out.copy_(self._parts(x, wp, split_bounds(K, 64, k_split)))
            return out
        y = lt.rne(self._mm(x, wp) + (0 if bias is None else bias.double()), dt)
        if y_packed:  # the header's fragment order, written from its statement (unpack_rows reads it back)
            tiles = -(-M // 16)
            yp = torch.zeros(tiles * 16, N, dtype=dt)
            yp[:M] = y
            return yp.view(tiles, 16, N // 64, 2, 4, 8).permute(2, 0, 3, 4, 1, 5).reshape(-1)
        out.copy_(y)
        return out


# ------------------------------------------------------------------------------------------------------------------------------
# the same list read out of the dispatch sources: a new LT_CASE, unit count, batch case or a moved threshold makes the CPU test fail
# ------------------------------------------------------------------------------------------------------------------------------
def _strip_ifdef(src, macro):
    """src without the lines between `#ifdef macro` and its `#endif` (measurement-only instantiations)."""
    import re

    return re.sub(r"#ifdef " + macro + r"\b.*?#endif", "", src, flags=re.S)


def instantiations_in_sources(csrc):
    """The kernel instantiations a release build can launch, parsed from the template arguments, case lists and thresholds of the host dispatch code in
    `csrc` (a directory).  Raises AssertionError when a threshold the *_inst functions restate is no longer in the source as they state it."""
    import os
    import re

    def read(name):
        with open(os.path.join(csrc, name)) as f:
            return f.read()

    T = {"bf16_t": "bf16", "f16_t": "f16", "f32_t": "f32"}
    out = set()
    # linear.hip
    src = read("linear.hip")
    out |= {f"linear_simple_kernel<{T[t]}>" for t in re.findall(r"\(linear_simple_kernel<(\w+)>\)", src)}
    out |= {f"linear_mfma_kernel<{T[t]},{k}>" for t, k in re.findall(r"\(linear_mfma_kernel<(\w+), (\d+)>\)", src)}
    assert src.count("if (K >= 1024) hipLaunchKernelGGL((linear_mfma_kernel<") == 2
    tk = re.search(r"linear_splitk_wide_kernel<TT, (\d+), MTWV>", src).group(1)
    out |= {f"linear_splitk_wide_kernel<{T[t]},{tk},{m}>" for t, m in re.findall(r"DL_WIDE\((\w+_t), (\d+)\)", src)}
    out |= {f"linear_splitk_kernel<{T[t]},{k}>" for t, k in re.findall(r"\(linear_splitk_kernel<(\w+), (\d+)>\)", src)}
    assert "if (M <= 192) {" in src and src.count("if (M <= 128) DL_WIDE(") == 2
    # gemv.hip
    src = read("gemv.hip")
    body = src[src.index('extern "C" int dl_gemv(') :]
    batches = sorted({int(b) for b in re.findall(r"gemv_launch<T, (\d+)>", body)})
    assert batches == list(range(1, 9)) and "default: rc = gemv_launch<T, 8>" in body
    variant = src[src.index("static int gemv_variant(") : src.index("static int gemv_launch(")]
    assert re.findall(r"gemv_go<T, B, MODE, (\w+), (\d), (\d)>", variant) == [("true", "2", "4"), ("false", "1", "8"), ("false", "2", "4")]
    for needle in ("if constexpr (B == 1 && MODE == 0 && Elem<T>::kVec == 8)", "if (K / 8 <= 64 * 16)", "if (K / 8 <= 512)", "if (K / 8 <= 2 * 64 * 16)",
                   "if (((K / 8 + 1) / 2 + 63) / 64 <= 12)", "if constexpr (B == 1 && MODE == 0) return gemv_go<T, B, MODE, false, 1, 8>"):
        assert needle in variant, needle
    launch = src[src.index("static int gemv_launch(") : src.index("// ---- dl_gemv_qkv_attn")]
    modes = sorted(int(m) for m in re.findall(r"gemv_variant<T, B, (\d)>", launch))
    for t in ("bf16", "f16", "f32"):
        for B in batches:
            for m in modes:
                out.add(f"gemv_kernel<{t},{B},{m},pair,2,4>")
                out.add(f"gemv_kernel<{t},1,0,plain,1,8>" if (B == 1 and m == 0) else f"gemv_kernel<{t},{B},{m},plain,2,4>")
    for t in ("bf16", "f16"):
        out |= {f"gemv_b1_plain_kernel<{t},{c}>" for c in re.findall(r"\(gemv_b1_plain_kernel<T, (\d+)>\)", variant)}
        out |= {f"gemv_b1_plain_halves_kernel<{t},{c}>" for c in re.findall(r"\(gemv_b1_plain_halves_kernel<T, (\d+)>\)", variant)}
    # gemv_mx8.hip
    src = read("gemv_mx8.hip")
    assert "constexpr int R = 2, U = 4;" in src
    batches = sorted({int(b) for b in re.findall(r"gemv_mx8_launch<T, (\d+)>", src)})
    forms = re.findall(r"gemv_mx8_go<T, B, (\d), (\w+)>", src)
    for t in ("bf16", "f16", "f32"):
        out |= {f"gemv_mx8_kernel<{t},{B},{m},{'pair' if p == 'true' else 'plain'},2,4>" for B in batches for m, p in forms}
    # gemm_smallm.hip / gemm_mx8.hip
    src = read("gemm_smallm.hip")
    out |= {f"gemm_smallm_kernel<{T[t]},{nb},{nw}>" for t, nb, nw in re.findall(r"sm_go<(\w+), (\d), (\d)>", src)}
    out |= {f"gemm_smallm_staged_kernel<{T[t]},{nb},{kc},{nw}>" for t, nb, kc, nw in re.findall(r"sm_go_staged<(\w+), (\d), (\d+), (\d+)>", src)}
    assert "const bool w8 = wg_waves != 4;" in src and "if (variant == 0) variant = 2;" in src
    out |= {f"gemm_mx8_kernel<{T[t]},{nb}>" for t, nb in re.findall(r"mg_go<(\w+), (\d)>\(DL_MG_ARGS\)", read("gemm_mx8.hip"))}
    # linear_packed.hip: lp_nu (ABL == 0 branch) -> lp_tpw -> lp_epi
    src = _strip_ifdef(_strip_ifdef(read("linear_packed.hip"), "DL_LP_MEASURE_12U"), "DL_LP_ABLATIONS")
    nu_body = src[src.index("static int lp_nu(") :]
    nu_body = nu_body[nu_body.index("} else {") : nu_body.index("dl_linear_packed: units_per_workgroup=%d is not built")]
    units = sorted(int(u) for u in re.findall(r"case (\d+): return lp_tpw<T, \1, ABL>", nu_body))
    tpw_body = src[src.index("static int lp_tpw(") : src.index("static int lp_nu(")]
    tpws = sorted(int(t) for t in re.findall(r"case (\d): return lp_epi<T, NU, \1, ABL>", tpw_body))
    assert "kLpConsumers = 4" in src and "if constexpr (NU % 2 == 0 && ABL == 0) {" in src
    for t in ("bf16", "f16"):
        for nu in units:
            for tpw in tpws:
                for epi in (0, 1, 2, 3):
                    if not (epi == 1 and nu % 2):
                        out.add(f"linear_packed_kernel<{t},NU{nu},TPW{tpw},{LP_EPI_NAME[epi]}>")
    # linear_tiles.hip: lt_shape's two case lists
    src = _strip_ifdef(read("linear_tiles.hip"), "DL_LT_MEASURE")
    for t in ("bf16", "f16"):
        for tm, wn, nuw, wdir, dw in re.findall(r"^\s*LT_CASE\((\d+), (\d), (\d), (\d), (\d)\);", src, flags=re.M):
            assert wdir == "1"
            for epi in ("BIAS", "QGELU", "GELU", "PARTS"):
                out.add(f"linear_tiles_kernel<{t},TM{tm},WN{wn},NUW{nuw},{epi},DW{dw}>")
        for tm, dw in re.findall(r"^\s*LT_CASE_PARTS\((\d+), (\d)\);", src, flags=re.M):
            out.add(f"linear_tiles_kernel<{t},TM{tm},WN4,NUW2,PARTS,DW{dw}>")
    return out
