"""The table behind tests/test_rowwise_exact_gpu.py: one entry per instantiation and branch of the launches that normalise a row or apply an activation, and
the code that drives it.  Expectations: oracle/rowwise_truth.py (a feasible set per element).  Every launch writes into NaN guard bands and is repeated
once with the same bits (Runner.check_set, on oracle/linear_cases.Runner).  docs/rowwise_exactness.md lists the table and what it found.

Row classes: `lattice` (statistics exact in fp32 in any order, RHO_LATTICE) and `generic` (RHO_GENERIC); fp16 additionally gets one non-finite row on the
residual-add paths.  The undecided share of a launch is a property of the reference alone and is capped here (CAP_*), before anything is compared."""
from __future__ import annotations

import os
import re
from functools import lru_cache

import torch

from oracle import linear_cases as lc
from oracle import ref_cpu as orc
from oracle import rowwise_truth as rt

BF16, F16, F32 = rt.BF16, rt.F16, rt.F32
DT = lc.DT
HALF = (BF16, F16)
ALL = (BF16, F16, F32)
EPS = 1e-5
CAP_LATTICE, CAP_GENERIC = 0.005, 0.02
RHO = {"lattice": rt.RHO_LATTICE, "generic": rt.RHO_GENERIC}

# H of the block-per-row kernels: one vector, a ragged first pass, 2056 = 257 vectors and 4104 = 513 (a pair whose second vector one lane holds), whole passes,
# five passes (an odd count for the pair loop), the largest
H_BLOCK = {BF16: (8, 264, 2056, 4096, 4104, 5120, 16384), F16: (8, 264, 2056, 4096, 4104, 5120, 16384), F32: (4, 132, 1028, 4096, 8192)}
H_REFUSED = {BF16: 16392, F16: 16392, F32: 8196}
# H of the wave-per-row kernels: 1, 1, 2, 3, 3, 4, 4, 8, 8 vectors per lane, ragged last passes (520, 1032, 1544, 3592)
H_WAVE = (8, 512, 520, 1032, 1536, 1544, 2048, 3592, 4096)
PARTS_SLICES = (1, 3, 8, 9, 17)


# ------------------------------------------------------------------------------------------------------------------------------
# rows
# ------------------------------------------------------------------------------------------------------------------------------
def _cycle(make, n):
    out, seed = [], 0
    while sum(t.shape[0] for t in out) < n:
        out.append(make(seed))
        seed += 1
    return torch.cat(out)[:n]


@lru_cache(maxsize=256)
def rows(family, cls, H, dtype, n=None, seed=0):
    """fp64 [n, H] of model-dtype values.  family rms / ln; cls lattice / generic."""
    if cls == "lattice":
        make = (lambda s: rt.rms_lattice_rows(H, dtype, 16 * seed + s)) if family == "rms" else (lambda s: rt.ln_lattice_rows(H, dtype, 16 * seed + s))
        k = len(rt.RMS_LATTICE_KINDS if family == "rms" else rt.LN_LATTICE_KINDS)
    else:
        kinds = rt.RMS_GENERIC_KINDS if family == "rms" else rt.LN_GENERIC_KINDS
        make = lambda s: rt.generic_rows(H, dtype, kinds, 16 * seed + s)
        k = len(kinds)
    return _cycle(make, k if n is None else n)


def weight(H, dtype):
    return rt.norm_weight(H).to(dtype)


def bias(H, dtype):
    return rt.norm_bias(H).to(dtype)


def truth(family, x, w, b, cls):
    if family == "rms":
        return rt.rms_truth(x, w, EPS, RHO[cls])
    return rt.ln_truth(x, w, b, EPS, RHO[cls], exact_mean=cls == "lattice")


@lru_cache(maxsize=256)
def add_case(family, cls, H, dtype, n=None, seed=0):
    """-> (h0, delta, x) model dtype, x = RNE_T(h0 + delta): lattice rows are split so that the sum lands back on the lattice."""
    if cls == "lattice":
        x = rows(family, cls, H, dtype, n, seed)
        h0, d = rt.split_add(x, dtype, seed, rt.row_quantum(x))
    else:
        h0 = rows(family, cls, H, dtype, n, seed)
        d = (0.25 * rows(family, cls, H, dtype, n, seed + 7)).to(dtype).double()
        x = rt.to_t(h0 + d, dtype).double()
    return h0.to(dtype), d.to(dtype), x.to(dtype)


@lru_cache(maxsize=256)
def parts_case(family, cls, H, dtype, n_slices, n=None, seed=0, bias_too=False):
    """-> (h0, parts fp32 [n_slices, R, H], lin_bias or None, x): x = RNE_T(h0 + RNE_T(sum of the parts in slice order (+ bias, last)))."""
    h0, d, x = add_case(family, cls, H, dtype, n, seed)
    lb = None
    if cls == "lattice":
        q = rt.row_quantum(x.double())
        if bias_too:  # one bias for all rows: an integer multiple of every row's quantum
            lb = torch.full((H,), float(q.max()), dtype=torch.float64).to(dtype)
        p = rt.split_parts(d.double() - (0 if lb is None else lb.double()), n_slices, seed, q)
        return h0, p, lb, x
    g = torch.Generator().manual_seed(500 + seed + n_slices)
    p = (torch.randn((n_slices,) + tuple(h0.shape), generator=g, dtype=torch.float64) * d.double().abs().clamp_min(2.0**-20) / n_slices**0.5).float()
    acc = torch.zeros(h0.shape, dtype=F32)
    for s in range(n_slices):
        acc = acc + p[s]
    if bias_too:
        lb = (0.1 * d[0].double()).to(dtype)
        acc = acc + lb.float()
    x = (h0.float() + acc.to(dtype).float()).to(dtype)
    return h0, p, lb, x


@lru_cache(maxsize=64)
def nonfinite_case(H, n_slices=0):
    """fp16: h0 = delta = 60000 in two elements, so the residual stream holds +inf there."""
    h0 = rows("rms", "generic", H, F16, 1, seed=3).clone()
    d = (0.25 * rows("rms", "generic", H, F16, 1, seed=4)).clone()
    for k in (1, H - 2):
        h0[0, k] = d[0, k] = 60000.0
    h0, d = h0.to(F16), d.to(F16)
    x = (h0.float() + d.float()).to(F16)
    assert int(torch.isinf(x).sum()) == 2
    return h0, d, x


class PatternOnly(rt.Feasible):
    """Only the NaN / finite pattern of lo (the oracle's output on a non-finite row) is specified."""
    def undecided(self):
        return 0.0

    def ok(self, out):
        out = out.detach().cpu()
        return (torch.isnan(out) == torch.isnan(self.lo)) & (torch.isfinite(out) == torch.isfinite(self.lo))


# ------------------------------------------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class Runner(lc.Runner):
    def __init__(self, ops, device="cuda"):
        super().__init__(ops, device)
        self.undecided = {}

    def check_set(self, tag, fn, F, shape=None, unpack=None, strided=False, cap=None):
        """fn(view) launches into `view`: a contiguous tensor of `shape` (default F's) inside a NaN band, or a strided [M, N] view.  unpack(view) -> the
        tensor F speaks about.  cap: the largest undecided share the reference may have here."""
        shape = tuple(F.shape) if shape is None else tuple(shape)
        und = F.undecided()
        self.undecided[tag] = und
        self.n += 1
        if cap is not None and und > cap:
            self.bad.append(dict(tag=f"{tag}: undecided share {und:.4f} of the reference exceeds {cap}", differing=0, guard_intact=True, second_launch_same=True))
        res = []
        for _ in range(2):
            buf, view = self.out2d(shape[0], shape[1], F.dtype) if strided else self.flat(shape, F.dtype)
            fn(view)
            res.append((buf, view))
        (b0, v0), (b1, v1) = res
        got = (v0 if unpack is None else unpack(v0)).detach().cpu()
        ok = F.ok(got)
        g = b0.clone()
        if strided:
            g[1 : shape[0] + 1, : shape[1]] = float("nan")
        else:
            n = 1
            for s in shape:
                n *= s
            g[64 : 64 + n] = float("nan")
        guard = bool(torch.isnan(g).all())
        same = bool((_bits(v0) == _bits(v1)).all())
        if not (bool(ok.all()) and guard and same):
            idx = torch.nonzero(~ok)
            pick = lambda t: None if t is None else t[~ok][:6].double().tolist()
            self.bad.append(dict(tag=tag, differing=int((~ok).sum()), of=ok.numel(), first=idx[:6].tolist(), got=got[~ok][:6].double().tolist(), lo=pick(F.lo), hi=pick(F.hi),
                                 v=pick(F.v), e=pick(F.e), guard_intact=guard, second_launch_same=same))
        return v0

    def banded(self, t, tag):
        """A contiguous device copy of t inside a NaN band that finish() checks (an in-place residual stream)."""
        buf, view = self.flat(tuple(t.shape), t.dtype)
        view.copy_(t.to(self.dev))
        self.bands.append((tag, buf, 64, 64 + t.numel(), None))
        return view

    def same_bits(self, tag, a, b):
        """a == b as values, NaN equal to NaN (an in-place stream that holds inf / NaN)."""
        self.n += 1
        a, b = a.detach().cpu(), b.detach().cpu()
        eq = (a == b) | (torch.isnan(a) & torch.isnan(b))
        if not bool(eq.all()):
            self.bad.append(dict(tag=tag, differing=int((~eq).sum()), of=a.numel(), first=torch.nonzero(~eq)[:6].tolist(), guard_intact=True, second_launch_same=True))

    def refused(self, tag, fn):
        self.n += 1
        try:
            fn()
        except self.ops.HipOpsError:
            return
        self.bad.append(dict(tag=f"{tag}: not refused", differing=0, guard_intact=True, second_launch_same=True))


def _inplace(R, tag, h0, launch, F, want_h, **kw):
    """launch(h, out): h is updated in place.  A fresh banded h for each of the two launches; both must end as want_h."""
    hs = []

    def fn(out):
        h = R.banded(h0, f"{tag} h")
        hs.append(h)
        launch(h, out)

    R.check_set(tag, fn, F, **kw)
    for h in hs:
        R.same_bits(f"{tag} residual stream", h, want_h)


def _add_only(R, tag, h0, launch, want_h):
    h = R.banded(h0, f"{tag} h")
    launch(h)
    R.same_bits(f"{tag} residual stream", h, want_h)


def _cap(cls, family="rms"):
    return CAP_LATTICE if cls == "lattice" else (CAP_GENERIC if family == "rms" else None)


# ------------------------------------------------------------------------------------------------------------------------------
# dl_rmsnorm / dl_add_rmsnorm / dl_add_rmsnorm_parts
# ------------------------------------------------------------------------------------------------------------------------------
def _t(dt):
    return {BF16: "bf16_t", F16: "f16_t", F32: "f32_t"}[dt]


RMS_TABLE = [dict(id=f"rmsnorm-{DT[dt]}-H{H}", dtype=dt, H=H, inst={f"rmsnorm_kernel<{_t(dt)},0>", f"rmsnorm_kernel<{_t(dt)},1>"}, passes=-(-H // (256 * rt.VEC[dt])))
             for dt in ALL for H in H_BLOCK[dt]]


def run_rms(R, e):
    dt, H = e["dtype"], e["H"]
    ops = R.ops
    w = weight(H, dt)
    wd = R.d(w)
    for cls in ("lattice", "generic"):
        x = rows("rms", cls, H, dt).to(dt)
        xd = R.d(x)
        R.check_set(f"{e['id']} {cls} dl_rmsnorm", lambda out: ops.rmsnorm(xd, wd, EPS, out=out), truth("rms", x, w, None, cls), cap=_cap(cls))
        h0, d, xa = add_case("rms", cls, H, dt)
        dd = R.d(d)
        _inplace(R, f"{e['id']} {cls} dl_add_rmsnorm", h0, lambda h, out: ops.add_rmsnorm(h, dd, wd, EPS, out=out), truth("rms", xa, w, None, cls), xa, cap=_cap(cls))
        _add_only(R, f"{e['id']} {cls} dl_add_rmsnorm w=None", h0, lambda h: ops.add_rmsnorm(h, dd, None, EPS), xa)
    if dt == F16:
        h0, d, xa = nonfinite_case(H)
        dd = R.d(d)
        _inplace(R, f"{e['id']} non-finite dl_add_rmsnorm", h0, lambda h, out: ops.add_rmsnorm(h, dd, wd, EPS, out=out), PatternOnly(dt, lo=orc.rmsnorm(xa, w, EPS), hi=None), xa)
    if H == H_BLOCK[dt][-1]:
        Hr = H_REFUSED[dt]
        z = torch.zeros(2, Hr, dtype=dt, device=R.dev)
        wz = torch.ones(Hr, dtype=dt, device=R.dev)
        R.refused(f"{e['id']} dl_rmsnorm H={Hr}", lambda: ops.rmsnorm(z, wz, EPS))
        R.refused(f"{e['id']} dl_add_rmsnorm H={Hr}", lambda: ops.add_rmsnorm(z, z.clone(), wz, EPS))


RMS_PARTS_TABLE = [dict(id=f"add_rmsnorm_parts-{DT[dt]}-H{H}", dtype=dt, H=H, inst={f"rmsnorm_kernel<{_t(dt)},2>"}, slices=PARTS_SLICES, pairs=-(-H // (512 * rt.VEC[dt])))
                   for dt in ALL for H in H_BLOCK[dt]]


def run_rms_parts(R, e):
    dt, H = e["dtype"], e["H"]
    ops = R.ops
    w = weight(H, dt)
    wd = R.d(w)
    for cls in ("lattice", "generic"):
        for ns in e["slices"]:
            h0, p, _, x = parts_case("rms", cls, H, dt, ns)
            pd = R.d(p)
            tag = f"{e['id']} {cls} n_slices {ns}"
            _inplace(R, tag, h0, lambda h, out: ops.add_rmsnorm_parts(h, pd, wd, EPS, out=out), truth("rms", x, w, None, cls), x, cap=_cap(cls))
            if ns in (3, 9):
                _add_only(R, f"{tag} w=None", h0, lambda h: ops.add_rmsnorm_parts(h, pd, None, EPS), x)
    if H == H_BLOCK[dt][-1]:
        Hr = H_REFUSED[dt]
        R.refused(f"{e['id']} H={Hr}", lambda: ops.add_rmsnorm_parts(torch.zeros(2, Hr, dtype=dt, device=R.dev), torch.zeros(1, 2, Hr, dtype=F32, device=R.dev), torch.ones(Hr, dtype=dt, device=R.dev), EPS))


# ------------------------------------------------------------------------------------------------------------------------------
# the three _packed forms: dl_linear_packed's activation order
# ------------------------------------------------------------------------------------------------------------------------------
def lp_tiles(n_rows):
    return 4 * -(-(-(-n_rows // 16)) // 4)


def unpack_lp(p, n_rows, H, tiles):
    """Xp[step = k / 64][tile][k half][lane = 16 ((k % 32) / 8) + row % 16][8] -> [n_rows, H]."""
    return p[: tiles * 16 * H].view(H // 64, tiles, 2, 4, 16, 8).permute(1, 4, 0, 2, 3, 5).reshape(tiles * 16, H)[:n_rows]


def pack_lp(x, tiles):
    """The inverse (rows past the last one: zero), for the CPU stand-in."""
    n, H = x.shape
    xp = torch.zeros(tiles * 16, H, dtype=x.dtype)
    xp[:n] = x
    return xp.view(tiles, 16, H // 64, 2, 4, 8).permute(2, 0, 3, 4, 1, 5).reshape(-1)


PACKED_TABLE = [dict(id=f"rmsnorm_packed-{DT[dt]}-R{n}-H{H}", dtype=dt, rows=n, H=H, inst={f"rmsnorm_kernel<{_t(dt)},{a}>+packed" for a in (0, 1, 2)})
                for dt in HALF for n in (1, 17, 256) for H in (64, 4096, 5120)]


def _mixed_rows(family, H, dt, n):
    """n rows: lattice rows first (half), generic rows after; -> list of (cls, slice)."""
    nl = (n + 1) // 2
    return [("lattice", slice(0, nl), nl)] + ([("generic", slice(nl, n), n - nl)] if n > nl else [])


def run_rms_packed(R, e):
    dt, n, H = e["dtype"], e["rows"], e["H"]
    ops = R.ops
    w = weight(H, dt)
    wd = R.d(w)
    tiles = lp_tiles(n)
    shape = (tiles * 16 * H,)
    unpack = lambda p: unpack_lp(p, n, H, tiles)
    groups = _mixed_rows("rms", H, dt, n)
    # plain
    x = torch.cat([rows("rms", cls, H, dt, k).to(dt) for cls, _, k in groups])
    F = rt.stack([truth("rms", x[sl], w, None, cls) for cls, sl, _ in groups])
    xd = R.d(x)
    y = R.check_set(f"{e['id']} dl_rmsnorm_packed", lambda out: ops.rmsnorm(xd, wd, EPS, out=out, packed=True), F, shape=shape, unpack=unpack, cap=CAP_GENERIC)
    z = R.check_set(f"{e['id']} dl_rmsnorm", lambda out: ops.rmsnorm(xd, wd, EPS, out=out), F, cap=CAP_GENERIC)
    R.same_bits(f"{e['id']} dl_rmsnorm_packed == dl_rmsnorm", unpack(y), z)
    # add
    cs = [add_case("rms", cls, H, dt, k) for cls, _, k in groups]
    h0, d, xa = (torch.cat([c[i] for c in cs]) for i in range(3))
    F = rt.stack([truth("rms", xa[sl], w, None, cls) for cls, sl, _ in groups])
    dd = R.d(d)
    outs = []
    _inplace(R, f"{e['id']} dl_add_rmsnorm_packed", h0, lambda h, out: outs.append(ops.add_rmsnorm(h, dd, wd, EPS, out=out, packed=True)), F, xa, shape=shape, unpack=unpack, cap=CAP_GENERIC)
    _inplace(R, f"{e['id']} dl_add_rmsnorm", h0, lambda h, out: outs.append(ops.add_rmsnorm(h, dd, wd, EPS, out=out)), F, xa, cap=CAP_GENERIC)
    R.same_bits(f"{e['id']} dl_add_rmsnorm_packed == dl_add_rmsnorm", unpack(outs[0]), outs[2])
    # parts
    for ns in (3, 9):
        cs = [parts_case("rms", cls, H, dt, ns, k) for cls, _, k in groups]
        h0, p, xa = torch.cat([c[0] for c in cs]), torch.cat([c[1] for c in cs], 1).contiguous(), torch.cat([c[3] for c in cs])
        F = rt.stack([truth("rms", xa[sl], w, None, cls) for cls, sl, _ in groups])
        pd = R.d(p)
        outs = []
        _inplace(R, f"{e['id']} dl_add_rmsnorm_parts_packed n_slices {ns}", h0, lambda h, out: outs.append(ops.add_rmsnorm_parts(h, pd, wd, EPS, out=out, packed=True)), F, xa, shape=shape,
                 unpack=unpack, cap=CAP_GENERIC)
        _inplace(R, f"{e['id']} dl_add_rmsnorm_parts n_slices {ns}", h0, lambda h, out: outs.append(ops.add_rmsnorm_parts(h, pd, wd, EPS, out=out)), F, xa, cap=CAP_GENERIC)
        R.same_bits(f"{e['id']} dl_add_rmsnorm_parts_packed == dl_add_rmsnorm_parts", unpack(outs[0]), outs[2])
    if n == 256:
        z = torch.zeros(257, H, dtype=dt, device=R.dev)
        R.refused(f"{e['id']} rows 257", lambda: ops.rmsnorm(z, wd, EPS, packed=True))
        R.refused(f"{e['id']} add rows 257", lambda: ops.add_rmsnorm(z, z.clone(), wd, EPS, packed=True))
        R.refused(f"{e['id']} parts rows 257", lambda: ops.add_rmsnorm_parts(z, torch.zeros(1, 257, H, dtype=F32, device=R.dev), wd, EPS, packed=True))


# ------------------------------------------------------------------------------------------------------------------------------
# dl_layernorm / dl_add_layernorm (a workgroup per row)
# ------------------------------------------------------------------------------------------------------------------------------
LN_TABLE = [dict(id=f"layernorm-{DT[dt]}-H{H}", dtype=dt, H=H, inst={f"layernorm_kernel<{_t(dt)},false>", f"layernorm_kernel<{_t(dt)},true>"}) for dt in ALL for H in H_BLOCK[dt]]


def _und_rows(R, tag, F):
    """LayerNorm generic rows have no cap: the undecided share of every row is recorded (the GPU test prints it)."""
    for i in range(F.shape[0]):
        R.undecided[f"{tag} row {i}"] = F.rows(slice(i, i + 1)).undecided()


def run_ln(R, e):
    dt, H = e["dtype"], e["H"]
    ops = R.ops
    w, b = weight(H, dt), bias(H, dt)
    wd, bd = R.d(w), R.d(b)
    for cls in ("lattice", "generic"):
        x = rows("ln", cls, H, dt).to(dt)
        F = truth("ln", x, w, b, cls)
        xd = R.d(x)
        n = x.shape[0]
        if cls == "generic":
            _und_rows(R, f"{e['id']} generic dl_layernorm", F)
        R.check_set(f"{e['id']} {cls} dl_layernorm", lambda out: ops.layernorm(xd, wd, bd, EPS, out=out), F, cap=_cap(cls, "ln"))
        idx = torch.tensor([n - 1, 0, 0] + list(range(1, n)), dtype=torch.int32)  # a gather with a repeat and a permutation
        Fi = F.rows(idx.long())
        idx_d = R.d(idx)
        R.check_set(f"{e['id']} {cls} dl_layernorm row_index", lambda out: ops.layernorm(xd, wd, bd, EPS, row_index=idx_d, rows=idx.numel(), out=out), Fi, cap=_cap(cls, "ln"))
        h0, d, xa = add_case("ln", cls, H, dt)
        dd = R.d(d)
        _inplace(R, f"{e['id']} {cls} dl_add_layernorm", h0, lambda h, out: ops.add_layernorm(h, dd, wd, bd, EPS, out=out), truth("ln", xa, w, b, cls), xa, cap=_cap(cls, "ln"))
        _add_only(R, f"{e['id']} {cls} dl_add_layernorm w=None", h0, lambda h: ops.add_layernorm(h, dd), xa)
    if dt == F16:
        h0, d, xa = nonfinite_case(H)
        dd = R.d(d)
        want = torch.nn.functional.layer_norm(xa.float(), (H,), w.float(), b.float(), EPS).to(dt)
        _inplace(R, f"{e['id']} non-finite dl_add_layernorm", h0, lambda h, out: ops.add_layernorm(h, dd, wd, bd, EPS, out=out), PatternOnly(dt, lo=want, hi=None), xa)
    if H == H_BLOCK[dt][-1]:
        Hr = H_REFUSED[dt]
        z = torch.zeros(2, Hr, dtype=dt, device=R.dev)
        wz = torch.ones(Hr, dtype=dt, device=R.dev)
        R.refused(f"{e['id']} dl_layernorm H={Hr}", lambda: ops.layernorm(z, wz, wz, EPS))
        R.refused(f"{e['id']} dl_add_layernorm H={Hr}", lambda: ops.add_layernorm(z, z.clone(), wz, wz, EPS))


# ------------------------------------------------------------------------------------------------------------------------------
# dl_layernorm_rows / dl_add_layernorm_rows / dl_add_layernorm_parts (a wave per row)
# ------------------------------------------------------------------------------------------------------------------------------
def vpl(H):
    return -(-(H // 8) // 64)


def ln_wave_inst(dt, add, H, n_slices=0):
    v = vpl(H)
    ns = n_slices if (add == 2 and v <= 2 and n_slices in (2, 4)) else 0
    return f"layernorm_wave_kernel<{_t(dt)},{add},{v},{ns}>"


def _wave_slices(H):
    return (2, 4, 3)  # 2 and 4: the NS specialisations at <= 2 vectors per lane, the generic loop beyond (4 at H = 4096); 3: always the generic loop


LN_WAVE_TABLE = [dict(id=f"layernorm_rows-{DT[dt]}-H{H}", dtype=dt, H=H, vpl=vpl(H), ragged=(H // 8) % 64 != 0,
                      inst={ln_wave_inst(dt, 0, H), ln_wave_inst(dt, 1, H)} | {ln_wave_inst(dt, 2, H, ns) for ns in _wave_slices(H)}) for dt in HALF for H in H_WAVE]
H_WAVE_REFUSED = 2056  # 5 vectors per lane


def tiles_rows(n_rows):
    return -(-n_rows // 16)


def run_ln_wave(R, e):
    dt, H = e["dtype"], e["H"]
    ops = R.ops
    w, b = weight(H, dt), bias(H, dt)
    wd, bd = R.d(w), R.d(b)
    packed = H % 64 == 0
    for cls in ("lattice", "generic"):
        cap = _cap(cls, "ln")
        x = rows("ln", cls, H, dt).to(dt)
        n = x.shape[0]
        tiles = tiles_rows(n)
        pshape, unpack = (tiles * 16 * H,), (lambda p: unpack_lp(p, n, H, tiles))
        F = truth("ln", x, w, b, cls)
        if cls == "generic":
            _und_rows(R, f"{e['id']} generic dl_layernorm_rows", F)
        xd = R.d(x)
        y = R.check_set(f"{e['id']} {cls} dl_layernorm_rows", lambda out: ops.layernorm_rows(xd, wd, bd, EPS, out=out), F, cap=cap)
        if packed:
            yp = R.check_set(f"{e['id']} {cls} dl_layernorm_rows packed", lambda out: ops.layernorm_rows(xd, wd, bd, EPS, out=out, packed=True), F, shape=pshape, unpack=unpack, cap=cap)
            R.same_bits(f"{e['id']} {cls} packed == row-major", unpack(yp), y)
        h0, d, xa = add_case("ln", cls, H, dt)
        dd = R.d(d)
        Fa = truth("ln", xa, w, b, cls)
        _inplace(R, f"{e['id']} {cls} dl_add_layernorm_rows", h0, lambda h, out: ops.add_layernorm_rows(h, dd, wd, bd, EPS, out=out), Fa, xa, cap=cap)
        if packed:
            _inplace(R, f"{e['id']} {cls} dl_add_layernorm_rows packed", h0, lambda h, out: ops.add_layernorm_rows(h, dd, wd, bd, EPS, out=out, packed=True), Fa, xa, shape=pshape,
                     unpack=unpack, cap=cap)
        _add_only(R, f"{e['id']} {cls} dl_add_layernorm_rows w=None", h0, lambda h: ops.add_layernorm_rows(h, dd), xa)
        for ns in _wave_slices(H):
            for with_bias in (False, True):
                h0, p, lb, xp = parts_case("ln", cls, H, dt, ns, None, 0, with_bias)
                pd, lbd = R.d(p), R.d(lb)
                Fp = truth("ln", xp, w, b, cls)
                tag = f"{e['id']} {cls} dl_add_layernorm_parts n_slices {ns} bias {with_bias}"
                _inplace(R, tag, h0, lambda h, out: ops.add_layernorm_parts(h, pd, lbd, wd, bd, EPS, out=out), Fp, xp, cap=cap)
                if packed and with_bias:
                    _inplace(R, f"{tag} packed", h0, lambda h, out: ops.add_layernorm_parts(h, pd, lbd, wd, bd, EPS, out=out, packed=True), Fp, xp, shape=pshape, unpack=unpack, cap=cap)
                if ns == 3:
                    _add_only(R, f"{tag} w=None", h0, lambda h: ops.add_layernorm_parts(h, pd, lbd), xp)
    if dt == F16:
        h0, d, xa = nonfinite_case(H)
        dd = R.d(d)
        want = torch.nn.functional.layer_norm(xa.float(), (H,), w.float(), b.float(), EPS).to(dt)
        _inplace(R, f"{e['id']} non-finite dl_add_layernorm_rows", h0, lambda h, out: ops.add_layernorm_rows(h, dd, wd, bd, EPS, out=out), PatternOnly(dt, lo=want, hi=None), xa)
    if H == H_WAVE[-1]:
        Hr = H_WAVE_REFUSED
        z = torch.zeros(2, Hr, dtype=dt, device=R.dev)
        wz = torch.ones(Hr, dtype=dt, device=R.dev)
        R.refused(f"{e['id']} dl_layernorm_rows H={Hr}", lambda: ops.layernorm_rows(z, wz, wz, EPS))
        R.refused(f"{e['id']} dl_add_layernorm_rows H={Hr}", lambda: ops.add_layernorm_rows(z, z.clone(), wz, wz, EPS))
        R.refused(f"{e['id']} dl_add_layernorm_parts H={Hr}", lambda: ops.add_layernorm_parts(z, torch.zeros(2, 2, Hr, dtype=F32, device=R.dev), None, wz, wz, EPS))


# ------------------------------------------------------------------------------------------------------------------------------
# dl_compact_tokens with norm_w
# ------------------------------------------------------------------------------------------------------------------------------
COMPACT_TABLE = [dict(id=f"compact_tokens-{DT[dt]}-H264", dtype=dt, H=264, inst={f"compact_tokens+rmsnorm<{_t(dt)}>"}) for dt in ALL]


def run_compact(R, e):
    """One sequence of 2 + 9 + 2 tokens whose image span holds the lattice and the generic rows; 5 of the 9 image tokens are kept."""
    dt, H = e["dtype"], e["H"]
    w = weight(H, dt)
    xl, xg = rows("rms", "lattice", H, dt).to(dt), rows("rms", "generic", H, dt).to(dt)
    h = torch.cat([xg[:2], xl, xg, xl[:2]])  # 2 + 5 + 4 + 2
    n_img, k, start = 9, 5, 2
    keep = torch.tensor([[0, 2, 4, 5, 8]])
    cu, cu2 = torch.tensor([0, 13], dtype=torch.int32), torch.tensor([0, 9], dtype=torch.int32)
    sel = [0, 1] + [start + int(i) for i in keep[0]] + [11, 12]
    cls_of = ["generic"] * 2 + ["lattice"] * 5 + ["generic"] * 4 + ["lattice"] * 2
    F = rt.stack([truth("rms", h[i : i + 1], w, None, cls_of[i]) for i in sel])
    args = (R.d(h), R.d(keep), R.d(cu), R.d(cu2), R.d(torch.tensor([start], dtype=torch.int32)), n_img, k, 9, R.d(w), EPS)
    outs = []

    def fn(out):
        h_out, pos, x_out = R.ops.compact_tokens(*args)
        outs.append((h_out, pos))
        out.copy_(x_out)

    R.check_set(f"{e['id']} fused rmsnorm", fn, F, cap=CAP_GENERIC)
    R.same_bits(f"{e['id']} rows", outs[0][0], h[sel])
    R.same(f"{e['id']} positions", outs[0][1].cpu().long(), torch.tensor(sel))


# ------------------------------------------------------------------------------------------------------------------------------
# gemv_build_x seen directly: W = I, so y[b, n] = x[b, n] with a single term
# ------------------------------------------------------------------------------------------------------------------------------
PLAIN, ADDNORM, SILUMUL, PAIR = lc.PLAIN, lc.ADDNORM, lc.SILUMUL, lc.PAIR
MAXC_K = {BF16: 8192, F16: 8192, F32: 4096}  # K up to here: the prologue's rows stay in registers (256 threads x MAXC = 4 vectors); beyond: LDS
GEMV_K = (512, 4104, 8200, 12296)


def _prologue_branch(K, dt):
    return "registers" if K <= MAXC_K[dt] else "lds"


def _build_x_entries():
    out = []
    for dt in ALL:
        for K in GEMV_K:
            for mode in (ADDNORM, SILUMUL):
                Bs = list(range(1, 9)) if K == 512 else [1, 3, 8]
                out.append(dict(id=f"build_x-{DT[dt]}-{lc.MODE_NAME[mode]}-K{K}", dtype=dt, K=K, mode=mode, batches=Bs, branch=_prologue_branch(K, dt) if mode == ADDNORM else "n/a",
                                inst={lc.gemv_inst(dt, B, mode, K) for B in Bs} | ({lc.gemv_mx8_inst(dt, B, mode) for B in Bs} if (mode == ADDNORM and K % 32 == 0) else set())))
    return out


BUILD_X_TABLE = _build_x_entries()
PK_IDENTITY_K = (1024, 4096)  # dl_gemv_pk's ADDNORM shapes (K % 1024 == 0, K <= 8192, bf16, one row)
BUILD_X_PK_TABLE = [dict(id=f"build_x_pk-bf16-ADDNORM-K{K}", dtype=BF16, K=K, mode=ADDNORM, inst={f"gemv_pk ADDNORM K{K}"}) for K in PK_IDENTITY_K]


def silumul_rows(cls, B, K, dt, seed=0):
    """gate|up [B, 2K]: `values` walks through the finite values of the dtype (fp32: bf16's) against the eight up values; `generic` is randn x {0.01, 1, 6, 40}."""
    g = torch.Generator().manual_seed(700 + seed + B)
    if cls == "lattice":
        vals = rt.all_values(dt if dt != F32 else BF16).float()
        vals = vals[torch.isfinite(vals) & (vals.abs() <= (512.0 if dt == F16 else 2.0**100))]  # silu(g) u stays finite: W = I multiplies every x by 0
        gate = vals[torch.randint(0, vals.numel(), (B, K), generator=g)]
        ups = rt.up_values(dt if dt != F32 else BF16).float()
        up = ups[torch.randint(0, 8, (B, K), generator=g)]
    else:
        scale = torch.tensor([0.01, 1.0, 6.0, 40.0])[torch.randint(0, 4, (B, K), generator=g)]
        gate = torch.randn(B, K, generator=g) * scale
        up = torch.randn(B, K, generator=g)
    return torch.cat([gate, up], 1).to(dt)


def _identity(R, K, dt):
    return torch.eye(K, dtype=dt, device=R.dev)


def run_build_x(R, e, pk=False):
    dt, K, mode = e["dtype"], e["K"], e["mode"]
    ops = R.ops
    eye = _identity(R, K, dt)
    routes = []
    if pk:
        from dynamic_llava_amd import bf16pack as bp

        p = getattr(ops, "pack_bf16", lambda t: bp.pack(t, force=True))(eye)
        routes.append(("dl_gemv_pk", lambda y, **kw: ops.gemv_pk(p, y, mode=mode, **kw)))
        Bs = [1]
    else:
        maxb = ops.gemv_max_batch(K, dt)
        Bs = [B for B in e["batches"] if B <= maxb]
        routes.append(("dl_gemv", lambda y, **kw: ops.gemv(eye, y, mode=mode, **kw)))
        if mode == ADDNORM and K % 32 == 0:
            q, sc = ops.quantize_mx8(eye, model_dtype=dt)
            from dynamic_llava_amd import mxfp8

            R.same(f"{e['id']} the identity quantises exactly", mxfp8.dequantize_mx8(q.cpu(), sc.cpu(), torch.float32), torch.eye(K))
            routes.append(("dl_gemv_mx8", lambda y, **kw: ops.gemv_mx8(q, sc, y, mode=mode, **kw)))
    w = weight(K, dt)
    wd = R.d(w)
    for B in Bs:
        for cls in ("lattice", "generic"):
            for name, go in routes:
                tag = f"{e['id']} {name} B{B} {cls}"
                if mode == ADDNORM:
                    h0, d, xa = add_case("rms", cls, K, dt, B, seed=B)
                    for with_delta in (True, False):
                        hn = xa if with_delta else h0
                        F = truth("rms", hn, w, None, cls)
                        h_in, dd = R.d(h0), (R.d(d) if with_delta else None)
                        h_outs = []

                        def fn(y):
                            ho = R.banded(torch.full((B, K), float("nan"), dtype=dt), f"{tag} h_out") if with_delta else None
                            h_outs.append(ho)
                            go(y, h_in=h_in, h_out=ho, delta=dd, norm_w=wd, eps=EPS)

                        R.check_set(f"{tag} delta {with_delta}", fn, F, strided=True, cap=_cap(cls))
                        if with_delta:
                            for ho in h_outs:
                                R.same_bits(f"{tag} h_out", ho, xa)
                else:
                    gu = silumul_rows(cls, B, K, dt)
                    F = rt.silu_mul_truth(gu[:, :K], gu[:, K:])
                    gud = R.strided(gu)
                    R.check_set(tag, lambda y: go(y, x=gud), F, strided=True, cap=CAP_GENERIC)
    del eye


# ------------------------------------------------------------------------------------------------------------------------------
# activations: every 16-bit input
# ------------------------------------------------------------------------------------------------------------------------------
ACT_TABLE = [dict(id=f"silu_mul-{DT[dt]}", dtype=dt, op="silu_mul", inst={f"silu_mul_kernel<{_t(dt)},false>", f"silu_mul_kernel<{_t(dt)},true>"}) for dt in ALL] + \
            [dict(id=f"silu_mul_parts-{DT[dt]}", dtype=dt, op="silu_mul_parts", inst={f"silu_mul_parts_kernel<{_t(dt)}>"}) for dt in ALL] + \
            [dict(id=f"quick_gelu-{DT[dt]}", dtype=dt, op="quick_gelu", inst={f"quick_gelu_kernel<{_t(dt)},false>", f"quick_gelu_kernel<{_t(dt)},true>"}) for dt in ALL]


@lru_cache(maxsize=None)
def act_inputs(dt):
    """-> (gate_up [8, 2 I], finite mask [I]): row r pairs every gate with up value r."""
    if dt == F32:  # one row: the eight up values cycled along the sweep
        g = rt.fp32_gates()
        up = rt.up_values(BF16).float()[torch.arange(g.numel()) % 8]
        return torch.cat([g, up])[None].contiguous(), torch.isfinite(g)
    else:
        g = rt.all_values(dt)
        ups = rt.up_values(dt)
    gate = g[None, :].expand(8, -1)
    up = ups[:, None].expand(-1, g.numel())
    return torch.cat([gate, up], 1).contiguous(), torch.isfinite(g.float())


class exact_act:
    """DL_EXACT_ACT=1 for the launches inside (the library reads it at every call)."""
    def __enter__(self):
        self.old = os.environ.get("DL_EXACT_ACT")
        os.environ["DL_EXACT_ACT"] = "1"

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["DL_EXACT_ACT"]
        else:
            os.environ["DL_EXACT_ACT"] = self.old


class FiniteGates(rt.Feasible):
    """The criterion on the columns of finite gates only."""
    fin = None

    def ok(self, out):
        return rt.Feasible.ok(self, out) | ~self.fin

    def undecided(self):
        if self.lo is None:
            return 0.0
        return float(((self.lo != self.hi) & self.fin).double().sum() / self.fin.double().sum())


def _finite(F, fin_mask):
    G = FiniteGates(F.dtype, F.lo, F.hi, F.v, F.e)
    G.fin = fin_mask.expand(tuple(F.shape))
    return G


def _agree_on_nonfinite(R, tag, a, b, fin):
    """finite gates: bit-equal; non-finite gates: bit-equal or both NaN."""
    R.n += 1
    a, b = a.detach().cpu(), b.detach().cpu()
    bits = _bits(a) == _bits(b)
    ok = torch.where(fin.expand(tuple(a.shape)), bits, bits | (torch.isnan(a) & torch.isnan(b)))
    if not bool(ok.all()):
        R.bad.append(dict(tag=tag, differing=int((~ok).sum()), of=ok.numel(), first=torch.nonzero(~ok)[:6].tolist(), guard_intact=True, second_launch_same=True))


def run_act(R, e):
    dt, op = e["dtype"], e["op"]
    ops = R.ops
    gu, fin = act_inputs(dt)
    I = gu.shape[1] // 2
    if op == "quick_gelu":
        x = gu[0, :I].contiguous()
        F = _finite(rt.quick_gelu_truth(torch.where(fin, x, torch.zeros_like(x))), fin)
        xd = R.d(x)
        a = R.check_set(f"{e['id']} default", lambda out: ops.quick_gelu(xd, out=out), F, cap=CAP_GENERIC)
        with exact_act():
            b = R.check_set(f"{e['id']} DL_EXACT_ACT=1", lambda out: ops.quick_gelu(xd, out=out), F, cap=CAP_GENERIC)
        _agree_on_nonfinite(R, f"{e['id']} default == exact", a, b, fin)
        return
    g = torch.where(fin[None, :], gu[:, :I], torch.zeros_like(gu[:, :I]))
    F = _finite(rt.silu_mul_truth(g, gu[:, I:]), fin[None, :])
    if op == "silu_mul":
        gud = R.d(gu)
        a = R.check_set(f"{e['id']} default", lambda out: ops.silu_mul(gud, out=out), F, cap=CAP_GENERIC)
        with exact_act():
            b = R.check_set(f"{e['id']} DL_EXACT_ACT=1", lambda out: ops.silu_mul(gud, out=out), F, cap=CAP_GENERIC)
        _agree_on_nonfinite(R, f"{e['id']} default == exact", a, b, fin[None, :])
    else:  # one fp32 slice that holds the 16-bit values: cast(sum) is the value itself
        pd = R.d(gu.float()[None].contiguous())
        R.check_set(f"{e['id']} one slice", lambda out: ops.silu_mul_parts(pd, out), F, cap=CAP_GENERIC)


# ------------------------------------------------------------------------------------------------------------------------------
# the same activations inside the GEMM / GEMV epilogues: K = 64, x[m, 0] = 1, W_gate[n, 0] = the n-th 16-bit value
# ------------------------------------------------------------------------------------------------------------------------------
EPI_K = 64


@lru_cache(maxsize=None)
def epi_gates(dt):
    """All 16-bit values (fp32: bf16's, |g| < 2^100) with the non-finite ones replaced by 0, and the up value of each: the eight, cycled."""
    g = rt.all_values(dt if dt != F32 else BF16).float()
    g = torch.where(torch.isfinite(g) & ((g.abs() < 2.0**100) | (dt != F32)), g, torch.zeros_like(g))
    ups = rt.up_values(dt if dt != F32 else BF16).float()
    return g.to(dt), ups[torch.arange(g.numel()) % 8].to(dt)


def _epi_x(M, dt, seed=0):
    g = torch.Generator().manual_seed(900 + seed)
    x = (torch.randint(0, 2, (M, EPI_K), generator=g).float() * 2 - 1) * torch.randint(1, 3, (M, EPI_K), generator=g).float()
    x[:, 0] = 1.0
    return x.to(dt)


def _col0(vals, dt):
    w = torch.zeros(vals.numel(), EPI_K, dtype=dt)
    w[:, 0] = vals
    return w


def silu_pair_interval(vg, eg, vu, eu):
    """fp32: out = fl(fl(silu(g)) u) with g in vg +- eg, u in vu +- eu (|silu'| <= 1.1)."""
    s = rt.silu64(vg)
    over, edge = rt.exp_overflows(vg)
    s = torch.where(over, torch.zeros_like(s), s)
    v = s * vu
    e = 1.1 * eg * (vu.abs() + eu) + s.abs() * eu + v.abs() * (rt.RHO_ACT + 2 * rt.U32) + rt.TINY32 * (1 + vu.abs())
    e = torch.where(edge | (rt.exp_overflows(vg - eg)[0] != rt.exp_overflows(vg + eg)[0]), e + (rt.silu64(vg) * vu).abs() * 1.01, e)
    return rt.Feasible(F32, v=v, e=e)


def _gemv_pair_modes(dt):
    return (PLAIN, ADDNORM, SILUMUL) if dt == F32 else (PLAIN,)


GEMV_PAIR_TABLE = [dict(id=f"gemv_pair-{DT[dt]}-B{B}-{lc.MODE_NAME[m]}", dtype=dt, B=B, mode=m | PAIR, inst={lc.gemv_inst(dt, B, m | PAIR, EPI_K)})
                   for dt in ALL for B in (range(1, 9) if dt == F32 else (1, 8)) for m in _gemv_pair_modes(dt)]


def _x0_operands(R, B, dt, pro):
    """-> (kwargs of the launch, v0 [B, 1], e0 [B, 1], h_out check or None): the prologue's x with x[b, 0] = v0 +- e0 (exactly 1 for PLAIN)."""
    one = torch.ones(B, 1, dtype=torch.float64)
    if pro == PLAIN:
        return dict(x=R.strided(_epi_x(B, dt, B))), one, 0 * one, None
    if pro == ADDNORM:  # h + delta = +-1 everywhere (+1 in column 0): mean(hn^2) = 1, x0 = norm_w[0] RNE_T(r), norm_w[0] = 1
        sign = _epi_x(B, dt, B).double().sign()
        nw = weight(EPI_K, dt).clone()
        nw[0] = 1.0
        F = rt.rms_truth(sign.to(dt), nw, EPS, rt.RHO_LATTICE)
        ho = torch.full((B, EPI_K), float("nan"), dtype=dt, device=R.dev)
        kw = dict(h_in=R.d((3 * sign).to(dt)), delta=R.d((-2 * sign).to(dt)), norm_w=R.d(nw), eps=EPS, h_out=ho)
        if dt == F32:
            return kw, F.v[:, :1], F.e[:, :1], (ho, sign.to(dt))
        assert torch.equal(F.lo[:, :1].double(), one) and torch.equal(F.hi[:, :1].double(), one)
        return kw, one, 0 * one, (ho, sign.to(dt))
    gu = torch.cat([_epi_x(B, dt, B), _epi_x(B, dt, B + 1)], 1)  # SILUMUL: gate 16, up 1 in column 0
    gu[:, 0] = 16.0
    F = rt.silu_mul_truth(gu[:, :EPI_K], gu[:, EPI_K:])
    if dt == F32:
        return dict(x=R.strided(gu)), F.v[:, :1], F.e[:, :1], None
    assert torch.equal(F.lo[:, :1].double(), 16 * one) and torch.equal(F.hi[:, :1].double(), 16 * one)
    return dict(x=R.strided(gu)), 16 * one, 0 * one, None


def _pair_truth(dt, gates, ups, v0, e0):
    """y[b, i] for gate accumulators gates[i] x0[b] and up accumulators ups[i] x0[b]."""
    g64, u64 = gates.double()[None, :], ups.double()[None, :]
    if dt != F32:
        assert float(e0.abs().max()) == 0.0
        g = rt.to_t(g64 * v0, dt)  # one exact term: the accumulator is the product, cast(acc) its rounding
        u = rt.to_t(u64 * v0, dt)
        return rt.silu_mul_truth(g, u)
    vg, vu = g64 * v0, u64 * v0
    return silu_pair_interval(vg, g64.abs() * e0 + vg.abs() * rt.U32 + rt.TINY32, vu, u64.abs() * e0 + vu.abs() * rt.U32 + rt.TINY32)


def run_gemv_pair(R, e, mx8=False):
    dt, B, mode = e["dtype"], e["B"], e["mode"]
    ops = R.ops
    if mx8:
        gates, ups = mx8_gates(dt)
    else:
        gates, ups = epi_gates(dt)
    w = torch.cat([_col0(gates, dt), _col0(ups, dt)])
    kw, v0, e0, ho = _x0_operands(R, B, dt, mode & 3)
    if mx8:
        from dynamic_llava_amd import mxfp8

        qh, sh = mxfp8.quantize_mx8(w, dt)
        assert torch.equal(mxfp8.dequantize_mx8(qh, sh, torch.float32).double(), w.double()), "the weights must be exactly e4m3fn x E8M0"
        q, sc = ops.quantize_mx8(R.d(w), model_dtype=dt)
        R.same(f"{e['id']} dl_quantize_mx8 codes", q, qh)
        R.same(f"{e['id']} dl_quantize_mx8 scales", sc, sh)
        go = lambda y: ops.gemv_mx8(q, sc, y, mode=mode, **kw)
    else:
        wd = R.d(w)
        go = lambda y: ops.gemv(wd, y, mode=mode, **kw)
    F = _pair_truth(dt, gates, ups, v0, e0)
    R.check_set(f"{e['id']}", go, F, strided=True, cap=CAP_GENERIC)
    if ho is not None:
        R.same_bits(f"{e['id']} h_out", ho[0], ho[1])


@lru_cache(maxsize=None)
def mx8_gates(dt):
    """A sample, not an enumeration: m 2^e with m in {1, 1.125, .., 1.75} (the e4m3 mantissas below the saturation at 1.75 x 2^8) and e in [-20, 7]."""
    m = torch.tensor([1.0, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, -1.25])
    ex = 2.0 ** torch.arange(-20, 8, dtype=torch.float32)
    g = (m[:, None] * ex[None, :]).reshape(-1)
    ups = rt.up_values(dt if dt != F32 else BF16).float()
    ups = torch.where(ups == ups[2], torch.tensor(1.5), ups)    # 1 + ulp and 0.333 are no e4m3 values: 1.5 and 0.3125 instead
    ups = torch.where(ups == ups[4], torch.tensor(0.3125), ups)
    ups = torch.where(ups == ups[5], torch.tensor(96.0), ups)   # 100 = 1.5625 x 2^6 needs four mantissa bits
    return g.to(dt), ups[torch.arange(g.numel()) % 8].to(dt)


GEMV_MX8_PAIR_TABLE = [dict(id=f"gemv_mx8_pair-{DT[dt]}-B{B}", dtype=dt, B=B, mode=ADDNORM | PAIR, inst={lc.gemv_mx8_inst(dt, B, ADDNORM | PAIR)})
                       for dt in ALL for B in (range(1, 9) if dt == F32 else (1, 8))]

LP_PAIR_TABLE = [dict(id=f"linear_packed_pair-{DT[dt]}-M{M}", dtype=dt, M=M, inst={f"linear_packed_kernel<{DT[dt]},NUauto,TPW1,SILU_PAIR> rounding store"}) for dt in HALF for M in (1, 17)]


def run_lp_pair(R, e):
    dt, M = e["dtype"], e["M"]
    ops = R.ops
    gates, ups = epi_gates(dt)
    w = torch.cat([_col0(gates, dt), _col0(ups, dt)])
    wp = ops.pack_weight_tiles(R.d(w), gate_up_pairs=True)
    x = R.strided(_epi_x(M, dt, M))
    F = lp_pair_truth(dt, M)
    R.check_set(e["id"], lambda y: ops.linear_packed(x, wp, w.shape[0], out=y, epilogue=lc.LP_SILU_PAIR), F, strided=True, cap=CAP_GENERIC)


LT_QGELU, LT_GELU = 1, 2
LT_ACT_TABLE = [dict(id=f"linear_tiles_act-{DT[dt]}-{s}-{name}", dtype=dt, tile_shape=s, epi=epi, inst={lc.lt_inst(dt, s, 0).replace("BIAS", name)})
                for dt in HALF for s in lc.LT_SHAPES for epi, name in ((LT_QGELU, "QGELU"), (LT_GELU, "GELU"))]


@lru_cache(maxsize=None)
def lt_act_truth(dt, epi, M):
    a = epi_gates(dt)[0][None, :].expand(M, -1)
    return rt.quick_gelu_truth(a) if epi == LT_QGELU else rt.gelu_truth(a)


@lru_cache(maxsize=None)
def lp_pair_truth(dt, M):
    gates, ups = epi_gates(dt)
    return _pair_truth(dt, gates, ups, torch.ones(M, 1, dtype=torch.float64), torch.zeros(M, 1, dtype=torch.float64))


def run_lt_act(R, e):
    dt, shape, epi = e["dtype"], e["tile_shape"], e["epi"]
    ops = R.ops
    gates, _ = epi_gates(dt)
    M = 32
    w = _col0(gates, dt)
    wp = ops.pack_weight_tiles(R.d(w))
    x = R.strided(_epi_x(M, dt, 5))
    F = lt_act_truth(dt, epi, M)
    # (GELU: no cap -- an absolute error against a result that vanishes in the negative tail leaves most of the tail undecided; the share is recorded)
    R.check_set(e["id"], lambda y: ops.linear_tiles(x, wp, w.shape[0], out=y, epilogue=epi, tile_shape=shape), F, strided=True, cap=CAP_GENERIC if epi == LT_QGELU else None)


TABLES = {
    "rmsnorm": (RMS_TABLE, run_rms),
    "add_rmsnorm_parts": (RMS_PARTS_TABLE, run_rms_parts),
    "rmsnorm_packed": (PACKED_TABLE, run_rms_packed),
    "layernorm": (LN_TABLE, run_ln),
    "layernorm_rows": (LN_WAVE_TABLE, run_ln_wave),
    "compact_tokens": (COMPACT_TABLE, run_compact),
    "build_x": (BUILD_X_TABLE, run_build_x),
    "build_x_pk": (BUILD_X_PK_TABLE, lambda R, e: run_build_x(R, e, pk=True)),
    "activations": (ACT_TABLE, run_act),
    "gemv_pair": (GEMV_PAIR_TABLE, run_gemv_pair),
    "gemv_mx8_pair": (GEMV_MX8_PAIR_TABLE, lambda R, e: run_gemv_pair(R, e, mx8=True)),
    "linear_packed_pair": (LP_PAIR_TABLE, run_lp_pair),
    "linear_tiles_act": (LT_ACT_TABLE, run_lt_act),
}


def driven():
    """Every instantiation name this table drives (the linear family's names among them: what leaves linear_cases.omitted())."""
    return set().union(*(e["inst"] for table, _ in TABLES.values() for e in table))


# what this table does not launch: (what, why)
OMITTED = [
    ("dl_gemv_pk on the identity at K = 512, 4104, 8200, 12296", "gemv_pk_ok: the ADDNORM prologue of the packed GEMV is built for K % 1024 == 0, K <= 8192 only; K = 1024 and 4096 are driven instead"),
    ("dl_gemv_pk with GEMV_SILUMUL", "not built: dl_gemv_pk takes PLAIN, ADDNORM and ADDNORM | OUT_SILU_PAIR"),
    ("dl_gemv_mx8 on the identity at K = 4104, 8200, 12296", "MXFP8 rows are blocks of 32: K % 32 != 0 is refused; K = 512 is driven"),
    ("gemv_build_x inside dl_gemv_qkv_attn / dl_gemv_gu_tp", "the same function, but these launches need a KV cache / the text predictor around them; held by their own bit-equality tests against dl_gemv"),
    ("dl_gemm_mx8 activation epilogue", "there is none: dl_gemm_mx8 stores or writes partial sums"),
]


# ------------------------------------------------------------------------------------------------------------------------------
# generic rows of the whole table, for measuring RHO_GENERIC (tests/test_rowwise_truth_cpu.py)
# ------------------------------------------------------------------------------------------------------------------------------
def generic_rows_of_the_table():
    """Yields (family, tag, rows [R, H] model dtype) for every generic statistic the table asks a kernel for."""
    for dt in ALL:
        for H in H_BLOCK[dt]:
            yield "rms", f"{DT[dt]} H{H}", rows("rms", "generic", H, dt).to(dt)
            yield "rms", f"{DT[dt]} H{H} add", add_case("rms", "generic", H, dt)[2]
            yield "rms", f"{DT[dt]} H{H} parts", parts_case("rms", "generic", H, dt, 3)[3]
            if H >= 8:
                yield "ln", f"{DT[dt]} H{H}", rows("ln", "generic", H, dt).to(dt)
                yield "ln", f"{DT[dt]} H{H} add", add_case("ln", "generic", H, dt)[2]
        for K in GEMV_K:
            yield "rms", f"{DT[dt]} K{K} gemv", add_case("rms", "generic", K, dt, 8, seed=8)[2]
    for dt in HALF:
        for H in H_WAVE:
            yield "ln", f"{DT[dt]} H{H} wave", rows("ln", "generic", H, dt).to(dt)
            yield "ln", f"{DT[dt]} H{H} wave parts", parts_case("ln", "generic", H, dt, 3, None, 0, True)[3]


# ------------------------------------------------------------------------------------------------------------------------------
# the table without a GPU
# ------------------------------------------------------------------------------------------------------------------------------
class ReferenceOps(lc.ReferenceOps):
    """oracle/ref_cpu.py's expressions behind hip_ops' argument lists (fp32 statistics by torch, the header's rounding points)."""
    HipOpsError = ValueError

    def gemv_max_batch(self, K, dt):
        return self.real.gemv_max_batch(K, dt)

    @staticmethod
    def _limit(H, dt):
        if H % rt.VEC[dt] or H > 256 * 8 * rt.VEC[dt]:
            raise ValueError(f"unsupported H={H}")

    @staticmethod
    def _ln(x, w, b, eps):
        xf = x.float()
        mean = xf.mean(-1, keepdim=True)
        d = xf - mean
        return (d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps) * w.float() + b.float()).to(x.dtype)

    def _store(self, y, out, packed, tiles):
        if packed:
            out[: tiles * 16 * y.shape[1]].copy_(pack_lp(y, tiles))
        else:
            out.copy_(y)
        return out

    def rmsnorm(self, x, w, eps, out=None, packed=False):
        self._limit(x.shape[-1], x.dtype)
        if packed and x.shape[0] > 256:
            raise ValueError("rows <= 256")
        return self._store(orc.rmsnorm(x, w, eps), out, packed, lp_tiles(x.shape[0]))

    def add_rmsnorm(self, h, delta, w, eps, out=None, packed=False):
        self._limit(h.shape[-1], h.dtype)
        if packed and h.shape[0] > 256:
            raise ValueError("rows <= 256")
        h.copy_((h.float() + delta.float()).to(h.dtype))
        return None if w is None else self._store(orc.rmsnorm(h, w, eps), out, packed, lp_tiles(h.shape[0]))

    @staticmethod
    def _sum_parts(parts, extra=None):
        acc = torch.zeros(parts.shape[1:], dtype=F32)
        for s in range(parts.shape[0]):
            acc = acc + parts[s]
        return acc if extra is None else acc + extra.float()

    def add_rmsnorm_parts(self, h, parts, w=None, eps=1e-6, out=None, packed=False):
        self._limit(h.shape[-1], h.dtype)
        if packed and h.shape[0] > 256:
            raise ValueError("rows <= 256")
        h.copy_((h.float() + self._sum_parts(parts).to(h.dtype).float()).to(h.dtype))
        return None if w is None else self._store(orc.rmsnorm(h, w, eps), out, packed, lp_tiles(h.shape[0]))

    def layernorm(self, x, w, b, eps=1e-5, row_index=None, rows=None, out=None):
        self._limit(x.shape[-1], x.dtype)
        return out.copy_(self._ln(x if row_index is None else x[row_index.long()], w, b, eps))

    def add_layernorm(self, h, delta, w=None, b=None, eps=1e-5, out=None):
        self._limit(h.shape[-1], h.dtype)
        h.copy_((h.float() + delta.float()).to(h.dtype))
        return None if w is None else out.copy_(self._ln(h, w, b, eps))

    @staticmethod
    def _wave_limit(H):
        if H % 8 or vpl(H) not in (1, 2, 3, 4, 8):
            raise ValueError(f"H={H} is not built")

    def layernorm_rows(self, x, w, b, eps=1e-5, out=None, packed=False):
        self._wave_limit(x.shape[-1])
        return self._store(self._ln(x, w, b, eps), out, packed, tiles_rows(x.shape[0]))

    def add_layernorm_rows(self, h, delta, w=None, b=None, eps=1e-5, out=None, packed=False):
        self._wave_limit(h.shape[-1])
        h.copy_((h.float() + delta.float()).to(h.dtype))
        return None if w is None else self._store(self._ln(h, w, b, eps), out, packed, tiles_rows(h.shape[0]))

    def add_layernorm_parts(self, h, parts, bias=None, w=None, b=None, eps=1e-5, out=None, packed=False):
        self._wave_limit(h.shape[-1])
        h.copy_((h.float() + self._sum_parts(parts, bias).to(h.dtype).float()).to(h.dtype))
        return None if w is None else self._store(self._ln(h, w, b, eps), out, packed, tiles_rows(h.shape[0]))

    def compact_tokens(self, h_in, keep_idx, cu_in, cu_out, img_start, n_img, k, total_out, norm_w=None, eps=0.0):
        s = int(img_start[0])
        sel = list(range(s)) + [s + int(i) for i in keep_idx[0]] + list(range(s + n_img, int(cu_in[1])))
        h = h_in[sel]
        return h, torch.tensor(sel, dtype=torch.int32), orc.rmsnorm(h, norm_w, eps)

    def silu_mul(self, gate_up, out=None):
        return out.copy_(self._silu_pair(gate_up, gate_up.dtype))

    def silu_mul_parts(self, parts, out):
        return out.copy_(self._silu_pair(self._sum_parts(parts).to(out.dtype), out.dtype))

    def quick_gelu(self, x, out=None):
        return out.copy_(rt.emulate_quick_gelu(x))

    def pack_bf16(self, w):
        return w

    def gemv_pk(self, p, y, **kw):
        return self.gemv(p, y, **kw)

    @staticmethod
    def _mm(x, w, k0=0, k1=None):
        """x @ w^T in fp64, the weight rows in blocks (the identity at K = 12296 is 1.2 GB in fp64)."""
        xs = x[:, k0:k1].double()
        return torch.cat([xs @ w[n : n + 2048, k0:k1].double().T for n in range(0, w.shape[0], 2048)], 1)

    def gemv(self, w, y, x=None, mode=0, h_in=None, h_out=None, delta=None, norm_w=None, eps=0.0, grid_cap=0):
        dt = y.dtype
        if mode & 3 == ADDNORM:
            hn = h_in if delta is None else (h_in.float() + delta.float()).to(dt)
            if delta is not None:
                h_out.copy_(hn)
            x = orc.rmsnorm(hn, norm_w, eps)
        elif mode & 3 == SILUMUL:
            x = self._silu_pair(x, dt)
        t = self._mm(x, w).float().to(dt)
        y.copy_(self._silu_pair(t, dt) if mode & PAIR else t)

    def linear_tiles(self, x, wp, N, bias=None, out=None, epilogue=0, **kw):
        if epilogue not in (LT_QGELU, LT_GELU):
            return super().linear_tiles(x, wp, N, bias=bias, out=out, epilogue=epilogue, **kw)
        a = self._mm(x, wp).float().to(x.dtype)
        af = a.float()
        return out.copy_(rt.emulate_quick_gelu(a) if epilogue == LT_QGELU else (0.5 * af * (1.0 + torch.erf(af * 0.70710678118654752440))).to(x.dtype))


# ------------------------------------------------------------------------------------------------------------------------------
# the same branches read out of csrc/: a new vectors-per-lane case, NS form or a moved threshold fails the CPU test until the table follows
# ------------------------------------------------------------------------------------------------------------------------------
def branches_in_sources(csrc):
    def read(name):
        with open(os.path.join(csrc, name)) as f:
            return f.read()

    src = read("elementwise.hip")
    out = dict(
        ln_wave_cases=sorted(int(v) for v in re.findall(r"^\s*LN_WAVE_CASE\((\d+)\);", src, flags=re.M)),
        ns_forms=sorted(int(n) for n in re.findall(r"if \(v_ <= 2 && n_slices == (\d+)\) LN_WAVE_GO\(v_, \1\)", src)),
        ns_max_vpl=sorted({int(v) for v in re.findall(r"if \(v_ <= (\d+) && n_slices == \d+\)", src)}),
        max_vec_per_thread=int(re.search(r"constexpr int kMaxVecPerThread = (\d+);", src).group(1)),
        threads=int(re.search(r"constexpr int kThreads = (\d+);", src).group(1)),
        parts_batch=int(re.search(r"constexpr int kPartsBatch = (\d+);", src).group(1)),
    )
    pro = read("gemv_prologue.h")
    out["maxc"] = int(re.search(r"constexpr int MAXC = (\d+);", pro).group(1))
    out["gemv_threads"] = int(re.search(r"constexpr int kGemvThreads = (\d+);", pro).group(1))
    assert "if (nvec <= kGemvThreads * MAXC) {" in pro
    return out
