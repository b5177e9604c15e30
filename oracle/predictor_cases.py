"""The tables behind tests/test_predictor_exact_gpu.py and the code that drives them: the text predictor (three launches, and as extra workgroups of
dl_gemv_gu_tp / dl_gemv_gu_tp_pk), the vision predictor stage by stage out of its workspace, and dl_decode_advance.  Expectations: oracle/predictor_truth.py.
The runner stands on oracle/linear_cases.Runner: every buffer a launch writes lies in a guard band, every launch runs twice and must return the same bits.

The launches go through an adaptor, so that the same tables run without a GPU on the documented arithmetic (EmuAdaptor: predictor_truth.emulate_*, in a
summation order of no kernel, optionally with one mutated step) -- tests/test_predictor_truth_cpu.py dry-runs every runner that way and shows each mutant
outside its set.  branches_in_sources() reads the thresholds the shapes were chosen for out of csrc/; coverage() names the entry that reaches each branch."""
from __future__ import annotations

import math
import os
import re
from functools import lru_cache

import torch
import torch.nn.functional as Fn

from oracle import linear_cases as lc
from oracle import predictor_truth as pt
from oracle import rowwise_truth as rt

BF16, F16, F32 = rt.BF16, rt.F16, rt.F32
DT = lc.DT
ALL = (BF16, F16, F32)
HALF = (BF16, F16)
EPS = pt.EPS
GAIN = 50.0  # the last predictor layer of the "trained-like" initialiser (oracle/fixtures.make_state_dict, predictor_gain)
U_T = {BF16: 2.0**-9, F16: 2.0**-12, F32: 2.0**-24}
TP_KEYS = ("ln_w", "ln_b", "l1_w", "l1_b", "l3_w", "l3_b", "l5_w", "l5_b", "l7_w", "l7_b")
VP_KEYS = ("ln_w", "ln_b", "down_w", "down_b", "out0_w", "out0_b", "out2_w", "out2_b", "out4_w", "out4_b")
BLK_KEYS = ("norm1_w", "norm1_b", "qkv_w", "proj_w", "proj_b", "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


# ------------------------------------------------------------------------------------------------------------------------------
# adaptors
# ------------------------------------------------------------------------------------------------------------------------------
class HipAdaptor:
    device = "cuda"

    def __init__(self, ops):
        self.ops, self.HipOpsError = ops, ops.HipOpsError

    def _tpw(self, W):
        w = self.ops.TpWeights()
        for k in TP_KEYS:
            setattr(w, k, W[k].data_ptr())
        return w

    def tp(self, x, W, D, ws, lg, dec):
        self.ops.text_predictor_decide(x, self._tpw(W), D, ws, lg, dec)

    def gu_tp_workspace(self, D):
        return self.ops.gemv_gu_tp_workspace(D, self.device)

    def gu_tp(self, wgu, y, h_in, h_out, delta, nw, W, D, ws, lg, dec, pos, gran, tag, err, packed):
        if packed:
            from dynamic_llava_amd import bf16pack as bp

            self.ops.gemv_gu_tp_pk(bp.pack(wgu, force=True), y, h_in, h_out, delta, nw, EPS, self._tpw(W), D, ws, lg, dec, pos, gran, tag, err=err)
        else:
            self.ops.gemv_gu_tp(wgu, y, h_in, h_out, delta, nw, EPS, self._tpw(W), D, ws, lg, dec, pos, gran, tag, err=err)

    def vp_workspace_bytes(self, B, n, H, D, FF, dt):
        return int(self.ops.lib().dl_vision_predictor_workspace_bytes(B, n, H, D, FF, self.ops.dtype_code(dt)))

    def vp(self, hidden, cu, st, n, W, D, nhead, FF, ws, layers):
        w = self.ops.VpWeights()
        for k in VP_KEYS:
            setattr(w, k, W[k].data_ptr())
        w.num_layers = layers
        for j in range(layers):
            for k in BLK_KEYS:
                setattr(w.blocks[j], k, W["blocks"][j][k].data_ptr())
        return self.ops.vision_predictor(hidden, cu, st, n, w, D, nhead, FF, workspace=ws)

    def advance(self, logits, nxt, out_ids, step, fin, eos, pad, kf, ks, dec, mnt):
        self.ops.decode_advance(logits, nxt, out_ids, step, fin, list(eos) if eos[0] >= 0 else -1, pad, kf, ks, dec, mnt)


class EmuAdaptor:
    """The documented arithmetic on the CPU behind the same calls; `mutant` alters one step (predictor_truth.*_MUTANTS)."""
    device = "cpu"

    class HipOpsError(RuntimeError):
        pass

    def __init__(self, order=1, mutant=None):
        self.order, self.mutant = order, mutant

    def tp(self, x, W, D, ws, lg, dec):
        B, H = x.shape
        dt = x.dtype
        V = rt.VEC[dt]
        if not (H % V == 0 and x.stride(0) % V == 0 and H <= H_MAX and D % 32 == 0):
            raise self.HipOpsError("refused")
        buf = x.as_strided((B, x.stride(0)), (x.stride(0), 1), x.storage_offset())
        o = pt.emulate_tp(buf, None, W, self.order, self.mutant if self.mutant in pt.TP_MUTANTS else None)
        ws[: B * D].view(B, D).copy_(o["h1"])
        ws[B * D : B * D + B * (D // 2)].view(B, D // 2).copy_(o["a1"])
        if lg is not None:
            lg.copy_(o["logits"])
        dec.copy_(o["decision"])

    def gu_tp_workspace(self, D):
        return torch.zeros(D + D // 2, dtype=torch.int64)

    def gu_tp(self, wgu, y, h_in, h_out, delta, nw, W, D, ws, lg, dec, pos, gran, tag, err, packed):
        self.tp(h_in, W, D, ws, lg, dec)
        hn = (h_in.float() + delta.float()).to(h_in.dtype)
        h_out.copy_(hn)
        x = nw * (hn.float() * torch.rsqrt(hn.float().pow(2).mean(-1, keepdim=True) + EPS)).to(hn.dtype)
        t = (x.float() @ wgu.float().T).to(hn.dtype)
        I = t.shape[1] // 2
        y.copy_((Fn.silu(t[:, :I].float()).to(hn.dtype).float() * t[:, I:].float()).to(hn.dtype))

    def vp_workspace_bytes(self, B, n, H, D, FF, dt):
        return pt.vp_layout(B, n, H, D, FF, dt)["total"]

    def vp(self, hidden, cu, st, n, W, D, nhead, FF, ws, layers):
        dt = hidden.dtype
        B, H = cu.numel() - 1, hidden.shape[1]
        M = B * n
        m = self.mutant
        L = pt.vp_layout(B, n, H, D, FF, dt)
        es = 4 if dt == F32 else 2
        put = lambda name, t: ws[L[name] : L[name] + t.numel() * t.element_size()].view(t.dtype).copy_(t.reshape(-1))
        ri, ci = pt.build_index(cu, st, B, n, m if m in pt.INDEX_MUTANTS else None)
        put("row_index", ri)
        put("cu_img", ci)
        x0 = rt.emulate_layernorm(hidden[ri.long()], W["ln_w"], W["ln_b"], EPS, None, self.order)
        put("x0", x0)
        hs = pt.emulate_dense(x0.float(), W["down_w"], W["down_b"], dt, True, self.order).to(dt)
        if layers:
            hs = block_chain(hs.view(B, n, D), W["blocks"][:layers], nhead)[-1].reshape(M, D)
        put("hs", hs)
        z = pt.emulate_pool(hs.view(B, n, D), self.order, m if m in pt.POOL_MUTANTS else None).reshape(M, D)
        put("z", z)
        z1 = pt.emulate_dense(z.float(), W["out0_w"], W["out0_b"], dt, True, self.order).to(dt)
        put("z1", z1)
        z2 = pt.emulate_dense(z1.float(), W["out2_w"], W["out2_b"], dt, True, self.order).to(dt)
        put("z2", z2)
        lg, sc = pt.emulate_head(z2, W["out4_w"], W["out4_b"], self.order, m if m in pt.HEAD_MUTANTS else None)
        return lg.view(B, n, 2), sc.view(B, n)

    def advance(self, logits, nxt, out_ids, step, fin, eos, pad, kf, ks, dec, mnt):
        VE = rt.VEC[logits.dtype]
        vec_ok = logits.stride(0) % VE == 0 and logits.data_ptr() % 16 == 0
        o = pt.emulate_advance(logits, step, fin, out_ids, eos, pad, kf, ks, dec, mnt, vec_ok, self.mutant if self.mutant in pt.ADVANCE_MUTANTS else None)
        for t, k in ((nxt, "next_ids"), (out_ids, "out_ids"), (step, "step"), (fin, "finished"), (kf, "kv_full"), (ks, "kv_sparse")):
            t.copy_(o[k])
        if int(o["spare"]) != -7:  # the emulated write past the last row: lands in the guard band behind out_ids
            out_ids.as_strided((1,), (1,), out_ids.storage_offset() + out_ids.numel()).copy_(o["spare"])


def block_chain(h, blks, nhead):
    """The transformer blocks of the vision predictor (oracle/ref_cpu.vision_predictor's loop) in h's dtype; -> [h after block 1, after block 2, ..]."""
    B, n, D = h.shape
    outs = []
    for k in blks:
        y = Fn.layer_norm(h, (D,), k["norm1_w"], k["norm1_b"], 1e-5)
        qkv = Fn.linear(y, k["qkv_w"]).reshape(B, n, 3, nhead, D // nhead).permute(2, 0, 3, 1, 4)
        a = Fn.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], dropout_p=0.0).transpose(1, 2).reshape(B, n, D)
        h = h + Fn.linear(a, k["proj_w"], k["proj_b"])
        y = Fn.layer_norm(h, (D,), k["norm2_w"], k["norm2_b"], 1e-5)
        h = h + Fn.linear(Fn.gelu(Fn.linear(y, k["fc1_w"], k["fc1_b"])), k["fc2_w"], k["fc2_b"])
        outs.append(h)
    return outs


# ------------------------------------------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


class Runner(lc.Runner):
    def __init__(self, adaptor):
        super().__init__(adaptor, adaptor.device)
        self.undecided, self.ratios = {}, {}

    def fail(self, tag, **kw):
        self.bad.append(dict(tag=tag, **kw))

    def stage(self, tag, out, F, decided=False):
        """out (CPU) must lie in F; decided: the reference alone must leave no element undecided (asserted first)."""
        self.n += 1
        und = F.undecided()
        self.undecided[tag] = und
        if decided and (und != 0.0 or (F.lo is None and float(F.e.max()) != 0.0)):  # fp32: the interval must have width 0
            self.fail(f"{tag}: undecided share {und} of a lattice stage is not 0")
        ok = F.ok(out)
        if not bool(ok.all()):
            pick = lambda t: None if t is None else t[~ok][:4].double().tolist()
            self.fail(tag, outside=int((~ok).sum()), of=ok.numel(), first=torch.nonzero(~ok)[:4].tolist(), got=out.detach().cpu()[~ok][:4].double().tolist(), lo=pick(F.lo),
                      hi=pick(F.hi), v=pick(F.v), e=pick(F.e))

    def equal(self, tag, a, b):
        """The same bits (NaN payloads included)."""
        self.n += 1
        a, b = _bits(a), _bits(b)
        if a.shape != b.shape or not bool((a == b).all()):
            ne = (a != b) if a.shape == b.shape else None
            self.fail(tag, differing=None if ne is None else int(ne.sum()), of=a.numel(), first=None if ne is None else torch.nonzero(ne)[:4].tolist())

    def truth(self, tag, cond, **kw):
        self.n += 1
        if not cond:
            self.fail(tag, **kw)

    def ints(self, t, tag, fill=-77):
        """A device copy of the integer tensor t inside a band of `fill`."""
        n = t.numel()
        buf = torch.full((n + 128,), fill, dtype=t.dtype, device=self.dev)
        buf[64 : 64 + n] = t.reshape(-1).to(self.dev)
        self.bands.append((tag, buf, 64, 64 + n, fill))
        return buf[64 : 64 + n].view(t.shape)

    def floats(self, shape, dtype, tag):
        buf, view = self.flat(shape, dtype)
        self.bands.append((tag, buf, 64, 64 + view.numel(), None))
        return view

    def refused(self, tag, fn):
        self.n += 1
        try:
            fn()
        except self.ops.HipOpsError:
            return
        self.fail(f"{tag}: not refused")


def _dense(R, tag, *a):
    """pt.dense_truth(*a); when an exact stage is handed an intermediate that has left the lattice, that is recorded and the stage judged by the generic bound."""
    try:
        return pt.dense_truth(*a)
    except pt.PremiseError as e:
        R.fail(f"{tag}: {e} -- the previous stage has left the lattice")
        a = list(a)
        a[5] = False
        return pt.dense_truth(*a)


def _split(F, j):
    pick = lambda t: None if t is None else t[..., j]
    return pt.StageSet(F.dtype, pick(F.lo), pick(F.hi), pick(F.v), pick(F.e), F.between)


def _bounds(F):
    return (F.v - F.e, F.v + F.e) if F.lo is None else (F.lo.double(), F.hi.double())


# ------------------------------------------------------------------------------------------------------------------------------
# text predictor: cases
# ------------------------------------------------------------------------------------------------------------------------------
class TpCase:
    def __init__(self, cls, dtype, x, W, finite, tie=False):
        self.cls, self.dtype, self.x, self.W, self.finite, self.tie = cls, dtype, x, W, finite, tie
        self.D = W["l1_w"].shape[0]


def _generic_weights(H, D, dt, seed):
    g = torch.Generator().manual_seed(4000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    W = dict(ln_w=1 + 0.1 * rn(H), ln_b=0.05 * rn(H))
    for name, n, k in (("l1", D, H), ("l3", D // 2, D), ("l5", D // 4, D // 2), ("l7", 2, D // 4)):
        W[name + "_w"] = rn(n, k) * ((GAIN if name == "l7" else 1.0) / math.sqrt(k))
        W[name + "_b"] = 0.05 * rn(n)
    return {k: v.to(dt) for k, v in W.items()}


@lru_cache(maxsize=None)
def tp_case(cls, H, D, B, dt, tie=False, seed=0):
    V = rt.VEC[dt]
    if cls == "lattice":
        hot = pt.stage1_priority(H, V)
        ln_w, ln_b = pt.lattice_ln(H, dt, seed, hot)
        x = pt.lattice_rows(H, B, dt, seed, hot)
        xs = pt.lattice_ln_out(x, ln_w, ln_b)
        l1_w, l1_b, h1 = pt.lattice_layer(xs, D, dt, seed + 1, 4, hot, limit=64)
        l3_w, l3_b, a1 = pt.lattice_layer(h1, D // 2, dt, seed + 2, 3, limit=128)
        l5_w, l5_b, a2 = pt.lattice_layer(a1, D // 4, dt, seed + 3, 2)
        for s in range(64):
            l7_w, l7_b, lg = pt.lattice_layer(a2, 2, dt, seed + 10 + s, 2, dead_every=0, gelu=False)
            if tie:  # equal rows and equal biases: the two logits are the same number for every input
                l7_w[1], l7_b[1] = l7_w[0], l7_b[0]
                break
            gap = lg[:, 0] - lg[:, 1]
            if bool((gap != 0).all()) and (B < 3 or dt == F32 or (bool((gap > 0).any()) and bool((gap < 0).any()))) and (B > 1 or (gap[0] > 0) == (seed % 2 == 0) or s > 32):
                break
        else:
            raise AssertionError("no l7 with gaps of both signs")
        W = dict(ln_w=ln_w, ln_b=ln_b, l1_w=l1_w, l1_b=l1_b, l3_w=l3_w, l3_b=l3_b, l5_w=l5_w, l5_b=l5_b, l7_w=l7_w, l7_b=l7_b)
        return TpCase(cls, dt, x, W, torch.ones(B, dtype=torch.bool), tie)
    W = _generic_weights(H, D, dt, seed)
    kinds = ("randn", "outlier", "offset")
    cand = torch.cat([rt.generic_rows(H, dt, kinds, 31 * seed + s) for s in range(-(-(4 * B + 9) // 3))]).to(dt)
    emu = pt.emulate_tp(cand, None, W)
    F5 = pt.dense_truth(emu["a1"].double(), W["l5_w"], W["l5_b"], dt)
    F7 = pt.dense_truth(None, W["l7_w"], W["l7_b"], dt, False, False, *_bounds(F5))
    lo, hi = _bounds(F7)
    tol = (hi - lo).max(-1).values + 2.0**-126
    gap = (emu["logits"][:, 0] - emu["logits"][:, 1]).double()
    strong = gap.abs() >= 16 * tol
    pos, neg = [int(i) for i in torch.nonzero(strong & (gap > 0))[:, 0]], [int(i) for i in torch.nonzero(strong & (gap < 0))[:, 0]]
    n_fin = B - 1 if B >= 3 else B
    need = -(-B // 2)
    picked = []
    for i in range(need):  # alternating sign
        src = pos if i % 2 == 0 else neg
        assert src, "no candidate row with a logit gap of 16 x the tolerance and the wanted sign"
        picked.append(src.pop(0))
    rest = [i for i in range(cand.shape[0]) if i not in picked]
    picked += rest[: n_fin - len(picked)]
    x = cand[picked[:n_fin]]
    finite = torch.ones(B, dtype=torch.bool)
    if B >= 3:  # one non-finite row: every logit is NaN, the decision must be 0
        bad = cand[rest[-1]].clone()
        bad[H // 2] = float("inf")
        x = torch.cat([x, bad[None]])
        finite[-1] = False
    return TpCase(cls, dt, x.contiguous(), W, finite)


def tp_launch(R, c, pad, tag, logits_null=False):
    """-> the outputs on the CPU: h1, a1 (the workspace), logits, decision."""
    B, H = c.x.shape
    D = c.D
    xbuf = torch.full((B, H + pad), float("nan"), dtype=c.dtype, device=R.dev)
    xbuf[:, :H] = c.x.to(R.dev)
    W = {k: R.d(v) for k, v in c.W.items()}
    ws = R.workspace(B * (D + D // 2), f"{tag} workspace")
    lg = R.floats((B, 2), F32, f"{tag} logits")
    dec = R.ints(torch.full((B,), -5, dtype=torch.int32), f"{tag} decision")
    R.ops.tp(xbuf[:, :H], W, D, ws, None if logits_null else lg, dec)
    return dict(h1=ws[: B * D].view(B, D).cpu(), a1=ws[B * D :].view(B, D // 2).cpu(), logits=lg.cpu(), decision=dec.cpu())


def tp_judge(R, tag, c, o):
    dt, W, fin = c.dtype, c.W, c.finite
    exact = c.cls == "lattice"
    F1 = pt.stage1_truth(c.x[fin], W["ln_w"], W["ln_b"], W["l1_w"], W["l1_b"], c.cls, exact)
    R.stage(f"{tag} stage 1", o["h1"][fin], F1, decided=exact)
    F3 = _dense(R, f"{tag} stage 2a", o["h1"][fin].double(), W["l3_w"], W["l3_b"], dt, True, exact)
    R.stage(f"{tag} stage 2a", o["a1"][fin], F3, decided=exact)
    F5 = _dense(R, f"{tag} stage 2b", o["a1"][fin].double(), W["l5_w"], W["l5_b"], dt, True, exact)  # a2 stays in LDS: its set feeds the last layer as an interval
    exact = exact and float((_bounds(F5)[1] - _bounds(F5)[0]).max()) == 0.0
    F7 = pt.dense_truth(None, W["l7_w"], W["l7_b"], dt, False, exact, *_bounds(F5))
    R.stage(f"{tag} stage 2b logits", o["logits"][fin], F7, decided=exact)
    lg, dec = o["logits"], o["decision"]
    R.equal(f"{tag} decision == (logit0 > logit1) on the kernel's logits", dec, (lg[:, 0] > lg[:, 1]).int())
    R.truth(f"{tag} a non-finite row decides 0", bool((dec[~fin] == 0).all()))
    det, want = pt.decision_truth(_split(F7, 0), _split(F7, 1))
    B = c.x.shape[0]
    R.truth(f"{tag} determined rows {int(det.sum())} of {B}", int(det.sum()) >= -(-B // 2) if c.cls == "generic" else True)
    R.truth(f"{tag} decision against truth", bool((dec[fin][det] == want[det]).all()), got=dec[fin][det].tolist(), want=want[det].tolist())
    if c.tie:
        R.truth(f"{tag} a planted tie gives equal logits and decides 0", bool((lg[:, 0] == lg[:, 1]).all()) and bool((dec == 0).all()))


# 16-bit: H = 8 (one vector), 520 (a ragged pass of the 64 lanes and of the 256 threads), 5120 = 64 * kTp1MaxChunks vectors (the last H whose weight rows are
# prefetched), 5128 (the first past it: the streaming loop), 12288 (the largest; 12296 is refused).  D: 32 / 96 / 128 one pass of stage 2b, 256 two, 384 three
# (an odd count with PB = 2), 1024 eight (the most the prefetch takes), 1056 (K5 / V = 66 > 64: tp_dense).  fp32: the same in 4-element vectors; D = 512 / 544
# are its K5 / V = 64 / 68.  Large H goes with small D and the reverse; the row stride is H or H + 16.
TP_SHAPES = {
    "16": [(8, 1024, 3, 0), (8, 1056, 1, 16), (520, 384, 32, 16), (520, 256, 3, 0), (5120, 128, 3, 16), (5128, 96, 3, 0), (5128, 32, 32, 16), (12288, 32, 1, 0), (12288, 96, 3, 16)],
    "32": [(4, 1024, 3, 0), (4, 1056, 1, 16), (260, 512, 3, 16), (260, 544, 32, 0), (260, 256, 1, 16), (2560, 384, 3, 0), (2560, 128, 32, 16), (2564, 96, 3, 16), (2564, 32, 1, 0)],
}
H_MAX, H_REFUSED = 12288, {BF16: 12296, F16: 12296, F32: 12292}
TP_TABLE = [dict(id=f"tp-{DT[dt]}-H{H}-D{D}-B{B}-pad{pad}", dtype=dt, H=H, D=D, B=B, pad=pad) for dt in ALL for (H, D, B, pad) in TP_SHAPES["32" if dt == F32 else "16"]] + \
           [dict(id=f"tp-f32-H{H_MAX}-D32-B1-pad0", dtype=F32, H=H_MAX, D=32, B=1, pad=0)]


def run_tp(R, e):
    dt, H, D, B, pad = e["dtype"], e["H"], e["D"], e["B"], e["pad"]
    for cls, tie in (("lattice", False), ("lattice", True), ("generic", False)):
        c = tp_case(cls, H, D, B, dt, tie)
        tag = f"{e['id']} {cls}{' tie' if tie else ''}"
        o = [tp_launch(R, c, pad, tag) for _ in range(2)]
        for k in o[0]:
            R.equal(f"{tag} second launch {k}", o[0][k], o[1][k])
        tp_judge(R, tag, c, o[0])
        if not tie:
            n = tp_launch(R, c, pad, f"{tag} logits_out NULL", logits_null=True)
            R.equal(f"{tag} logits_out NULL decision", n["decision"], o[0]["decision"])
            R.equal(f"{tag} logits_out NULL h1", n["h1"], o[0]["h1"])
            R.truth(f"{tag} logits_out NULL: nothing written", bool(torch.isnan(n["logits"]).all()))
    if H == H_MAX:
        Hr = H_REFUSED[dt]
        W = {k: R.d(v) for k, v in _generic_weights(Hr, D, dt, 0).items()}  # sized for Hr: a launch that is not refused stays in bounds
        z = torch.zeros(1, Hr, dtype=dt, device=R.dev)
        ws = R.workspace(D + D // 2, f"{e['id']} refused workspace")
        dec = R.ints(torch.full((1,), -5, dtype=torch.int32), f"{e['id']} refused decision")
        R.refused(f"{e['id']} H={Hr}", lambda: R.ops.tp(z, W, D, ws, None, dec))
        R.truth(f"{e['id']} refused: nothing written", bool((dec.cpu() == -5).all()))


# ------------------------------------------------------------------------------------------------------------------------------
# the fused launches: the same stage bodies as extra workgroups of the gate|up projection (MAXC = 8 up to H = 4096, 10 beyond)
# ------------------------------------------------------------------------------------------------------------------------------
GU_TABLE = [dict(id=f"gu_tp{'_pk' if pk else ''}-{DT[dt]}-H{H}-D{D}", dtype=dt, H=H, D=D, packed=pk, maxc=pt.FUSED_MAXC[0] if H // rt.VEC[dt] <= 64 * pt.FUSED_MAXC[0] else pt.FUSED_MAXC[1])
            for dt in ALL for (H, D) in ((1024, 64), (1024, 384), (5120, 64), (5120, 384)) for pk in ((False, True) if dt == BF16 else (False,))]
GU_I = 64


def gu_launch(R, c, tag, packed, call_tag):
    dt = c.dtype
    H, D = c.x.shape[1], c.D
    g = torch.Generator().manual_seed(77)
    wgu = R.d((torch.randn(2 * GU_I, H, generator=g) * 0.02).to(dt))
    nw = R.d((1 + 0.1 * torch.randn(H, generator=g)).to(dt))
    delta = R.d((0.25 * torch.randn(1, H, generator=g)).to(dt))
    W = {k: R.d(v) for k, v in c.W.items()}
    ws = R.workspace(D + D // 2, f"{tag} workspace")
    lg = R.floats((1, 2), F32, f"{tag} logits")
    dec = R.ints(torch.full((1,), -5, dtype=torch.int32), f"{tag} decision")
    y = R.floats((1, GU_I), dt, f"{tag} y")
    h_out = R.floats((1, H), dt, f"{tag} h_out")
    err = R.ints(torch.zeros(1, dtype=torch.int32), f"{tag} err")
    pos = R.d(torch.tensor([50], dtype=torch.int32))
    gran = R.ops.gu_tp_workspace(D)
    R.ops.gu_tp(wgu, y, R.d(c.x), h_out, delta, nw, W, D, ws, lg, dec, pos, gran, call_tag, err, packed)
    R.truth(f"{tag} err flag 0", int(err.cpu()) == 0)
    R.truth(f"{tag} y and h_out written", bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(h_out.float()).all()) if bool(c.finite.all()) else True)
    return dict(h1=ws[:D].view(1, D).cpu(), a1=ws[D:].view(1, D // 2).cpu(), logits=lg.cpu(), decision=dec.cpu())


def run_gu_tp(R, e):
    dt, H, D = e["dtype"], e["H"], e["D"]
    for cls in ("lattice", "generic"):
        c = tp_case(cls, H, D, 1, dt)
        tag = f"{e['id']} {cls}"
        sep = tp_launch(R, c, 0, f"{tag} separate")
        o = [gu_launch(R, c, tag, e["packed"], t) for t in (3, 4)]
        for k in sep:
            R.equal(f"{tag} second launch {k}", o[0][k], o[1][k])
            R.equal(f"{tag} {k} == the separate launches", o[0][k], sep[k])
        tp_judge(R, tag, c, o[0])


# ------------------------------------------------------------------------------------------------------------------------------
# vision predictor
# ------------------------------------------------------------------------------------------------------------------------------
class VpCase:
    pass


def _vp_generic_weights(H, D, FF, dt, layers, seed):
    g = torch.Generator().manual_seed(5000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    gain, bias, mat = (lambda n: 1 + 0.1 * rn(n)), (lambda n: 0.05 * rn(n)), (lambda n, k, s=1.0: rn(n, k) * (s / math.sqrt(k)))
    W = dict(ln_w=gain(H), ln_b=bias(H), down_w=mat(D, H), down_b=bias(D), out0_w=mat(D // 2, D), out0_b=bias(D // 2), out2_w=mat(D // 4, D // 2), out2_b=bias(D // 4),
             out4_w=mat(2, D // 4, GAIN), out4_b=bias(2))
    W["blocks"] = [dict(norm1_w=gain(D), norm1_b=bias(D), qkv_w=mat(3 * D, D), proj_w=mat(D, D), proj_b=bias(D), norm2_w=gain(D), norm2_b=bias(D), fc1_w=mat(FF, D), fc1_b=bias(FF),
                        fc2_w=mat(D, FF), fc2_b=bias(D)) for _ in range(layers)]
    cast = lambda d: {k: (v.to(dt) if torch.is_tensor(v) else [cast(b) for b in v]) for k, v in d.items()}
    return cast(W)


@lru_cache(maxsize=None)
def vp_case(cls, dt, H, D, FF, n, B, layers, seed=0):
    """Packed hidden rows: sequence b holds 2 + 3 b text rows, its n image rows, 5 - b text rows (ragged cu_seqlens, a different img_start per row)."""
    c = VpCase()
    g = torch.Generator().manual_seed(6000 + seed)
    c.cls, c.dtype, c.H, c.D, c.FF, c.n, c.B, c.layers = cls, dt, H, D, FF, n, B, layers
    c.nhead = 2
    W = _vp_generic_weights(H, D, FF, dt, layers, seed)
    pre, post = [2 + 3 * b for b in range(B)], [5 - b for b in range(B)]
    lens = [pre[b] + n + post[b] for b in range(B)]
    c.cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    c.img_start = torch.tensor(pre, dtype=torch.int32)
    M = B * n
    if cls == "lattice":
        V = rt.VEC[dt]
        hot = pt.stage1_priority(H, V)
        W["ln_w"], W["ln_b"] = pt.lattice_ln(H, dt, seed, hot)
        img = pt.lattice_rows(H, M, dt, seed, hot)
        xs = pt.lattice_ln_out(img, W["ln_w"], W["ln_b"])
        W["down_w"], W["down_b"], c.hs_exact = pt.lattice_layer(xs, D, dt, seed + 1, 4, hot, limit=28)  # 2049 x 28 < 65504: the fp16 total stays finite
    else:
        img = torch.cat([rt.generic_rows(H, dt, ("randn", "outlier", "offset", "randn3"), 17 * seed + s) for s in range(-(-M // 4))])[:M].to(dt)
    hidden = torch.randn(int(c.cu[-1]), H, generator=g).to(dt)
    rows, _ = pt.build_index(c.cu, c.img_start, B, n)
    hidden[rows.long()] = img
    c.hidden, c.W, c.rows = hidden, W, rows
    return c


def vp_launch(R, c, layers, tag):
    dt, B, n, H, D, FF = c.dtype, c.B, c.n, c.H, c.D, c.FF
    L = pt.vp_layout(B, n, H, D, FF, dt)
    R.truth(f"{tag} vp_layout total == dl_vision_predictor_workspace_bytes", L["total"] == R.ops.vp_workspace_bytes(B, n, H, D, FF, dt))
    ws = R.workspace_bytes(L["total"], f"{tag} workspace")
    dev = lambda d: {k: (R.d(v) if torch.is_tensor(v) else [dev(b) for b in v]) for k, v in d.items()}
    hidden, cu, st, W = R.d(c.hidden), R.d(c.cu), R.d(c.img_start), dev(c.W)  # (alive until the copies below have synchronised)
    lg, sc = R.ops.vp(hidden, cu, st, n, W, D, c.nhead, FF, ws, layers)
    M = B * n
    es = 4 if dt == F32 else 2
    get = lambda name, cols, t=dt: ws[L[name] : L[name] + M * cols * (es if t == dt else 4)].cpu().view(t).view(M, cols)
    return dict(row_index=get("row_index", 1, torch.int32).view(-1), cu_img=ws[L["cu_img"] : L["cu_img"] + (B + 1) * 4].cpu().view(torch.int32), x0=get("x0", H), hs=get("hs", D),
                z=get("z", D), z1=get("z1", D // 2), z2=get("z2", D // 4), logits=lg.cpu().view(M, 2), score=sc.cpu().view(M))


def vp_judge(R, tag, c, o, layers):
    dt, W, B, n, D = c.dtype, c.W, c.B, c.n, c.D
    lattice = c.cls == "lattice"
    ri, ci = pt.build_index(c.cu, c.img_start, B, n)
    R.equal(f"{tag} row_index", o["row_index"], ri)
    R.equal(f"{tag} cu_img", o["cu_img"], ci)
    Fx = rt.ln_truth(c.hidden[ri.long()], W["ln_w"], W["ln_b"], EPS, rt.RHO_LATTICE if lattice else rt.RHO_GENERIC, exact_mean=lattice)
    R.stage(f"{tag} x0", o["x0"], Fx, decided=lattice and dt != F32)
    if layers == 0:
        R.stage(f"{tag} down", o["hs"], _dense(R, f"{tag} down", o["x0"].double(), W["down_w"], W["down_b"], dt, True, lattice), decided=lattice)
    hs = o["hs"].view(B, n, D)
    ints = bool((hs.double() == hs.double().round()).all()) and float(hs.double().abs().sum(1).max()) < 2**24
    R.truth(f"{tag} lattice hs are integers", ints or not lattice)
    R.stage(f"{tag} pool_concat", o["z"].view(B, n, D), pt.pool_truth(hs, exact=lattice and ints), decided=lattice and ints and dt != F32)
    R.stage(f"{tag} out0", o["z1"], pt.dense_truth(o["z"].double(), W["out0_w"], W["out0_b"], dt))
    R.stage(f"{tag} out2", o["z2"], pt.dense_truth(o["z1"].double(), W["out2_w"], W["out2_b"], dt))
    R.stage(f"{tag} head logits", o["logits"], pt.dense_truth(o["z2"].double(), W["out4_w"], W["out4_b"], dt, False))
    R.stage(f"{tag} score", o["score"], pt.score_truth(o["logits"]))


def blocks_check(R, tag, c, hs0, hs_l, layers):
    """hs after `layers` blocks against the fp64 chain started from the kernel's own hs0; the tolerance comes from the same-dtype eager chain's error."""
    dt, B, n, D = c.dtype, c.B, c.n, c.D
    h0 = hs0.view(B, n, D)
    b64 = [{k: v.double() for k, v in b.items()} for b in c.W["blocks"][:layers]]
    truth = block_chain(h0.double(), b64, c.nhead)[-1]
    eager = block_chain(h0, c.W["blocks"][:layers], c.nhead)[-1].double()
    tol = 4 * (eager - truth).abs().amax(-1, keepdim=True) + 2 * U_T[dt] * truth.abs()
    err = (hs_l.view(B, n, D).double() - truth).abs()
    ratio = float((err / tol).max())
    R.ratios[tag] = dict(ratio=ratio, eager_row_max=float((eager - truth).abs().amax(-1).max()), kernel_max=float(err.max()))
    R.truth(f"{tag}: |hs - fp64 chain| <= 4 x the eager chain's row maximum + 2 U |truth| (largest ratio {ratio:.3f})", ratio <= 1.0)


VP_SHAPES = [(128, 36, 3, 2), (256, 257, 3, 2), (128, 577, 3, 1), (256, 577, 1, 0), (128, 257, 1, 1)]
VP_TABLE = [dict(id=f"vp-{DT[dt]}-D{D}-n{n}-B{B}-L{L}", dtype=dt, D=D, n=n, B=B, layers=L) for dt in ALL for (D, n, B, L) in VP_SHAPES] + \
           [dict(id="vp-f16-D128-n2049-B1-L0", dtype=F16, D=128, n=2049, B=1, layers=0)]
VP_H = VP_FF = 256


def run_vp(R, e):
    dt, D, n, B, layers = e["dtype"], e["D"], e["n"], e["B"], e["layers"]
    cl = vp_case("lattice", dt, VP_H, D, VP_FF, n, B, 0)
    o = vp_launch(R, cl, 0, f"{e['id']} lattice")
    vp_judge(R, f"{e['id']} lattice", cl, o, 0)
    c = vp_case("generic", dt, VP_H, D, VP_FF, n, B, layers)
    runs = {}
    for L in range(layers + 1):
        tag = f"{e['id']} generic layers {L}"
        o = [vp_launch(R, c, L, tag) for _ in range(2 if L in (0, layers) else 1)]
        if len(o) == 2:
            for k in o[0]:
                R.equal(f"{tag} second launch {k}", o[0][k], o[1][k])
        vp_judge(R, tag, c, o[0], L)
        runs[L] = o[0]
        if L:
            blocks_check(R, f"{e['id']} blocks 1..{L}", c, runs[0]["hs"], o[0]["hs"], L)


# ------------------------------------------------------------------------------------------------------------------------------
# dl_decode_advance
# ------------------------------------------------------------------------------------------------------------------------------
ADV_V = {"16": (1, 7, 8, 9, 32768, 32771, 32776, 65541), "32": (1, 3, 4, 5, 16384, 16387, 16388, 32773)}
ADV_TABLE = [dict(id=f"advance-{DT[dt]}-V{V}", dtype=dt, V=V) for dt in ALL for V in ADV_V["32" if dt == F32 else "16"]]
OUT_CAP = 4
ADV_MIN_NEW = 2  # min_new_tokens of the launches with an EOS set


def adv_positions(V, VE):
    """Index 0, the last index, the start of the tail, and both sides of every vector, wave, thread-block and loop-trip boundary below V."""
    out = [0, V - 1, (V // VE) * VE]
    for b in (VE, 64 * VE, 1024 * VE, 2048 * VE, pt.TRIP_CHUNKS * VE, pt.TRIP_CHUNKS * VE + 1024 * VE):
        out += [b - 1, b]
    return sorted({p for p in out if 0 <= p < V})


@lru_cache(maxsize=None)
def adv_case(dt, V, seed=0):
    """-> dict: logits [B, V] and the per-row state.  Rows: one per planted maximum; tie pairs across every boundary (and first / last index); the EOS rows (the
    banned id holds the maximum, a runner-up elsewhere); NaN rows; a -inf row."""
    VE = rt.VEC[dt]
    g = torch.Generator().manual_seed(7000 + seed + V)
    P = adv_positions(V, VE)
    rows, meta = [], []

    def base():
        return torch.randn(V, generator=g).clamp(-6, 6)

    for p in P:
        r = base()
        r[p] = 50.0
        rows.append(r)
    for a, b in [(p - 1, p) for p in P if p - 1 in P] + [(0, V - 1)]:
        if a != b:
            r = base()
            r[a] = r[b] = 50.0
            rows.append(r)
    n_plain = len(rows)
    eos = tuple(P[-1 - i] if i < len(P) else -1 for i in range(3))  # the EOS set: the last planted positions
    eos_rows = {}  # row -> (its step, the EOS id that holds its maximum): one copy banned (step 0), one not (step = min_new_tokens)
    for i, e in enumerate(eos):
        if e < 0:
            continue
        r = base()
        r[e] = 60.0  # the banned id holds the maximum
        runner = P[i % len(P)] if P[i % len(P)] != e else (e + 1) % V
        if runner != e:
            r[runner] = 40.0  # (it may itself be banned: then the background decides)
        for st in (0, ADV_MIN_NEW):
            eos_rows[len(rows)] = (st, e)
            rows.append(r.clone())
    r = base()
    r[V // 2] = float("nan")
    r[0] = 30.0
    rows.append(r)
    rows.append(torch.full((V,), float("nan")))
    rows.append(torch.full((V,), float("-inf")))
    r = base()
    r[V - 1] = float("inf")
    rows.append(r)
    logits = torch.stack(rows).to(dt)
    B = logits.shape[0]
    ar = torch.arange(B)
    step = torch.tensor([0, 1, OUT_CAP - 1, OUT_CAP, 2], dtype=torch.int32)[ar % 5]
    fin = ((ar % 7) == 6).int()
    for row, (st, _) in eos_rows.items():
        step[row], fin[row] = st, 0
    for n_eos in (1, 2, 3):  # every id of every EOS set is, on some unfinished row, the banned argmax -- and the unbanned one
        for e in eos[:n_eos]:
            if e >= 0:
                for st in (0, ADV_MIN_NEW):
                    assert any(s_ == st and e_ == e and int(logits[row_].float().argmax()) == e for row_, (s_, e_) in eos_rows.items()), (V, n_eos, e, st)
    return dict(logits=logits, step=step, finished=fin, kv_full=(10 + ar).int(), kv_sparse=(5 + ar).int(), decision=(ar % 2).int(), eos=eos, n_plain=n_plain)


ADV_LAYOUTS = ("aligned", "offset_by_one", "odd_stride")
ADV_EOS = (0, 1, 2, 3)  # number of EOS ids in the set


def adv_launch(R, c, layout, n_eos, mnt, tag):
    dt = c["logits"].dtype
    VE = rt.VEC[dt]
    B, V = c["logits"].shape
    stride = -(-V // VE) * VE + (VE if layout != "odd_stride" else 1)
    off = 1 if layout == "offset_by_one" else 0
    raw = torch.full((B * stride + VE + off,), float("nan"), dtype=dt, device=R.dev)
    view = raw[off : off + B * stride].view(B, stride)[:, :V]
    view.copy_(c["logits"].to(R.dev))
    eos = tuple(c["eos"][:n_eos]) + (-1,) * (3 - n_eos) if n_eos else (-1, -1, -1)
    st = dict(step=R.ints(c["step"], f"{tag} step"), finished=R.ints(c["finished"], f"{tag} finished"), kv_full=R.ints(c["kv_full"], f"{tag} kv_full"),
              kv_sparse=R.ints(c["kv_sparse"], f"{tag} kv_sparse"), out_ids=R.ints(torch.full((B, OUT_CAP), -3, dtype=torch.int64), f"{tag} out_ids"),
              next_ids=R.ints(torch.full((B,), -9, dtype=torch.int64), f"{tag} next_ids"))
    dec = R.d(c["decision"])
    R.ops.advance(view, st["next_ids"], st["out_ids"], st["step"], st["finished"], eos, 0 if n_eos != 2 else 7, st["kv_full"], st["kv_sparse"], dec, mnt)
    want = pt.advance_ref(c["logits"], c["step"], c["finished"], torch.full((B, OUT_CAP), -3, dtype=torch.int64), eos, 0 if n_eos != 2 else 7, c["kv_full"], c["kv_sparse"], c["decision"], mnt)
    return {k: v.cpu() for k, v in st.items()}, want


def run_advance(R, e):
    dt, V = e["dtype"], e["V"]
    c = adv_case(dt, V)
    for layout in ADV_LAYOUTS:
        for n_eos in ADV_EOS:
            mnt = ADV_MIN_NEW if n_eos else 0
            tag = f"{e['id']} {layout} eos {n_eos}"
            (a, want), (b, _) = adv_launch(R, c, layout, n_eos, mnt, tag), adv_launch(R, c, layout, n_eos, mnt, tag)
            for k in a:
                R.equal(f"{tag} {k}", a[k], want[k])
                R.equal(f"{tag} second launch {k}", a[k], b[k])


TABLES = {"text_predictor": (TP_TABLE, run_tp), "gemv_gu_tp": (GU_TABLE, run_gu_tp), "vision_predictor": (VP_TABLE, run_vp), "decode_advance": (ADV_TABLE, run_advance)}


# ------------------------------------------------------------------------------------------------------------------------------
# the branches, read out of the sources
# ------------------------------------------------------------------------------------------------------------------------------
def branches_in_sources(csrc):
    """The thresholds the shapes above were chosen for, parsed out of csrc/tp_body.h, predictors.hip, advance.hip and gemv.hip; AssertionError when one is no longer
    written as restated here."""
    read = lambda name: open(os.path.join(csrc, name)).read()
    tp, pr, adv, gv = read("tp_body.h"), read("predictors.hip"), read("advance.hip"), read("gemv.hip")
    out = dict(max_chunks=int(re.search(r"constexpr int kTp1MaxChunks = (\d+);", tp).group(1)), pb=int(re.search(r"constexpr int PB = (\d+);", tp).group(1)))
    assert "const bool pre = nvec <= 64 * MAXC;" in tp
    m = re.search(r"const bool pre = K5 % V == 0 && K5 / V <= (\d+) && passes <= (\d+);", tp)
    out["k5_vecs"], out["max_passes"] = int(m.group(1)), int(m.group(2))
    assert "const int passes = (N5 + nw * 4 - 1) / (nw * 4);" in tp and "dim3(512), (size_t)(D / 2 + D / 4 + 2) * sizeof(float)" in pr  # 8 waves: 32 neurons a pass
    m = re.search(r"for \(int c0 = 0; c0 < n_chunks; c0 \+= (\d+) \* (\d+)\)", adv)
    out["trip_chunks"] = int(m.group(1)) * int(m.group(2))
    assert "(row_stride % VE == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0)" in adv
    out["h_max"] = int(re.search(r"DL_REQUIRE\(H <= (\d+), \"dl_text_predictor_decide", pr).group(1))
    m = re.search(r"if \(a\.K / Elem<T>::kVec <= 64 \* (\d+)\) hipLaunchKernelGGL\(\(gemv_gu_tp_kernel<T, (\d+), PK>\).*\n\s*else hipLaunchKernelGGL\(\(gemv_gu_tp_kernel<T, (\d+), PK>\)", gv)
    assert m and m.group(1) == m.group(2)
    out["fused_maxc"] = (int(m.group(2)), int(m.group(3)))
    assert "const float denom = Elem<T>::round((float)n);" in pr
    return out


def coverage(br):
    """branch -> the ids of the table entries that reach it (an empty list fails the CPU test)."""
    cov = {}
    add = lambda k, e: cov.setdefault(k, []).append(e["id"])
    for k in ("stage1 prefetch", "stage1 last prefetched H", "stage1 streaming, first H past the prefetch", "stage1 H_max", "2b prefetch", "2b tp_dense: K5 / V past the limit",
              "2b odd pass count > 1", "2b K5 / V at the limit", "row stride != H"):
        for t in ("16-bit", "fp32"):
            cov[f"{k} ({t})"] = []
    for e in TP_TABLE:
        V = rt.VEC[e["dtype"]]
        t = "fp32" if e["dtype"] == F32 else "16-bit"
        nvec, lim = e["H"] // V, 64 * br["max_chunks"]
        if nvec <= lim:
            add(f"stage1 prefetch ({t})", e)
        if nvec == lim:
            add(f"stage1 last prefetched H ({t})", e)
        if nvec == lim + 1:
            add(f"stage1 streaming, first H past the prefetch ({t})", e)
        if e["H"] == br["h_max"]:
            add(f"stage1 H_max ({t})", e)
        K5, N5 = e["D"] // 2, e["D"] // 4
        passes = -(-N5 // 32)
        pre = K5 % V == 0 and K5 // V <= br["k5_vecs"] and passes <= br["max_passes"]
        add(f"2b {'prefetch' if pre else 'tp_dense: K5 / V past the limit'} ({t})", e)
        if pre and passes % br["pb"] and passes > 1:
            add(f"2b odd pass count > 1 ({t})", e)
        if pre and K5 // V == br["k5_vecs"]:
            add(f"2b K5 / V at the limit ({t})", e)
        if e["pad"]:
            add(f"row stride != H ({t})", e)
    for mc in br["fused_maxc"]:
        cov[f"fused MAXC {mc}"] = [e["id"] for e in GU_TABLE if e["maxc"] == mc]
    cov["fused packed"] = [e["id"] for e in GU_TABLE if e["packed"]]
    for dt in ALL:
        VE, t = rt.VEC[dt], DT[dt]
        es = [e for e in ADV_TABLE if e["dtype"] == dt]
        cov[f"advance {t} V < one vector"] = [e["id"] for e in es if e["V"] < VE]
        cov[f"advance {t} tail"] = [e["id"] for e in es if e["V"] % VE and e["V"] > VE]
        cov[f"advance {t} one full trip"] = [e["id"] for e in es if e["V"] == br["trip_chunks"] * VE]
        cov[f"advance {t} second trip"] = [e["id"] for e in es if e["V"] // VE > br["trip_chunks"]]
        cov[f"advance {t} second trip and tail"] = [e["id"] for e in es if e["V"] // VE > br["trip_chunks"] and e["V"] % VE]
    for dt, ns in ((BF16, (257, 577)), (F16, (2049,))):
        for n in ns:
            assert float(torch.tensor(float(n)).to(dt)) != float(n)
            cov[f"pool_concat {DT[dt]} n = {n} is rounded"] = [e["id"] for e in VP_TABLE if e["dtype"] == dt and e["n"] == n]
    for L in (0, 1, 2):
        cov[f"vision num_layers {L}"] = [e["id"] for e in VP_TABLE if e["layers"] >= L]
    return cov
