"""The table of attention launches that tests/test_attn_routes_gpu.py asserts on and tools/attn_error_table.py reports: every kernel
dl_attn_prefill{,_cached} can dispatch to (by shape, or by the DL_PF_* switch the tuning tools use), the decode kernels over their launch
parameters, and the fused batch-1 launch -- each run on the hard inputs of oracle/attn_truth.py and compared with the fp64 truth under
the per-element bound.  `ops` is dynamic_llava_amd.hip_ops (passed in: the oracle does not import the product).

max_seqlen may OVERSTATE the longest row: model.py sizes the device-layout prefill for a width bucket (prefill.py _width_bucket, 16 rows by
default) while cu_seqlens, written on the device, holds the true widths.  Entries with `over` > 0 are therefore launched a second time with
max_seqlen + over (same route) and must return the same bits."""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass, field

import torch

from oracle import attn_truth as at
from oracle.ref_cpu import rope_table

PF_SWITCHES = ("DL_PF_NW", "DL_PF_PIPE", "DL_PF_WHOLE", "DL_PF_WHOLE_KW", "DL_PF_WHOLE128", "DL_PF_KSPLIT")
# thresholds the library caches on first use: they are crossed by shape below, and must not be set in the environment of a test run
PF_CACHED_THRESHOLDS = ("DL_PF_HEAD64_MIN", "DL_PF_WHOLE128_MIN", "DL_PF_WHOLE128_ZPAIRS")


@dataclass
class Prefill:
    route: str
    nH: int
    nKV: int
    d: int
    causal: bool
    lens: list
    env: dict = field(default_factory=dict)
    over: int = 0          # second launch with max_seqlen + over: same route, same bits
    check: list = None     # requests whose truth is evaluated (default: all)
    dtypes: tuple = (torch.bfloat16, torch.float16)

    @property
    def id(self):
        e = ",".join(f"{k[6:]}={v}" for k, v in self.env.items())
        return f"{self.route}-h{self.nH}kv{self.nKV}d{self.d}-{'causal' if self.causal else 'full'}-max{max(self.lens)}x{len(self.lens)}" + (f"-{e}" if e else "")


F32 = (torch.float32,)
_OFF128 = {"DL_PF_WHOLE128": "0", "DL_PF_KSPLIT": "0"}
_OFF64 = {"DL_PF_WHOLE": "0", "DL_PF_KSPLIT": "0"}
_HEAD64_LENS = [577] * 14 + [300, 608, 257, 590]

# Lengths sit on each route's own domain edges (1, 64/65, 128/129, 192/193, 256/257, 607/608/609 as the route allows); GQA where the
# kernel takes it.  At least one entry per compiled instantiation, the ones only a switch reaches included.
PREFILL_TABLE = [
    Prefill("NONE", 4, 2, 128, True, [0]),
    Prefill("SIMPLE_F32", 4, 2, 64, True, [1, 64, 65, 129, 300], dtypes=F32, over=7),
    Prefill("SIMPLE_F32", 4, 2, 128, False, [257, 1, 128, 33], dtypes=F32),
    Prefill("PLAIN_1W", 4, 2, 128, True, [1, 16, 17, 64, 65, 129, 200], env={"DL_PF_NW": "1", **_OFF128}),
    Prefill("PLAIN_1W", 4, 2, 64, False, [1, 63, 64, 65, 128, 129, 257], env={"DL_PF_NW": "1", **_OFF64}),
    Prefill("PLAIN_2W", 4, 2, 128, False, [1, 64, 65, 128, 129, 192, 193, 256]),
    Prefill("PLAIN_2W", 4, 4, 128, True, [1, 33, 64, 32]),
    Prefill("PLAIN_2W", 4, 2, 64, True, [1, 64, 65, 128, 129, 256]),
    Prefill("PLAIN_2W", 2, 2, 32, True, [37, 150, 5, 240], over=9),
    Prefill("PLAIN_2W", 4, 2, 128, True, [65, 129, 256, 1], env={"DL_PF_WHOLE128": "0"}),  # (key-split refuses > 192 rows: the plain kernel under the whole-head one)
    Prefill("PLAIN_4W", 4, 2, 128, True, [257, 300, 1, 609, 64], env={"DL_PF_PIPE": "0"}),
    Prefill("PLAIN_4W", 2, 2, 32, False, [300, 257, 65]),
    Prefill("PLAIN_4W_K128", 4, 2, 64, True, [257, 577, 608, 609, 1, 128, 129], over=15),
    Prefill("PLAIN_4W_K128", 4, 2, 64, False, [257, 607, 608, 1, 129], env=_OFF64),
    Prefill("PLAIN_4W_K128", 8, 8, 64, False, [609, 700, 64], env={"DL_PF_KSPLIT": "0"}),
    Prefill("PIPE_2W", 4, 2, 64, True, [1, 64, 65, 256, 129], env={"DL_PF_PIPE": "1"}),
    Prefill("PIPE_2W", 4, 2, 128, False, [129, 256, 1, 192, 193], env={"DL_PF_PIPE": "1"}),
    Prefill("PIPE_4W", 4, 2, 128, True, [300, 631, 17, 257, 256, 609], over=11),
    Prefill("PIPE_4W", 4, 2, 64, True, [257, 609, 64], env={"DL_PF_PIPE": "1"}),
    Prefill("PIPE_4W", 2, 1, 128, True, [4096]),
    Prefill("KSPLIT_D128_K2", 4, 2, 128, True, [128, 65, 1, 64, 127], env={"DL_PF_WHOLE128": "0"}),
    Prefill("KSPLIT_D128_K3", 4, 2, 128, True, [192, 129, 1, 65, 191], env={"DL_PF_WHOLE128": "0"}),
    Prefill("KSPLIT_D64", 4, 2, 64, False, [129, 250, 200, 1, 192, 193], over=5),
    Prefill("KSPLIT_D64", 4, 4, 64, False, [256, 130]),
    Prefill("KSPLIT_D64", 4, 2, 64, False, [577, 129, 1, 300, 257], env={"DL_PF_WHOLE": "0"}),
    Prefill("WHOLE_ROW_D64_KW2", 4, 2, 64, False, [257, 577, 608, 1, 300, 607], env={"DL_PF_WHOLE_KW": "2"}),
    Prefill("WHOLE_ROW_D64_KW4", 4, 2, 64, False, [257, 577, 608, 1, 300, 607], over=0),
    Prefill("WHOLE_ROW_D64_KW4", 16, 16, 64, False, [577, 64, 65], over=15),
    Prefill("HEAD_D64", 16, 16, 64, False, _HEAD64_LENS, check=[0, 14, 15, 16, 17]),
    Prefill("HEAD_D64", 32, 8, 64, False, [577, 576, 290, 601, 333, 480, 259, 512], check=[0, 2, 3, 6]),
    Prefill("WHOLE_D128_Z1", 32, 8, 128, True, [200, 64, 129, 96, 31, 241, 2, 160, 256, 65], over=0),
    Prefill("WHOLE_D128_Z2", 4, 2, 128, True, [170, 1, 64, 65, 200, 256, 129, 192, 193], over=0),
    Prefill("WHOLE_D128_Z2", 32, 32, 128, True, [170], over=6),
]


@contextlib.contextmanager
def pf_env(env, setenv=None, delenv=None):
    """The DL_PF_* switches of one table entry (all others unset) -- through monkeypatch's setenv / delenv when given, else os.environ, restored."""
    if setenv is not None:
        for k in PF_SWITCHES:
            delenv(k, raising=False)
        for k, v in env.items():
            setenv(k, v)
        yield
        return
    old = {k: os.environ.get(k) for k in PF_SWITCHES}
    try:
        for k in PF_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _heads(nH):
    return sorted({0, nH // 2, nH - 1})


def prefill_route(ops, e: Prefill, dtype, max_seqlen=None, out_rs=None):
    W = (e.nH + 2 * e.nKV) * e.d
    return ops.attn_prefill_route(len(e.lens), max(e.lens) if max_seqlen is None else max_seqlen, 0, e.nH, e.nKV, e.d, e.causal, False, W, W,
                                  e.nH * e.d + 16 if out_rs is None else out_rs, dtype)


PAD_ROWS, PAD_COLS = 80, 8  # NaN rows behind cu[-1] (inputs and output: more than one key tile), NaN columns on either side of the output slice


def run_prefill(ops, e: Prefill, dist, dtype, seed=0, outputs=None):
    """One table entry on one distribution: q, k, v are views of one fused buffer whose rows behind cu[-1] hold NaN; `out` is a column slice of
    a wider NaN buffer.  Returns (worst err / tol, worst err in ULP of the element, where) after asserting what must hold exactly: nothing
    outside the slice or behind cu[-1] is written, and an overstated max_seqlen changes no bit.  With a list as `outputs`, the launches' output
    tensors are appended to it after those assertions and the truth is not evaluated (tools/attn_error_table.py --digest)."""
    nH, nKV, d = e.nH, e.nKV, e.d
    total = sum(e.lens)
    W = (nH + 2 * nKV) * d
    qkv = torch.full((total + PAD_ROWS, W), float("nan"), dtype=dtype)
    cases, a = [], 0
    for b, L in enumerate(e.lens):
        if L > 0:
            q, k, v = at.make_case(dist, L, L, d, dtype, seed=seed * 131 + b, nH=nH, nKV=nKV)
            qkv[a : a + L] = torch.cat([q.reshape(L, -1), k.reshape(L, -1), v.reshape(L, -1)], 1)
            cases.append((q, k, v))
        else:
            cases.append(None)
        a += L
    cu = torch.tensor([0] + list(torch.tensor(e.lens).cumsum(0)), dtype=torch.int32).cuda()
    dev = qkv.cuda()
    outs = []
    for ms in [max(e.lens)] + ([max(e.lens) + e.over] if e.over else []):
        wide = torch.full((total + PAD_ROWS, nH * d + 2 * PAD_COLS), float("nan"), dtype=dtype, device="cuda")
        out = wide[:, PAD_COLS : PAD_COLS + nH * d]
        ops.attn_prefill(dev[:, : nH * d], dev[:, nH * d : (nH + nKV) * d], dev[:, (nH + nKV) * d :], out, cu, ms, nH, nKV, d, e.causal)
        torch.cuda.synchronize()
        w = wide.cpu()
        assert bool(torch.isnan(w[:, :PAD_COLS]).all()) and bool(torch.isnan(w[:, PAD_COLS + nH * d :]).all()), f"{e.id}: columns outside the output slice were written"
        assert bool(torch.isnan(w[total:]).all()), f"{e.id}: rows behind cu[-1] were written"
        outs.append(w[:total, PAD_COLS : PAD_COLS + nH * d].contiguous())
    if len(outs) == 2:
        assert torch.equal(outs[0].view(torch.int16 if dtype != torch.float32 else torch.int32), outs[1].view(torch.int16 if dtype != torch.float32 else torch.int32)), \
            f"{e.id}: max_seqlen overstated by {e.over} changes the result"
    if outputs is not None:
        outputs.extend(outs)
        return None
    out = outs[0].view(total, nH, d)
    worst = (0.0, 0.0, "")
    hs = _heads(nH)
    a = 0
    for b, L in enumerate(e.lens):
        if L > 0 and (e.check is None or b in e.check):
            q, k, v = cases[b]
            t = at.truth(q, k, v, causal=e.causal, heads=hs if L * nH > 2048 else None)
            r, ulps, i = at.worst_ratio(out[a : a + L][:, t.heads], t, d, dtype)
            if r > worst[0]:
                row, rem = divmod(i, len(t.heads) * d)
                worst = (r, ulps, f"request {b} (len {L}) row {row} head {t.heads[rem // d]} dim {rem % d}")
            worst = (worst[0], max(worst[1], ulps), worst[2])
        a += L
    return worst


# ---- dl_attn_prefill_cached ----
CACHED_KV_LEN = [0, 37, 200, 4000]
CACHED_TABLE = [  # (route, nH, nKV, d, chunk lengths)
    ("PLAIN_2W", 4, 2, 128, [70, 5, 64, 256]),
    ("PIPE_4W", 4, 2, 128, [300, 5, 270, 257]),
    ("PLAIN_2W", 4, 2, 64, [70, 5, 129, 33]),
    ("PLAIN_4W_K128", 4, 2, 64, [300, 5, 270, 257]),
    ("SIMPLE_F32", 4, 2, 128, [70, 5, 64, 257]),
]


def run_cached(ops, entry, dist, dtype, seed=0, outputs=None):
    """`outputs`: as in run_prefill."""
    route, nH, nKV, d, Lq = entry
    B, T_cap = len(Lq), 4400
    k_slab = torch.full((B, nKV, T_cap, d), float("nan"), dtype=dtype)
    v_slab = torch.full((B, nKV, T_cap, d), float("nan"), dtype=dtype)
    total = sum(Lq)
    qbuf = torch.full((total + PAD_ROWS, nH * d + 8), float("nan"), dtype=dtype)  # q: a column slice of a wider buffer
    cases, a = [], 0
    for b, L in enumerate(Lq):
        Lk = CACHED_KV_LEN[b] + L
        q, k, v = at.make_case(dist, L, Lk, d, dtype, seed=seed * 131 + 17 + b, nH=nH, nKV=nKV)
        qbuf[a : a + L, : nH * d] = q.reshape(L, -1)
        k_slab[b, :, :Lk] = k.transpose(0, 1)
        v_slab[b, :, :Lk] = v.transpose(0, 1)
        cases.append((q, k, v))
        a += L
    cu = torch.tensor([0] + list(torch.tensor(Lq).cumsum(0)), dtype=torch.int32).cuda()
    max_kv = max(x + y for x, y in zip(CACHED_KV_LEN, Lq))
    got = ops.attn_prefill_route(B, max(Lq), max_kv, nH, nKV, d, True, True, nH * d + 8, 0, nH * d + 2 * PAD_COLS, dtype)
    assert got == route, (entry, got)
    wide = torch.full((total + PAD_ROWS, nH * d + 2 * PAD_COLS), float("nan"), dtype=dtype, device="cuda")
    out = wide[:, PAD_COLS : PAD_COLS + nH * d]
    ops.attn_prefill_cached(qbuf.cuda()[:, : nH * d], k_slab.cuda(), v_slab.cuda(), torch.tensor(CACHED_KV_LEN, dtype=torch.int32).cuda(), out, cu, max(Lq), max_kv, nH, nKV, d)
    torch.cuda.synchronize()
    w = wide.cpu()
    assert bool(torch.isnan(w[:, :PAD_COLS]).all()) and bool(torch.isnan(w[:, PAD_COLS + nH * d :]).all()) and bool(torch.isnan(w[total:]).all()), "written outside the output"
    if outputs is not None:
        outputs.append(w[:total, PAD_COLS : PAD_COLS + nH * d].contiguous())
        return None
    out = w[:total, PAD_COLS : PAD_COLS + nH * d].reshape(total, nH, d)
    worst = (0.0, 0.0, "")
    a = 0
    for b, L in enumerate(Lq):
        q, k, v = cases[b]
        t = at.truth(q, k, v, causal=True, kv_offset=CACHED_KV_LEN[b], heads=_heads(nH) if k.shape[0] > 1024 else None)
        r, ulps, i = at.worst_ratio(out[a : a + L][:, t.heads], t, d, dtype)
        if r > worst[0]:
            row, rem = divmod(i, len(t.heads) * d)
            worst = (r, ulps, f"request {b} (kv_len {CACHED_KV_LEN[b]}, chunk {L}) row {row} head {t.heads[rem // d]} dim {rem % d}")
        worst = (worst[0], max(worst[1], ulps), worst[2])
        a += L
    return worst


# ---- decode ----
DECODE_KV_LEN = [0, 1, 63, 64, 127, 128, 129, 255, 256, 1023]
DECODE_POS = [5, 1, 700, 64, 127, 300, 129, 255, 2000, 1023]  # RoPE position of the new token: the un-evicted count, not the slot
DECODE_T_CAP = 1100
DECODE_HEADS = [(32, 32, 128), (8, 2, 128), (4, 4, 64), (8, 2, 64)]  # the production shape, GQA at both head dims
# (name, distribution, peak placement as a function of the row's slab length T): the dominant slab key under control
PLACEMENTS = [
    ("first_split", lambda T: (0, T // 2)),
    ("last_slab_key", lambda T: (T - 1, T // 2)),            # kv_len - 1: the last split; next to the splits a short row leaves empty
    ("straddle_64", lambda T: (min(63, T - 1), min(64, T - 1))),
    ("straddle_128", lambda T: (min(127, T - 1), min(128, T - 1))),
    ("straddle_256", lambda T: (min(255, T - 1), min(256, T - 1))),
]
DECODE_DISTS = [(n, n, None) for n in at.DISTRIBUTIONS + at.DECODE_ONLY] + [("late_peak@" + n, "late_peak", f) for n, f in PLACEMENTS]


def decode_launches(kernel):
    """(n_splits, keys_in_flight, chunk_keys, call_tag) of one kernel.  The production pairing of small batches is (1, 128, 256, -1)."""
    if kernel == "decode":
        return [(s, 64, 0, -1) for s in (1, 3, 4, 32)]
    out = []
    for kif in ((64,) if kernel == "parts" else (64, 128, 256)):
        for chunk in (0, 256, 100):
            for s in (1, 3, 4, 32):
                out.append((s, kif, chunk, -1))
                if kif == 64 and chunk == 0 and s > 1:  # where the launch accepts a tag: the splits are merged inside it
                    out.append((s, kif, chunk, 5))
    return out


def build_decode(kernel, dist_entry, dtype, nH, nKV, d, seed=0):
    """Inputs of one decode batch (CPU): qkv [B, (nH + 2 nKV) d] (un-rotated for the fused kernels), slabs with NaN behind kv_len."""
    _, dist, place = dist_entry
    B = len(DECODE_KV_LEN)
    fused = kernel != "decode"
    cos, sin = rope_table(d, 2048, 10000.0, dtype)
    k0 = torch.full((B, nKV, DECODE_T_CAP, d), float("nan"), dtype=dtype)
    v0 = torch.full((B, nKV, DECODE_T_CAP, d), float("nan"), dtype=dtype)
    qkv = torch.empty(B, (nH + 2 * nKV) * d, dtype=dtype)
    for b, T in enumerate(DECODE_KV_LEN):
        peak = place(T) if (place is not None and T > 0) else None
        q, k, v = at.make_case(dist, 1, T + 1, d, dtype, seed=seed * 131 + 41 + b, nH=nH, nKV=nKV, peak_at=peak, rope=(cos, sin, DECODE_POS[b]) if fused else None)
        k0[b, :, :T] = k[:T].transpose(0, 1)
        v0[b, :, :T] = v[:T].transpose(0, 1)
        qkv[b] = torch.cat([q.reshape(-1), k[T].reshape(-1), v[T].reshape(-1)])
    return qkv, k0, v0, cos, sin


def run_decode(ops, kernel, dist_entry, dtype, nH, nKV, d, seed=0, launches=None, outputs=None):
    """Every launch form of `kernel` ("decode": dl_attn_decode, "rope": dl_attn_decode_rope, "parts": dl_attn_decode_rope_parts) on one batch.
    The rotated query and the slab after the append come from dl_rope_kv_write; the fused kernels' slabs must equal them bit for bit.
    Returns {launch: (worst ratio, worst ulps, where)}.  `outputs`: as in run_prefill -- per launch the output slice and, for the fused kernels, the
    K and V rows the launch appended."""
    qkv, k0, v0, cos, sin = build_decode(kernel, dist_entry, dtype, nH, nKV, d, seed)
    B = len(DECODE_KV_LEN)
    lens = torch.tensor(DECODE_KV_LEN, dtype=torch.int32).cuda()
    posd = torch.tensor(DECODE_POS, dtype=torch.int32).cuda()
    cu = torch.arange(0, B + 1, dtype=torch.int32).cuda()
    cosd, sind = cos.cuda(), sin.cuda()
    k0d, v0d, qkvd = k0.cuda(), v0.cuda(), qkv.cuda()
    ka, va, qa = k0d.clone(), v0d.clone(), qkvd.clone()
    if kernel == "decode":  # no RoPE anywhere: the new token's row is appended as it is
        for b, T in enumerate(DECODE_KV_LEN):
            ka[b, :, T] = qa[b, nH * d : (nH + nKV) * d].view(nKV, d)
            va[b, :, T] = qa[b, (nH + nKV) * d :].view(nKV, d)
    else:
        ops.rope_kv_write(qa, cosd, sind, cu, None, posd, lens, ka, va, nH, nKV, d)
    torch.cuda.synchronize()
    q_ref, k_ref, v_ref = qa.cpu()[:, : nH * d].view(B, nH, d), ka.cpu(), va.cpu()
    truths = [] if outputs is not None else [
        at.truth(q_ref[b][None], k_ref[b, :, : T + 1].transpose(0, 1), v_ref[b, :, : T + 1].transpose(0, 1), heads=_heads(nH)) for b, T in enumerate(DECODE_KV_LEN)]
    rows = torch.arange(B, device="cuda")
    ws = ops.attn_decode_workspace(B, nH, d, 32, "cuda")
    res = {}
    for launch in (decode_launches(kernel) if launches is None else launches):
        n_splits, kif, chunk, tag = launch
        out = torch.full((B, nH * d + 2 * PAD_COLS), float("nan"), dtype=dtype, device="cuda")
        o = out[:, PAD_COLS : PAD_COLS + nH * d]
        if tag >= 0:
            ws.zero_()
        if kernel == "decode":
            ops.attn_decode(qa[:, : nH * d], ka, va, lens, 1, o, ws, n_splits, nH, nKV, d)
        else:
            kb, vb, qb = k0d.clone(), v0d.clone(), qkvd.clone()
            if kernel == "rope":
                ops.attn_decode_rope(qb, cosd, sind, posd, lens, kb, vb, o, ws, n_splits, nH, nKV, d, keys_in_flight=kif, chunk_keys=chunk, call_tag=tag)
                assert torch.equal(qb, qkvd), "the fused kernel must not modify qkv"
            else:  # the projection's two k ranges: 0.75 x + 0.25 x is x exactly in fp32
                buf = torch.full((2, B + 3, qkv.shape[1]), float("nan"), device="cuda")
                buf[0, :B], buf[1, :B] = 0.75 * qb.float(), 0.25 * qb.float()
                ops.attn_decode_rope_parts(buf[:, :B], cosd, sind, posd, lens, kb, vb, o, ws, n_splits, nH, nKV, d, chunk_keys=chunk, call_tag=tag)
            torch.cuda.synchronize()
            assert torch.equal(ka.nan_to_num(7.0), kb.nan_to_num(7.0)) and torch.equal(va.nan_to_num(7.0), vb.nan_to_num(7.0)), \
                f"{kernel} {launch}: slab contents after the append differ from dl_rope_kv_write's"
        w = out.cpu()
        assert bool(torch.isnan(w[:, :PAD_COLS]).all()) and bool(torch.isnan(w[:, PAD_COLS + nH * d :]).all()), f"{kernel} {launch}: written outside the output slice"
        got = w[:, PAD_COLS : PAD_COLS + nH * d].reshape(B, nH, d)
        if outputs is not None:
            outputs.append(got.contiguous())
            if kernel != "decode":
                outputs.extend(x[rows, :, lens.long()].cpu().contiguous() for x in (kb, vb))
        worst = (0.0, 0.0, "")
        for b, t in enumerate(truths):
            r, ulps, i = at.worst_ratio(got[b][None][:, t.heads], t, d, dtype)
            if r > worst[0]:
                worst = (r, ulps, f"row {b} (kv_len {DECODE_KV_LEN[b]}) head {t.heads[i // d]} dim {i % d}")
            worst = (worst[0], max(worst[1], ulps), worst[2])
        res[launch] = worst
    return res


# ---- dl_gemv_qkv_attn ----
QKV_ATTN_SHAPES = [(32, 32, 128, 4096), (8, 4, 64, 1024)]
QKV_ATTN_T_OLD = [0, 37, 199, 300, 700]
QKV_ATTN_DISTS = ("sink", "late_peak", "newtok", "newtok_mirror", "v_outlier")


def run_qkv_attn(ops, dist, dtype, nH, nKV, d, H, T_old, seed=0, outputs=None):
    """dl_gemv_qkv_attn with 1..4 attention workgroups per head on a planted slab.  The projection's output is the kernel's own (bit-equal to
    dl_gemv's, asserted); the slab is planted relative to the rotated query it implies; truth = the attention the launch performs.
    Returns {n_splits: (worst ratio, worst ulps, where)}.  `outputs`: as in run_prefill -- of the two launches and of every n_splits the attention
    output and the appended K and V rows; the truth is not evaluated."""
    g = torch.Generator().manual_seed(1000 * seed + T_old)
    rnd = lambda *shape, s=0.02: (torch.randn(*shape, generator=g) * s).to(dtype).cuda()
    N = (nH + 2 * nKV) * d
    W, nw = rnd(N, H), (1 + torch.randn(H, generator=g) * 0.1).to(dtype).cuda()
    T_cap = T_old + 40
    cos, sin = rope_table(d, T_cap + 8, 10000.0, dtype)
    cosd, sind = cos.cuda(), sin.cuda()
    h0, delta = rnd(1, H, s=1.0), rnd(1, H, s=1.0)
    lens = torch.tensor([T_old], dtype=torch.int32, device="cuda")
    pos = torch.tensor([T_old + 3], dtype=torch.int32, device="cuda")
    eps = 1e-5
    qkv_r, ho_r = torch.zeros(1, N, dtype=dtype, device="cuda"), torch.zeros(1, H, dtype=dtype, device="cuda")
    ops.gemv(W, qkv_r, mode=ops.GEMV_ADDNORM, h_in=h0, h_out=ho_r, delta=delta, norm_w=nw, eps=eps)
    # the rotated query, as dl_rope_kv_write computes it (bit-exact against the oracle in tests/test_kernels_gpu.py), on a scratch slab
    qa = qkv_r.clone()
    ks, vs = (torch.zeros(1, nKV, T_cap, d, dtype=dtype, device="cuda") for _ in range(2))
    ops.rope_kv_write(qa, cosd, sind, torch.tensor([0, 1], dtype=torch.int32, device="cuda"), None, pos, lens, ks, vs, nH, nKV, d)
    q_rot = qa.cpu()[0, : nH * d].view(nH, d)
    k, v = at.plant_slab(dist, q_rot, T_old, nKV, d, dtype, seed)
    k0 = torch.full((1, nKV, T_cap, d), float("nan"), dtype=dtype)
    v0 = torch.full((1, nKV, T_cap, d), float("nan"), dtype=dtype)
    k0[0, :, :T_old], v0[0, :, :T_old] = k.transpose(0, 1), v.transpose(0, 1)
    k_r, v_r = k0.cuda(), v0.cuda()
    out_r = torch.zeros(1, nH * d, dtype=dtype, device="cuda")
    ops.attn_decode_rope(qkv_r, cosd, sind, pos, lens, k_r, v_r, out_r, None, 1, nH, nKV, d, chunk_keys=256)
    torch.cuda.synchronize()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    gran = ops.gemv_qkv_attn_workspace(nH, nKV, d, "cuda")
    if outputs is not None:
        outputs.extend(x.cpu().contiguous() for x in (out_r, k_r[0, :, T_old], v_r[0, :, T_old]))
        t, res = None, {}
    else:
        t = at.truth(q_rot[None], k_r.cpu()[0, :, : T_old + 1].transpose(0, 1), v_r.cpu()[0, :, : T_old + 1].transpose(0, 1))
        res = {"two launches": at.worst_ratio(out_r.cpu().view(1, nH, d), t, d, dtype)}
    for ns in (1, 2, 3, 4):
        k_f, v_f = k0.cuda(), v0.cuda()
        qkv_f, ho_f, out_f = torch.zeros_like(qkv_r), torch.zeros_like(ho_r), torch.full((1, nH * d), float("nan"), dtype=dtype, device="cuda")
        ops.gemv_qkv_attn(W, qkv_f, h0, ho_f, delta, nw, eps, cosd, sind, pos, lens, k_f, v_f, out_f, gran, 10 + ns, nH, nKV, d, err=err, n_splits=ns)
        torch.cuda.synchronize()
        assert torch.equal(qkv_f, qkv_r) and torch.equal(ho_f, ho_r), f"n_splits {ns}: projection row / residual stream differ from dl_gemv's"
        assert torch.equal(k_f.nan_to_num(7.0), k_r.nan_to_num(7.0)) and torch.equal(v_f.nan_to_num(7.0), v_r.nan_to_num(7.0)), f"n_splits {ns}: appended K/V row"
        if outputs is not None:
            outputs.extend(x.cpu().contiguous() for x in (out_f, k_f[0, :, T_old], v_f[0, :, T_old]))
            continue
        r, ulps, i = at.worst_ratio(out_f.cpu().view(1, nH, d), t, d, dtype)
        res[ns] = (r, ulps, f"head {i // d} dim {i % d}")
    assert int(err.item()) == 0, "a consumer gave up waiting"
    return res
