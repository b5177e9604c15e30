"""GPU: MXFP8 decoder weights in decode batches of 4..32 rows -- dl_gemm_mx8 (exhaustive dequantisation through the matrix cores, fp64 truth on W' at the decoder
shapes, its partial sums through the existing consumers, argument checks) and the model with set_decode_weight_format("mxfp8", max_batch=32) against the
format-off model on W', against its own B = 1 runs, under hipGraph replay and after a weight edit.

Every model test asserts from model._dstate that the step took the dl_gemm_mx8 route: none can pass by running the model-dtype kernels."""
import math
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fixtures as fx  # noqa: E402

from dynamic_llava_amd import hip_ops as ops  # noqa: E402
from dynamic_llava_amd.mxfp8 import dequantize_mx8, e_min, gemm_mx8_slices, quantize_mx8  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
ULP = {torch.float16: 2.0**-10, torch.bfloat16: 2.0**-7}
_PROJ = re.compile(r"model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")
# (N, K) of q|k|v, o, gate|up and down at 7B and 13B (tests/test_mxfp8_gpu.py's SHAPES), and small shapes whose N is not a multiple of 16
SHAPES = {
    "7b": [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)],
    "13b": [(15360, 5120), (5120, 5120), (27648, 5120), (5120, 13824)],
    "small": [(132, 256), (200, 512), (132, 768), (64, 512)],
}


def _build(cfg_ns, sd, clip, dtype, fmt=None, max_batch=None):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig

    m = build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg_ns), sd, clip.state_dict() if clip is not None else None, dtype=dtype, device="cuda")
    if fmt is not None:
        m.set_decode_weight_format(fmt, max_batch=max_batch)
    return m


def _sd_prime(sd, dtype):
    """the state dict with every decoder projection weight replaced by its MXFP8 value W' (the pure-torch host reference, run on the device for speed:
    independent of dl_quantize_mx8), in `dtype`"""
    out = {}
    for k, v in sd.items():
        if _PROJ.match(k):
            w = v.to(dtype).cuda()
            q, s = quantize_mx8(w, dtype)
            out[k] = dequantize_mx8(q, s, dtype).cpu()
        else:
            out[k] = v.to(dtype) if v.is_floating_point() else v
    return out


def _took_mx8_gemm(model, B):
    st = model._dstate
    return st is not None and st.B == B and st.use_mx8_gemm and not st.use_gemv and not st.use_lp_mlp and st.o_parts is None


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1. exhaustive dequantisation through the matrix cores
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_exhaustive_dequantisation(dtype):
    """All 256 codes x every block exponent in [e_min, e_max] of the dtype (the dtype's subnormals included), one-hot x rows: y == q * 2^e bit for bit, through
    PLAIN (one slice: the kernel's own store; three slices: the reduce) and through the PARTS partial sums added in fp32.  K = 768 (three 256-code chunks, row r
    holds every code three times); the hot k walks over every position of a chunk -- all four lane groups of a fragment, both halves of a 16-byte load, every
    block of a chunk -- and over the three chunks."""
    e_lo = e_min(dtype)
    e_hi = 7 if dtype == torch.float16 else 119  # floor(log2(max finite)) - 8
    exps = torch.arange(e_lo, e_hi + 1)
    n = exps.numel()
    n_pad = (n + 3) // 4 * 4  # N % 4 == 0: the last rows repeat the last exponent
    exps = torch.cat([exps, exps[-1:].repeat(n_pad - n)])
    codes = torch.arange(256, dtype=torch.int32)
    codes[0x7F] = 0
    codes[0xFF] = 0
    K = 768
    q = codes.to(torch.uint8)[None].repeat(n_pad, 3).contiguous()  # [n_pad, 768]
    s = (exps + 127).to(torch.uint8)[:, None].repeat(1, K // 32).contiguous()
    want = dequantize_mx8(q, s, torch.float32)  # exact in fp32
    assert torch.equal(want.to(dtype).float(), want)  # and in the dtype
    assert bool(((want != 0) & (want.abs() < (2.0**-14 if dtype == torch.float16 else 2.0**-126))).any()), "subnormals of the dtype take part"
    qd, sd_ = q.cuda(), s.cuda()
    ws = torch.empty(3 * 32 * n_pad, dtype=torch.float32, device="cuda")
    for M in (4, 16, 17, 32):
        for k0 in range(0, K, M):  # every k of the row is hot once per M
            ks = [min(k0 + m, K - 1) for m in range(M)]
            x = torch.zeros(M, K, dtype=dtype, device="cuda")
            x[torch.arange(M), torch.tensor(ks)] = 1
            outs = {
                "plain1": ops.gemm_mx8(x, qd, sd_, workspace=ws, n_slices=1),
                "plain3": ops.gemm_mx8(x, qd, sd_, workspace=ws, n_slices=3),
            }
            for ns in (1, 3):
                parts, s_eff = ops.gemm_mx8_parts(x, qd, sd_, ws, n_slices=ns)
                assert s_eff == ns and parts.shape == (ns, M, n_pad)
                outs[f"parts{ns}"] = parts.sum(0).to(dtype)  # (one slice holds the value, the others exact zeros)
            exp = want[:, ks].T.contiguous()
            for name, y in outs.items():
                got = y.float().cpu()
                assert torch.equal(got, exp), (dtype, M, name, k0, int((got != exp).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 2. dl_gemm_mx8 against the fp64 truth on W'
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["small", "7b", "13b"])
def test_gemm_mx8_vs_fp64_truth_on_w_prime(dtype, which):
    """y = cast(fp32 sum of the exact products x * W'): within the PLAIN tolerance of test_gemv_mx8_modes_vs_fp32_reference (one output ulp of |acc| + 1e-5 of
    |x| @ |W'|^T for the fp32 summation), for every M class, forced and automatic split-K, strided X and Y whose NaN padding must stay NaN; a second run gives the
    same bits."""
    g = torch.Generator(device="cuda").manual_seed(3)
    U = ULP[dtype]
    for N, K in SHAPES[which]:
        W = (torch.randn(N, K, generator=g, device="cuda") / K**0.5).to(dtype)
        W[0, :64] *= 1e-6  # tiny blocks (the fp16 e_min clamp)
        W[1, :32] = 0
        q, s = ops.quantize_mx8(W)
        Wp64 = dequantize_mx8(q, s, dtype).double()
        ws = torch.empty(16 * 32 * N, dtype=torch.float32, device="cuda")
        for M in (4, 5, 8, 16, 17, 24, 32):
            xbuf = torch.full((M, K + 24), float("nan"), dtype=dtype, device="cuda")
            xbuf[:, :K] = torch.randn(M, K, generator=g, device="cuda").to(dtype)
            x = xbuf[:, :K]  # row stride K + 24
            acc = x.double() @ Wp64.T
            tol = U * acc.abs() + 1e-5 * (x.double().abs() @ Wp64.abs().T) + 1e-30
            for ns in (1, 2, 3, 0):
                s_eff = int(ops.lib().dl_gemm_mx8_slices(M, N, K, ns))
                assert s_eff == gemm_mx8_slices(M, N, K, ns) >= 1
                if ns:
                    assert s_eff >= min(ns, K // 256), "a forced slice count is only ever raised (the X slice must fit LDS) or cut to K / 256"
                ybuf = torch.full((M, N + 8), float("nan"), dtype=dtype, device="cuda")
                y = ybuf[:, :N]
                ops.gemm_mx8(x, q, s, out=y, workspace=ws, n_slices=ns)
                err = (y.double() - acc).abs()
                assert bool((err <= tol).all()), (which, N, K, M, ns, dtype, float((err - tol).max()))
                assert bool(torch.isnan(ybuf[:, N:]).all()) and bool(torch.isnan(xbuf[:, K:]).all()), "padding untouched"
                y2 = torch.full((M, N + 8), float("nan"), dtype=dtype, device="cuda")
                ops.gemm_mx8(x, q, s, out=y2[:, :N], workspace=ws, n_slices=ns)
                assert torch.equal(y2[:, :N].view(torch.int16), y.view(torch.int16)), "run twice: equal bits"
                # the PARTS form of the same call: its slices added in order and rounded once are the PLAIN result
                parts, sp = ops.gemm_mx8_parts(x, q, s, ws, n_slices=ns)
                assert sp == s_eff
                tot = parts[0].clone()
                for j in range(1, sp):
                    tot += parts[j]
                assert torch.equal(tot.to(dtype).view(torch.int16), y.contiguous().view(torch.int16)), (which, N, K, M, ns)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. the partial sums feed the existing consumers
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,H,I", [(4, 256, 512), (17, 512, 768), (32, 4096, 11008)])
def test_mx8_partials_consumers_bit_equal_reduce_then_op(dtype, M, H, I):
    """dl_gemm_mx8(PARTS) + dl_add_rmsnorm_parts / dl_silu_mul_parts == dl_gemm_mx8(PLAIN, reduced) + dl_add_rmsnorm / dl_silu_mul, bit for bit (the method of
    test_smallm_partials_consumers_bit_equal_reduce_then_op)."""
    g = torch.Generator().manual_seed(61)
    x = torch.randn(M, H, generator=g).to(dtype).cuda()
    act = torch.randn(M, I, generator=g).to(dtype).cuda()
    gu = ops.quantize_mx8((torch.randn(2 * I, H, generator=g) / math.sqrt(H)).to(dtype).cuda())
    dn_w = ops.quantize_mx8((torch.randn(H, I, generator=g) / math.sqrt(I)).to(dtype).cuda())
    h0 = torch.randn(M, H, generator=g).to(dtype).cuda()
    nw = (1 + 0.1 * torch.randn(H, generator=g)).to(dtype).cuda()
    ws = torch.empty(8 * M * 2 * I, dtype=torch.float32, device="cuda")
    ref = ops.silu_mul(ops.gemm_mx8(x, *gu, workspace=ws), out=torch.empty(M, I, dtype=dtype, device="cuda"))
    parts, s = ops.gemm_mx8_parts(x, *gu, ws)
    assert parts.shape == (s, M, 2 * I)
    out = ops.silu_mul_parts(parts, torch.empty(M, I, dtype=dtype, device="cuda"))
    assert torch.equal(out, ref)
    dn = ops.gemm_mx8(act, *dn_w, workspace=ws)
    h_a = h0.clone()
    x_a = ops.add_rmsnorm(h_a, dn, nw, 1e-5)
    parts, s = ops.gemm_mx8_parts(act, *dn_w, ws)
    h_b = h0.clone()
    x_b = ops.add_rmsnorm_parts(h_b, parts, nw, 1e-5)
    assert torch.equal(h_a, h_b) and torch.equal(x_a, x_b)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. bad arguments
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_gemm_mx8_rejects_bad_arguments():
    dt = torch.bfloat16
    N, K = 64, 512
    q, s = ops.quantize_mx8(torch.randn(N, K, device="cuda").to(dt))
    x = torch.randn(32, K, device="cuda").to(dt)
    x32 = x.float()
    y = torch.full((32, N), 7.0, dtype=dt, device="cuda")
    ws = torch.full((2 * 32 * N,), 7.0, dtype=torch.float32, device="cuda")
    lib = ops.lib()
    bf = ops.dtype_code(dt)
    cases = [  # (x, scale, M, K, n_slices, epilogue, dtype code, workspace bytes)
        (x, s, 4, 480, 0, ops.MX8_PLAIN, bf, ws.numel() * 4),  # K % 256
        (x, s, 0, K, 0, ops.MX8_PLAIN, bf, ws.numel() * 4),  # M = 0
        (x, s, 33, K, 0, ops.MX8_PLAIN, bf, ws.numel() * 4),  # M = 33
        (x32, s, 4, K, 0, ops.MX8_PLAIN, ops.dtype_code(torch.float32), ws.numel() * 4),  # fp32
        (x, None, 4, K, 0, ops.MX8_PLAIN, bf, ws.numel() * 4),  # NULL scale
        (x, s, 32, K, 2, ops.MX8_PLAIN, bf, 2 * 32 * N * 4 - 4),  # workspace too small for the two slices
        (x, s, 32, K, 1, ops.MX8_PARTS, bf, 32 * N * 4 - 4),  # PARTS always writes the workspace
        (x, s, 4, K, 0, 2, bf, ws.numel() * 4),  # unknown epilogue
    ]
    for x_, s_, M, K_, ns, ep, dc, wb in cases:
        rc = lib.dl_gemm_mx8(ops._p(x_), x_.stride(0), ops._p(q), ops._p(s_), ops._p(y), N, ops._p(ws), wb, M, N, K_, ns, ep, dc, ops._stream())
        assert rc == -1, (M, K_, ns, ep, dc, wb)
    assert lib.dl_gemm_mx8_slices(4, N, 480, 0) == 0 and lib.dl_gemm_mx8_workspace_bytes(33, N, K, 0) == 0
    with pytest.raises(ops.HipOpsError):
        ops.gemm_mx8(x, q, s, out=y, workspace=ws[: 32 * N], n_slices=2)
    with pytest.raises(ops.HipOpsError):
        ops.gemm_mx8_parts(x, q, s, ws[: 32 * N - 4], n_slices=1)
    torch.cuda.synchronize()
    assert bool((y.float() == 7.0).all()) and bool((ws == 7.0).all()), "a rejected call launched nothing"
    assert ops.gemm_mx8_ok(4, 64, 512, dt) and not ops.gemm_mx8_ok(4, 64, 480, dt) and not ops.gemm_mx8_ok(33, 64, 512, dt) and not ops.gemm_mx8_ok(4, 64, 512, torch.float32)
    assert not ops.gemm_mx8_ok(4, 66, 512, dt)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 5. the model against the format-off model on W'
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _ragged(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    n_q = torch.randint(8, 40, (B,), generator=g).tolist()
    prompts = [fx.make_prompt(cfg, 35, n_q[b], seed=20 + b) for b in range(B)]
    W = max(p.shape[0] for p in prompts)
    ids = torch.zeros(B, W, dtype=torch.long)
    am = torch.zeros(B, W, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]] = p
        am[b, : p.shape[0]] = 1
    return prompts, n_q, ids, am


@pytest.mark.parametrize("width", ["7b", "13b"])
def test_full_width_batched_vs_format_off_model(width):
    """test_full_width_vs_format_off_model's method at B = 4..32 with max_batch = 32: the MXFP8 model's logits are in the format-off model's noise class against
    the fp32 model on the same W', same greedy token unless the truth's top two are inside the two errors, equal KV lengths of the evicting layers.  (Boundary
    decisions are forced BEFORE the step, as _b1_step_following does: a step repeated afterwards would append its token a second time.)"""
    dtype = torch.bfloat16
    cfg = fx.llava7b_config(num_hidden_layers=3) if width == "7b" else fx.llava13b_config(num_hidden_layers=3)
    cfg.vocab_size = 4096
    H = cfg.hidden_size
    sd = fx.make_state_dict(cfg, seed=7, predictor_gain=50.0)
    sdp = _sd_prime(sd, dtype)
    mx = _build(cfg, sd, None, dtype, "mxfp8", max_batch=32)
    assert mx.knobs()["mx8_max_decode_batch"] == 32
    off = _build(cfg, sdp, None, dtype)
    truth = _build(cfg, {k: v.float() for k, v in sdp.items()}, None, torch.float32)  # fp32 model on the same W' values
    g = torch.Generator().manual_seed(21)
    steps = 8
    for B in (4, 7, 16, 32) if width == "7b" else (12, 32):
        feats = torch.randn(B, 576, H, generator=g)
        _, _, ids, am = _ragged(cfg, B, seed=5 + B)
        forced = fx.make_forced_tokens(cfg, steps, B, seed=6)
        models = {"mx": mx, "off": off, "truth": truth}
        state = {}
        n_forced = 0
        with torch.no_grad():
            for k, m in models.items():
                m.debug_records = {}
                out = m(ids.cuda(), attention_mask=am.cuda(), image_features=feats.to(m.dtype).cuda())
                state[k] = out.past_key_values
            for j in range(steps):
                logits = {}
                off_dec = off_tl = None
                for k in ("off", "truth", "mx"):
                    m = models[k]
                    # the format-off model leads; the other two FOLLOW its keep / evict decisions (force_text_decision overrides the bookkeeping only, set before the
                    # step: forward() advances the cache in place, so a step cannot be repeated afterwards), which keeps the caches comparable.  Their own
                    # decisions (debug_records) must agree outside the boundary band
                    m.force_text_decision = None if k == "off" else off_dec.view(-1, 1)
                    out = m(forced[j][:, None].cuda(), past_key_values=state[k])
                    m.force_text_decision = None
                    dec = m.debug_records["text_decision"].cpu().clone().reshape(-1)
                    if k == "off":
                        off_dec, off_tl = dec, m.debug_records["text_logit"].float().cpu()
                    elif not torch.equal(dec.bool(), off_dec.bool()):
                        tl = m.debug_records["text_logit"].float().cpu()
                        for b in range(B):
                            if bool(dec[b]) != bool(off_dec[b]):
                                assert fx.decision_may_differ(tl[b], m.dtype, off_tl[b], dtype), (width, B, j, k)
                        n_forced += 1
                    state[k] = out.past_key_values
                    logits[k] = out.logits[:, -1].float().cpu()
                assert _took_mx8_gemm(mx, B), f"B={B}: the step must run the four projections on dl_gemm_mx8"
                assert not off._dstate.use_mx8_gemm and not truth._dstate.use_mx8_gemm
                e_mx = (logits["mx"] - logits["truth"]).abs().amax(-1)
                e_off = (logits["off"] - logits["truth"]).abs().amax(-1)
                scale = logits["truth"].abs().amax(-1)
                print(f"{width} B={B} step {j}: max e_mx {float(e_mx.max()):.4g} e_off {float(e_off.max()):.4g} max|truth| {float(scale.max()):.4g}")
                assert bool((e_mx <= 2.0 * e_off + 2 * ULP[dtype] * scale).all()), (width, B, j, e_mx.tolist(), e_off.tolist())
                t2 = logits["truth"].topk(2, dim=-1).values
                gap = t2[:, 0] - t2[:, 1]
                same = logits["mx"].argmax(-1) == logits["off"].argmax(-1)
                assert bool((same | (gap <= e_mx + e_off)).all()), (width, B, j)
            lm = [int(x) for x in state["mx"][1][-1].cpu().reshape(-1)]
            lo = [int(x) for x in state["off"][1][-1].cpu().reshape(-1)]
            assert lm == lo, "KV lengths of the evicting layers"
        assert n_forced <= 2 * fx.MAX_FORCED_DECISIONS * B
    # the neighbouring routes are unchanged: 3 rows stream the codes through dl_gemv_mx8, 33 rows run the library GEMMs
    for B in (3, 33):
        feats = torch.randn(B, 576, H, generator=g).to(dtype)
        _, _, ids, am = _ragged(cfg, B, seed=5 + B)
        with torch.no_grad():
            out = mx(ids.cuda(), attention_mask=am.cuda(), image_features=feats.cuda())
            mx(fx.make_forced_tokens(cfg, 1, B, seed=6)[0][:, None].cuda(), past_key_values=out.past_key_values)
        st = mx._dstate
        assert st.B == B and not st.use_mx8_gemm
        assert (st.use_gemv and mx.decode_weight_format == "mxfp8") if B == 3 else (not st.use_gemv and not st.use_smallm)
    assert mx.decode_weight_bytes()["mxfp8"] == 3 * sum(N * K + N * K // 32 for N, K in SHAPES[width]), "no second copy of the codes"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 6. rows of a ragged batch equal their own B = 1 runs
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _b1_step_following(model, tok, pkv, dec_batched, gap_batched, where):
    """One B = 1 decode step whose keep / evict bookkeeping follows the batched run's decision; the step's own decision must agree outside the boundary band
    (tests/test_configs_gpu.py's helper).  Returns (output, True if the B = 1 run's own decision differed and was overridden)."""
    model.force_text_decision = torch.tensor([int(dec_batched)])
    o1 = model(tok, past_key_values=pkv)
    model.force_text_decision = None
    own = int(model.debug_records["text_decision"][0])
    tl = model.debug_records["text_logit"].cpu()
    gap1 = float((tl[0, 0] - tl[0, 1]).abs())
    if own != int(dec_batched):
        band = fx.boundary_band(tl[0], torch.bfloat16)
        assert min(gap1, float(gap_batched)) <= band, f"{where}: eviction decision differs away from the boundary (B=1 gap {gap1}, batched gap {float(gap_batched)}, band {band:.3g})"
        return o1, True
    return o1, False


def test_batched_mx8_rows_equal_their_b1_runs():
    """test_mid_batch_decode_smallm_rows_equal_b1's method with max_batch = 32: every compared row of a ragged batch (dl_gemm_mx8) against the same model's B = 1
    run (dl_gemv_mx8) -- logits within 8 ulp of max|logit|, decisions followed at boundaries, KV lengths."""
    dtype = torch.bfloat16
    cfg = fx.llava7b_config(num_hidden_layers=3)
    cfg.vocab_size = 4096
    sd = fx.make_state_dict(cfg, seed=11, predictor_gain=50.0)
    model = _build(cfg, sd, None, dtype, "mxfp8", max_batch=32)
    ulp = 2.0**-7
    for B in (4, 20, 32):
        prompts, n_q, ids, am = _ragged(cfg, B, seed=5)
        feats = torch.randn(B, 576, cfg.hidden_size, generator=torch.Generator().manual_seed(B)).to(dtype)
        forced = fx.make_forced_tokens(cfg, 8, B, seed=4)
        model.debug_records = {}
        with torch.no_grad():
            ob = model(ids.cuda(), attention_mask=am.cuda(), image_features=feats.cuda())
            pkv = ob.past_key_values
            hist, dec_b, gap_b = [], [], []
            for j in range(8):
                ob = model(forced[j][:, None].cuda(), past_key_values=pkv)
                pkv = ob.past_key_values
                hist.append(ob.logits[:, -1].cpu())
                dec_b.append(model.debug_records["text_decision"].cpu().clone())
                tl = model.debug_records["text_logit"].cpu()
                gap_b.append((tl[:, 0] - tl[:, 1]).abs())
            assert _took_mx8_gemm(model, B), f"B={B} must run on dl_gemm_mx8"
            lens_b = [t.clone() for t in pkv[1]]
            for b in sorted({0, B // 2, B - 1}):
                o1 = model(prompts[b][None].cuda(), image_features=feats[b : b + 1].cuda())
                p1 = o1.past_key_values
                kept, n_forced = 0, 0
                for j in range(8):
                    o1, f_ = _b1_step_following(model, forced[j][b : b + 1][:, None].cuda(), p1, dec_b[j][b], gap_b[j][b], f"B={B} row {b} step {j}")
                    p1 = o1.past_key_values
                    n_forced += f_
                    kept += int(dec_b[j][b])
                    ref = o1.logits[0, -1].cpu()
                    d = float((ref - hist[j][b]).abs().max())
                    print(f"B={B} row {b} step {j}: |diff| {d:.4g}, 8 ulp of max|logit| {8 * ulp * float(ref.abs().max()):.4g}")
                    assert d <= 8 * ulp * float(ref.abs().max()), f"B={B} row {b} step {j}"
                assert model._dstate.B == 1 and model._dstate.use_gemv, "the B = 1 run streams the codes through dl_gemv_mx8"
                assert int(lens_b[-1][b]) == 35 + 115 + n_q[b] + kept and int(lens_b[0][b]) == 35 + 576 + n_q[b] + 8
                assert int(p1[1][-1][0]) == int(lens_b[-1][b])
                assert n_forced <= fx.MAX_FORCED_DECISIONS, f"B={B} row {b}: {n_forced} of 8 decisions had to be followed: more than a boundary effect"
    model.debug_records = None


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 7. hipGraph replay, toggling max_batch, weight edits (bf16: an fp32 model never takes the route)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _tiny(seed=2):
    cfg = fx.tiny_config()  # hidden 256, intermediate 512: widths dl_gemm_mx8 takes
    sd = fx.make_state_dict(cfg, seed=seed, predictor_gain=50.0)
    clip = fx.build_clip(cfg, seed=1)
    return cfg, sd, clip


def _batch(cfg, B, seed=0):
    prompts = [fx.make_prompt(cfg, 2 + (3 * b) % 7, 4 + (5 * b) % 11, seed=seed + b) for b in range(B)]
    n = max(p.shape[0] for p in prompts)
    ids = torch.zeros(B, n, dtype=torch.long)
    am = torch.zeros(B, n, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]] = p
        am[b, : p.shape[0]] = 1
    return ids, am


def _gen(model, ids, am, images, n=10):
    return model.generate(ids.cuda(), attention_mask=am.cuda(), images=images.cuda(), max_new_tokens=n, eos_token_id=None, output_scores=True, return_dict_in_generate=True)


def _same(a, b):
    return torch.equal(a["sequences"], b["sequences"]) and all(torch.equal(x, y) for x, y in zip(a["scores"], b["scores"]))


def test_graph_replay_equals_eager_and_max_batch_toggle():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny()
    B = 8
    mx = _build(cfg, sd, clip, dtype, "mxfp8", max_batch=32)
    ids, am = _batch(cfg, B)
    images = fx.make_images(cfg, B, seed=3).to(dtype)
    outs, toks = {}, {}
    for graph in (True, False):
        mx.use_hip_graph = graph
        outs[graph] = _gen(mx, ids, am, images)
        assert _took_mx8_gemm(mx, B)
        toks[graph] = mx.generate(ids.cuda(), attention_mask=am.cuda(), images=images.cuda(), max_new_tokens=10, eos_token_id=None)  # (keeps its cache, and with it its graphs)
        assert _took_mx8_gemm(mx, B) and (not graph or len(mx._dstate.graphs) >= 1), "graph on: the steps are replayed from a captured graph"
    assert _same(outs[True], outs[False]), "hipGraph replay == eager launches on the dl_gemm_mx8 route"
    assert torch.equal(toks[True], toks[False]) and torch.equal(toks[True], outs[True]["sequences"])
    # toggling max_batch: each setting runs its own route (a graph captured under the other setting is never replayed) and reproduces its own results
    mx.use_hip_graph = True
    on1 = _gen(mx, ids, am, images)
    mx.set_decode_weight_format("mxfp8")
    assert mx._dstate is None and mx.knobs()["mx8_max_decode_batch"] is None
    off1 = _gen(mx, ids, am, images)
    assert mx._dstate.B == B and not mx._dstate.use_mx8_gemm
    mx.use_hip_graph = False
    off_eager = _gen(mx, ids, am, images)
    mx.use_hip_graph = True
    mx.set_decode_weight_format("mxfp8", max_batch=32)
    assert mx._dstate is None
    on2 = _gen(mx, ids, am, images)
    assert _took_mx8_gemm(mx, B)
    assert _same(on1, outs[False]) and _same(on2, outs[False]) and _same(off1, off_eager)
    assert not all(torch.equal(x, y) for x, y in zip(on1["scores"], off1["scores"])), "the two routes round differently somewhere in 10 steps of 8 rows: equal scores would mean one graph served both"
    # max_batch below the batch: the model-dtype route, bit-identical to max_batch = None
    mx.set_decode_weight_format("mxfp8", max_batch=4)
    low = _gen(mx, ids, am, images)
    assert not mx._dstate.use_mx8_gemm and _same(low, off1)
    # an fp32 model never takes the route
    m32 = _build(cfg, sd, clip, torch.float32, "mxfp8", max_batch=32)
    _gen(m32, ids, am, images.float(), n=3)
    assert m32._dstate.B == B and not m32._dstate.use_mx8_gemm
    with pytest.raises(ValueError):
        mx.set_decode_weight_format("mxfp8", max_batch=33)
    with pytest.raises(ValueError):
        mx.set_decode_weight_format("mxfp8", max_batch=2)
    with pytest.raises(ValueError):
        mx.set_decode_weight_format(None, max_batch=8)


def test_weight_changed_after_quantisation_is_requantised_at_b8():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny()
    B = 8
    mx = _build(cfg, sd, clip, dtype, "mxfp8", max_batch=32)
    ids, am = _batch(cfg, B)
    images = fx.make_images(cfg, B, seed=3).to(dtype)
    before = _gen(mx, ids, am, images, n=8)
    assert _took_mx8_gemm(mx, B)
    codes_before = mx.model.layers[1].mx8["down"][0].clone()
    sd2 = dict(sd)
    k = "model.layers.1.mlp.down_proj.weight"
    sd2[k] = sd[k] * 3.0 + 0.01
    with torch.no_grad():
        mx.model.layers[1].mlp.down_proj.weight.copy_(sd2[k].to(dtype).cuda())
    after = _gen(mx, ids, am, images, n=8)
    assert _took_mx8_gemm(mx, B) and mx.knobs()["mx8_max_decode_batch"] == 32
    assert not torch.equal(mx.model.layers[1].mx8["down"][0], codes_before)
    fresh = _build(cfg, sd2, clip, dtype, "mxfp8", max_batch=32)
    want = _gen(fresh, ids, am, images, n=8)
    assert _took_mx8_gemm(fresh, B)
    assert _same(after, want)
    assert not all(torch.equal(a, b) for a, b in zip(after["scores"], before["scores"]))
    q, s = quantize_mx8(sd2[k].to(dtype), dtype)
    assert torch.equal(mx.model.layers[1].mlp.down_proj.weight.cpu(), dequantize_mx8(q, s, dtype))
