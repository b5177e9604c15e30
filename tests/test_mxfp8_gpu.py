"""GPU: MXFP8 decoder weights -- dl_quantize_mx8 against the host reference, dl_gemv_mx8 (exhaustive dequantisation, every mode at the decoder shapes), and the
model in MXFP8 mode against (a) the oracle fed the host-dequantised state dict and (b) the format-off model built from the same W'.

The format has an exact definition: W' = q * 2^e is exact in the model dtype, so "the MXFP8 model" is the model-dtype model with weights W'."""
import copy
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fixtures as fx  # noqa: E402
from oracle.ref_cpu import Oracle  # noqa: E402

from dynamic_llava_amd import hip_ops as ops  # noqa: E402
from dynamic_llava_amd.mxfp8 import dequantize_mx8, e_min, quantize_mx8  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
ULP = {torch.float32: 2.0**-23, torch.float16: 2.0**-10, torch.bfloat16: 2.0**-7}
_PROJ = re.compile(r"model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)\.weight$")
# (N, K, mode) of q|k|v, o, gate|up and down: 7B, 13B, and tiny shapes
SHAPES = {
    "7b": [(12288, 4096, "qkv"), (4096, 4096, "o"), (22016, 4096, "gu"), (4096, 11008, "down")],
    "13b": [(15360, 5120, "qkv"), (5120, 5120, "o"), (27648, 5120, "gu"), (5120, 13824, "down")],
    "tiny": [(64, 64, "qkv"), (96, 32, "o"), (130, 96, "gu"), (72, 160, "down")],
}


def _build(cfg_ns, sd, clip, dtype, fmt=None):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig

    m = build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg_ns), sd, clip.state_dict() if clip is not None else None, dtype=dtype, device="cuda")
    if fmt is not None:
        m.set_decode_weight_format(fmt)
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


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1. the device quantiser
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _edge_rows(dtype):
    """hand-made blocks: zeros, power-of-two amax, RNE midpoints, saturation, e4m3 subnormals, the fp16 e_min clamp, sign of zero"""
    big = 256.0 if dtype != torch.float16 else 2.0**-6
    rows = [
        [0.0] * 32,
        [2.0**-3, -(2.0**-3), 2.0**-4] + [0.0] * 29,
        [256.0, 272.0, 304.0, 280.0, 273.0, -272.0, 1.0625, 1.1875] + [0.0] * 24,
        [500.0, -470.0, 464.0, 448.0, 440.0] + [1.0] * 27,
        [256.0, 2.0**-9, 3 * 2.0**-9, 7 * 2.0**-9, 2.0**-10, 3 * 2.0**-10, -(2.0**-9), 2.0**-6, 15 * 2.0**-10] + [-0.0] * 23,
        [2.0**-10, 2.0**-16, 2.0**-24, 2.0**-20] + [0.0] * 28,
        [big * (i - 16) / 16.0 for i in range(32)],
    ]
    return torch.tensor(rows, dtype=torch.float32).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_kernel_bit_exact_to_host_reference(dtype):
    g = torch.Generator(device="cuda").manual_seed(1)
    cases = [_edge_rows(dtype).cuda()]
    for shapes in (SHAPES["7b"], SHAPES["13b"]):
        for N, K, _ in shapes:
            w = torch.randn(N, K, generator=g, device="cuda") * (0.02 if dtype != torch.float32 else 1e-3)
            w[0, :64] *= 1e-6  # tiny blocks (the fp16 clamp)
            w[1, :32] = 0
            cases.append(w.to(dtype))
    for w in cases:
        for model_dtype in {dtype, torch.bfloat16, torch.float32, torch.float16} if w.shape[0] < 100 else {dtype}:
            qd, sd_ = ops.quantize_mx8(w, model_dtype)
            qh, sh = quantize_mx8(w, model_dtype)  # the host reference (pure torch, here on the device)
            assert torch.equal(qd, qh) and torch.equal(sd_, sh), (tuple(w.shape), dtype, model_dtype)
    # CPU host reference on the edge rows (same rule where it runs)
    qc, sc = quantize_mx8(_edge_rows(dtype))
    qd, sd_ = ops.quantize_mx8(_edge_rows(dtype).cuda())
    assert torch.equal(qc, qd.cpu()) and torch.equal(sc, sd_.cpu())
    bad = torch.randn(4, 64, device="cuda").to(dtype)
    bad[1, 3] = float("nan")
    with pytest.raises(ValueError):
        ops.quantize_mx8(bad)
    with pytest.raises(ops.HipOpsError):
        ops.quantize_mx8(torch.randn(4, 48, device="cuda").to(dtype))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 2. exhaustive dequantisation through dl_gemv_mx8
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_exhaustive_dequantisation(dtype):
    """All 256 codes x every block exponent in [e_min, e_max] of the dtype, one-hot x: y = q * 2^e exactly (the NaN codes 0x7f / 0xff read as 0 here: the
    quantiser never writes them)."""
    e_lo = e_min(dtype)
    e_hi = 7 if dtype == torch.float16 else 119  # floor(log2(max finite)) - 8
    exps = torch.arange(e_lo, e_hi + 1)
    n = exps.numel()
    codes = torch.arange(256, dtype=torch.int32)
    codes[0x7F] = 0
    codes[0xFF] = 0
    q = codes.to(torch.uint8)[None].repeat(n, 1).contiguous()  # [n, 256]: row r holds every code, K = 256 (8 blocks)
    s = (exps + 127).to(torch.uint8)[:, None].repeat(1, 8).contiguous()
    want = dequantize_mx8(q, s, torch.float32)  # exact in fp32
    assert torch.equal(want.to(dtype).float(), want)  # and in the dtype
    qd, sd_ = q.cuda(), s.cuda()
    for B in (1, 3):
        for k0 in range(0, 256, B):
            ks = [min(k0 + b, 255) for b in range(B)]
            x = torch.zeros(B, 256, dtype=dtype, device="cuda")
            for b, k in enumerate(ks):
                x[b, k] = 1
            y = torch.empty(B, n, dtype=dtype, device="cuda")
            ops.gemv_mx8(qd, sd_, y, x=x)
            got = y.float().cpu()
            for b, k in enumerate(ks):
                assert torch.equal(got[b], want[:, k]), (dtype, B, k)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. dl_gemv_mx8 in every mode at the decoder shapes
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _prologue_ref(h, delta, nw, eps, dtype):
    hn = h.float() if delta is None else (h.float() + delta.float()).to(dtype).float()
    r = torch.rsqrt(hn.pow(2).mean(-1, keepdim=True) + eps)
    return (nw.float() * (hn * r).to(dtype).float()).to(dtype), hn.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["tiny", "7b", "13b"])
def test_gemv_mx8_modes_vs_fp32_reference(dtype, which):
    g = torch.Generator(device="cuda").manual_seed(3)
    eps = 1e-5
    for N, K, kind in SHAPES[which]:
        W = (torch.randn(N, K, generator=g, device="cuda") / K**0.5).to(dtype)
        q, s = ops.quantize_mx8(W)
        Wp = dequantize_mx8(q, s, dtype)
        Wp64 = Wp.double()
        for B in (1, 2, 3):
            if B > ops.gemv_max_batch(K, dtype):
                continue
            h = torch.randn(B, K, generator=g, device="cuda").to(dtype)
            delta = (0.5 * torch.randn(B, K, generator=g, device="cuda")).to(dtype)
            nw = (1 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(dtype)
            if kind in ("qkv", "gu"):
                mode = ops.GEMV_ADDNORM | (ops.GEMV_OUT_SILU_PAIR if kind == "gu" else 0)
                x, _ = _prologue_ref(h, delta, nw, eps, dtype)
                y = torch.empty(B, N // 2 if kind == "gu" else N, dtype=dtype, device="cuda")
                h_out = torch.empty_like(h)
                ops.gemv_mx8(q, s, y, mode=mode, h_in=h, h_out=h_out, delta=delta, norm_w=nw, eps=eps)
                # h_out: bit-identical to dl_gemv's prologue on the same inputs
                y2 = torch.empty_like(y)
                h_out2 = torch.empty_like(h)
                ops.gemv(Wp, y2, mode=mode, h_in=h, h_out=h_out2, delta=delta, norm_w=nw, eps=eps)
                assert torch.equal(h_out.view(torch.uint8), h_out2.view(torch.uint8))
            else:
                mode = ops.GEMV_PLAIN
                x = torch.randn(B, K, generator=g, device="cuda").to(dtype)
                y = torch.empty(B, N, dtype=dtype, device="cuda")
                ops.gemv_mx8(q, s, y, x=x)
            acc = x.double() @ Wp64.T  # fp64 truth of the fp32 sum
            mag = x.double().abs() @ Wp64.abs().T  # scale of the fp32 summation noise
            U = ULP[dtype]
            noise = 1e-5 * mag
            if mode & ops.GEMV_ADDNORM:
                # the reference prologue's rsqrt may sit one fp32 ulp from the kernel's: an x element near a 16-bit rounding tie can then land one ulp away
                noise = noise + 8 * U * x.double().abs().amax(-1, keepdim=True) * Wp64.abs().amax(-1)[None]
            if kind == "gu":
                # through the epilogue cast(cast(silu(cast(g))) * cast(u)): one output-dtype rounding per step of the chain
                I = N // 2
                gg, uu = acc[:, :I], acc[:, I:]
                ref = torch.nn.functional.silu(gg) * uu
                tol = 1.1 * uu.abs() * (U * gg.abs() + noise[:, :I]) + (gg.abs() + 1) * (U * uu.abs() + noise[:, I:]) + 2 * U * ref.abs() + 1e-30
                err = (y.double() - ref).abs()
            else:
                rel = 1e-5 if dtype == torch.float32 else U
                tol = rel * acc.abs() + noise + 1e-30
                err = (y.double() - acc).abs()
            assert bool((err <= tol).all()), (which, N, K, kind, B, dtype, float((err - tol).max()))


def test_gemv_mx8_rejects_bad_arguments():
    dt = torch.bfloat16
    q, s = ops.quantize_mx8(torch.randn(64, 64, device="cuda").to(dt))
    x = torch.randn(1, 64, device="cuda").to(dt)
    y = torch.full((1, 64), 7.0, dtype=dt, device="cuda")
    lib = ops.lib()
    cases = [
        (0, q, s, 64, 48, 1, ops.dtype_code(dt)),  # K % 32
        (0, q, None, 64, 64, 1, ops.dtype_code(dt)),  # NULL scale
        (0, q, s, 64, 64, 9, ops.dtype_code(dt)),  # B over the maximum
        (0, q, s, 64, 64, 1, 9),  # unknown dtype
        (ops.GEMV_SILUMUL, q, s, 64, 64, 1, ops.dtype_code(dt)),  # mode outside the contract
    ]
    for mode, q_, s_, N, K, B, dc in cases:
        rc = lib.dl_gemv_mx8(mode, ops._p(q_), ops._p(s_), N, K, ops._p(x), 64, None, None, None, None, 0.0, ops._p(y), 64, B, dc, 0, ops._stream())
        assert rc == -1, (mode, N, K, B, dc)
    torch.cuda.synchronize()
    assert bool((y.float() == 7.0).all()), "a rejected call launched nothing"


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4.-6. the model in MXFP8 mode against the oracle on the host-dequantised state dict
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _tiny(dtype, seed=2):
    cfg = fx.tiny_config()
    sd = fx.make_state_dict(cfg, seed=seed, predictor_gain=50.0)
    clip = fx.build_clip(cfg, seed=1)
    return cfg, sd, clip


def test_generate_fp32_b1_vs_oracle_on_dequantised_weights():
    dtype = torch.float32
    cfg, sd, clip = _tiny(dtype)
    sdp = _sd_prime(sd, dtype)
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    assert model.knobs()["decode_weight_format"] == "mxfp8"
    ids = fx.make_prompt(cfg, 5, 7)[None]
    images = fx.make_images(cfg, 1)
    n = 8
    for graph in (False, True):
        model.use_hip_graph = graph
        out = model.generate(ids.cuda(), images=images.cuda(), max_new_tokens=n, eos_token_id=None)
        ref, _ = Oracle(cfg, sdp, dtype, clip=clip).greedy(ids, images=images, max_new_tokens=n, eos_token_id=None)
        assert out.cpu().tolist() == ref.tolist(), graph
    # step by step: logits, kept-image set, text decisions, KV lengths of both length groups
    model.debug_records = {}
    forced = fx.make_forced_tokens(cfg, 10, 1, seed=5)
    o = Oracle(cfg, sdp, dtype, clip=clip)
    with torch.no_grad():
        out = model(ids.cuda(), images=images.cuda())
        l, p = o.forward(ids, images=images)
        assert float((out.logits[0, -1].cpu() - l[0, -1]).abs().max()) < 1e-3
        assert torch.equal(model.debug_records["keep_index"].cpu(), o.records["keep_index"])
        pkv = out.past_key_values
        for j in range(10):
            out = model(forced[j][:, None].cuda(), past_key_values=pkv)
            pkv = out.past_key_values
            l, p = o.forward(forced[j][:, None], past_key_values=p)
            assert float((out.logits[0, -1].cpu() - l[0, -1]).abs().max()) < 1e-3, j
            assert bool(o.records["text_decision"][0, 0]) == bool(model.debug_records["text_decision"][0]), j
            assert int(p[1][-1][0]) == int(pkv[1][-1][0]) and int(p[1][0][0]) == int(pkv[1][0][0]), j


@pytest.mark.parametrize("B", [2, 3])
def test_batched_rows_equal_their_b1_oracle_runs(B):
    dtype = torch.float32
    cfg, sd, clip = _tiny(dtype)
    sdp = _sd_prime(sd, dtype)
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    prompts = [fx.make_prompt(cfg, 5, 7, seed=0), fx.make_prompt(cfg, 2, 15, seed=1), fx.make_prompt(cfg, 9, 3, seed=2)][:B]
    steps = 8
    images = fx.make_images(cfg, B, seed=3)
    forced = fx.make_forced_tokens(cfg, steps, B, seed=5)
    n = max(p.shape[0] for p in prompts)
    ids = torch.zeros(B, n, dtype=torch.long)
    am = torch.zeros(B, n, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]] = p
        am[b, : p.shape[0]] = 1
    model.debug_records = {}
    with torch.no_grad():
        out = model(ids.cuda(), attention_mask=am.cuda(), images=images.cuda())
        pkv = out.past_key_values
        cu = model.debug_records["cu_after"].cpu().tolist()
        hip = [[out.logits[b, cu[b + 1] - cu[b] - 1].cpu() for b in range(B)]]
        dec = []
        for j in range(steps):
            out = model(forced[j][:, None].cuda(), past_key_values=pkv)
            pkv = out.past_key_values
            hip.append([out.logits[b, -1].cpu() for b in range(B)])
            dec.append(model.debug_records["text_decision"].cpu().clone())
        for b in range(B):
            o = Oracle(cfg, sdp, dtype, clip=clip)
            l, p = o.forward(prompts[b][None], images=images[b : b + 1])
            assert float((l[0, -1] - hip[0][b]).abs().max()) < 1e-3
            for j in range(steps):
                l, p = o.forward(forced[j][b : b + 1][:, None], past_key_values=p)
                assert float((l[0, -1] - hip[j + 1][b]).abs().max()) < 1e-3, (b, j)
                assert bool(o.records["text_decision"][0, 0]) == bool(dec[j][b]), (b, j)
            assert int(p[1][-1][0]) == int(pkv[1][-1][b]) and int(p[1][0][0]) == int(pkv[1][0][b])
    # greedy generate: every row equals its own B=1 run of the same MXFP8 model
    gen = model.generate(ids.cuda(), attention_mask=am.cuda(), images=images.cuda(), max_new_tokens=6, eos_token_id=None).cpu()
    for b in range(B):
        one = model.generate(prompts[b][None].cuda(), images=images[b : b + 1].cuda(), max_new_tokens=6, eos_token_id=None).cpu()
        assert gen[b].tolist() == one[0].tolist(), b


def test_bf16_tiny_noise_class_vs_oracle_on_dequantised_weights():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny(dtype)
    sdp = _sd_prime(sd, dtype)
    model = _build(cfg, sd, clip, dtype, "mxfp8")
    clip16 = copy.deepcopy(clip).to(dtype)
    o = Oracle(cfg, sdp, dtype, clip=clip16)
    o32 = Oracle(cfg, sdp, torch.float32, clip=clip16)
    ids = fx.make_prompt(cfg, 5, 7)[None]
    images = fx.make_images(cfg, 1).to(dtype)
    forced = fx.make_forced_tokens(cfg, 8, 1, seed=5)
    model.debug_records = {}
    n_forced = 0
    with torch.no_grad():
        out = model(ids.cuda(), images=images.cuda())
        keep = model.debug_records["keep_index"].cpu()
        o.force_keep_index = keep
        o32.force_keep_index = keep
        l, p = o.forward(ids, images=images)
        l32, p32 = o32.forward(ids, images=images.float())
        pkv = out.past_key_values
        for j in range(8):
            out = model(forced[j][:, None].cuda(), past_key_values=pkv)
            pkv = out.past_key_values
            hd = bool(model.debug_records["text_decision"][0])
            htl = model.debug_records["text_logit"].float().cpu()[0]
            res = []
            for orc, pp in ((o, p), (o32, p32)):
                l_, p_ = orc.forward(forced[j][:, None], past_key_values=pp)
                if bool(orc.records["text_decision"][0, 0]) != hd:
                    assert fx.decision_may_differ(orc.records["text_logit"][0, 0], orc.dtype, htl, dtype), j
                    orc.force_text_decision = torch.tensor([[int(hd)]])
                    l_, p_ = orc.forward(forced[j][:, None], past_key_values=pp)
                    orc.force_text_decision = None
                    n_forced += 1
                res.append((l_, p_))
            (l, p), (l32, p32) = res
            e_hip = float((out.logits[0, -1].float().cpu() - l32[0, -1]).abs().max())
            e_ref = float((l[0, -1].float() - l32[0, -1]).abs().max())
            assert e_hip <= 2.0 * e_ref + 2 * ULP[dtype] * float(l32[0, -1].abs().max()), (j, e_hip, e_ref)
    assert n_forced <= 2 * fx.MAX_FORCED_DECISIONS


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 7. MXFP8 mode against the format-off model on W'
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _decode_logits(model, ids, am, images, forced, steps):
    model.debug_records = {}
    with torch.no_grad():
        out = model(ids.cuda(), attention_mask=am.cuda(), images=images.cuda())
        pre = out.logits.cpu()
        pkv = out.past_key_values
        ls = []
        for j in range(steps):
            out = model(forced[j][:, None].cuda(), past_key_values=pkv)
            pkv = out.past_key_values
            ls.append(out.logits[:, -1].cpu())
    return pre, ls, [x.cpu().clone() for x in pkv[1]]


def _batch(cfg, B, seed=0):
    prompts = [fx.make_prompt(cfg, 2 + (3 * b) % 7, 4 + (5 * b) % 11, seed=seed + b) for b in range(B)]
    n = max(p.shape[0] for p in prompts)
    ids = torch.zeros(B, n, dtype=torch.long)
    am = torch.zeros(B, n, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]] = p
        am[b, : p.shape[0]] = 1
    return ids, am


def test_mxfp8_mode_vs_format_off_model_on_w_prime():
    dtype = torch.float32
    cfg, sd, clip = _tiny(dtype)
    sdp = _sd_prime(sd, dtype)
    mx = _build(cfg, sd, clip, dtype, "mxfp8")
    off = _build(cfg, sdp, clip, dtype)
    # the weights the MXFP8 model holds ARE the host-dequantised ones
    for (k, v) in off.state_dict().items():
        if _PROJ.match(k):
            assert torch.equal(mx.state_dict()[k], v), k
    images = fx.make_images(cfg, 8, seed=3)
    for B in (1, 2, 3, 4, 8):
        ids, am = _batch(cfg, B)
        forced = fx.make_forced_tokens(cfg, 6, B, seed=5)
        pm, lm, km = _decode_logits(mx, ids, am, images[:B], forced, 6)
        po, lo, ko = _decode_logits(off, ids, am, images[:B], forced, 6)
        assert torch.equal(pm, po), f"prefill logits B={B}"
        if B >= 4:  # the FP8 path is not taken: bit-identical
            assert all(torch.equal(a, b) for a, b in zip(lm, lo)), f"decode B={B}"
            assert all(torch.equal(a, b) for a, b in zip(km, ko))
        else:
            assert all(float((a - b).abs().max()) < 1e-3 for a, b in zip(lm, lo)), f"decode B={B}"
        gm = mx.generate(ids.cuda(), attention_mask=am.cuda(), images=images[:B].cuda(), max_new_tokens=8, eos_token_id=None)
        go = off.generate(ids.cuda(), attention_mask=am.cuda(), images=images[:B].cuda(), max_new_tokens=8, eos_token_id=None)
        assert torch.equal(gm, go), f"tokens B={B}"
    # hipGraph and eager bit-identical in MXFP8 mode
    ids, am = _batch(cfg, 1)
    outs = []
    for graph in (True, False):
        mx.use_hip_graph = graph
        outs.append(mx.generate(ids.cuda(), images=images[:1].cuda(), max_new_tokens=10, eos_token_id=None, output_scores=True, return_dict_in_generate=True))
    assert torch.equal(outs[0]["sequences"], outs[1]["sequences"])
    assert all(torch.equal(a, b) for a, b in zip(outs[0]["scores"], outs[1]["scores"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 8. 7B / 13B widths, bf16, a few layers: against the format-off model on W'
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["7b", "13b"])
def test_full_width_vs_format_off_model(width):
    dtype = torch.bfloat16
    cfg = fx.llava7b_config(num_hidden_layers=3) if width == "7b" else fx.llava13b_config(num_hidden_layers=3)
    H = cfg.hidden_size
    sd = fx.make_state_dict(cfg, seed=7, predictor_gain=50.0)
    sdp = _sd_prime(sd, dtype)
    mx = _build(cfg, sd, None, dtype, "mxfp8")
    off = _build(cfg, sdp, None, dtype)
    truth = _build(cfg, {k: v.float() for k, v in sdp.items()}, None, torch.float32)  # fp32 model on the same W' values
    g = torch.Generator().manual_seed(21)
    steps = 16
    for B in (1, 2, 3):
        feats = torch.randn(B, 576, H, generator=g)
        ids = torch.stack([fx.make_prompt(cfg, 35, 20, seed=4 + b) for b in range(B)])
        forced = fx.make_forced_tokens(cfg, steps, B, seed=6)
        models = {"mx": mx, "off": off, "truth": truth}
        state = {}
        n_forced = 0
        with torch.no_grad():
            for k, m in models.items():
                m.debug_records = {}
                out = m(ids.cuda(), image_features=feats.to(m.dtype).cuda())
                state[k] = out.past_key_values
            for j in range(steps):
                logits = {}
                off_dec = off_tl = None
                for k in ("off", "truth", "mx"):
                    m = models[k]
                    out = m(forced[j][:, None].cuda(), past_key_values=state[k])
                    dec = m.debug_records["text_decision"].cpu().clone().reshape(-1)
                    if k == "off":
                        off_dec, off_tl = dec, m.debug_records["text_logit"].float().cpu()
                    elif not torch.equal(dec.bool(), off_dec.bool()):
                        # an eviction decision that fell the other way inside the boundary band: this model repeats the step (on the pre-step cache) with
                        # the format-off model's decision, so the caches stay comparable
                        tl = m.debug_records["text_logit"].float().cpu()
                        for b in range(B):
                            if bool(dec[b]) != bool(off_dec[b]):
                                assert fx.decision_may_differ(tl[b], m.dtype, off_tl[b], dtype), (width, B, j, k)
                        n_forced += 1
                        m.force_text_decision = off_dec.view(-1, 1)
                        out = m(forced[j][:, None].cuda(), past_key_values=state[k])
                        m.force_text_decision = None
                    state[k] = out.past_key_values
                    logits[k] = out.logits[:, -1].float().cpu()
                e_mx = (logits["mx"] - logits["truth"]).abs().amax(-1)
                e_off = (logits["off"] - logits["truth"]).abs().amax(-1)
                scale = logits["truth"].abs().amax(-1)
                assert bool((e_mx <= 2.0 * e_off + 2 * ULP[dtype] * scale).all()), (width, B, j, e_mx.tolist(), e_off.tolist())
                # identical greedy choice unless the top two logits of the fp32 truth are within the noise of the two 16-bit runs
                t2 = logits["truth"].topk(2, dim=-1).values
                gap = t2[:, 0] - t2[:, 1]
                same = logits["mx"].argmax(-1) == logits["off"].argmax(-1)
                assert bool((same | (gap <= e_mx + e_off)).all()), (width, B, j)
            lm = [int(x) for x in state["mx"][1][-1].cpu().reshape(-1)]
            lo = [int(x) for x in state["off"][1][-1].cpu().reshape(-1)]
            assert lm == lo, "KV lengths of the evicting layers"
        assert n_forced <= 2 * fx.MAX_FORCED_DECISIONS * B
    assert mx.decode_weight_bytes()["mxfp8"] == 3 * sum(N * K + N * K // 32 for N, K, _ in SHAPES[width])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 9.-10. weight changes and switching the format off
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_weight_changed_after_quantisation_is_requantised():
    dtype = torch.float32
    cfg, sd, clip = _tiny(dtype)
    mx = _build(cfg, sd, clip, dtype, "mxfp8")
    ids, am = _batch(cfg, 1)
    images = fx.make_images(cfg, 1, seed=3)
    before = mx.generate(ids.cuda(), images=images.cuda(), max_new_tokens=8, eos_token_id=None, output_scores=True, return_dict_in_generate=True)
    codes_before = mx.model.layers[1].mx8["down"][0].clone()
    # an in-place edit of one decoder weight after set_decode_weight_format
    sd2 = dict(sd)
    k = "model.layers.1.mlp.down_proj.weight"
    sd2[k] = sd[k] * 3.0 + 0.01
    with torch.no_grad():
        mx.model.layers[1].mlp.down_proj.weight.copy_(sd2[k].cuda())
    after = mx.generate(ids.cuda(), images=images.cuda(), max_new_tokens=8, eos_token_id=None, output_scores=True, return_dict_in_generate=True)
    assert not torch.equal(mx.model.layers[1].mx8["down"][0], codes_before)
    fresh = _build(cfg, sd2, clip, dtype, "mxfp8")
    want = fresh.generate(ids.cuda(), images=images.cuda(), max_new_tokens=8, eos_token_id=None, output_scores=True, return_dict_in_generate=True)
    assert torch.equal(after["sequences"], want["sequences"])
    assert all(torch.equal(a, b) for a, b in zip(after["scores"], want["scores"]))
    assert not all(torch.equal(a, b) for a, b in zip(after["scores"], before["scores"]))
    # and the parameter itself now holds W'' (the re-quantised value)
    q, s = quantize_mx8(sd2[k], dtype)
    assert torch.equal(mx.model.layers[1].mlp.down_proj.weight.cpu(), dequantize_mx8(q, s, dtype))


def test_format_none_restores_the_model_dtype_kernels():
    dtype = torch.bfloat16
    cfg, sd, clip = _tiny(dtype)
    sdp = _sd_prime(sd, dtype)
    mx = _build(cfg, sd, clip, dtype, "mxfp8")
    off = _build(cfg, sdp, clip, dtype)
    mx.set_decode_weight_format(None)
    assert mx.knobs()["decode_weight_format"] is None and mx.decode_weight_bytes()["total"] == 0
    assert all(getattr(l, "mx8", None) is None for l in mx.model.layers)
    ids, am = _batch(cfg, 1)
    images = fx.make_images(cfg, 1, seed=3).to(dtype)
    forced = fx.make_forced_tokens(cfg, 6, 1, seed=5)
    pm, lm, km = _decode_logits(mx, ids, am, images, forced, 6)
    po, lo, ko = _decode_logits(off, ids, am, images, forced, 6)
    assert torch.equal(pm, po) and all(torch.equal(a, b) for a, b in zip(lm, lo)) and all(torch.equal(a, b) for a, b in zip(km, ko))
    with pytest.raises(ValueError):
        mx.set_decode_weight_format("fp4")
