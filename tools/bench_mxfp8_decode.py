#!/usr/bin/env python
"""MXFP8 decoder weights: decode ms/token at B = 1, 2, 3 for the 7B and the 13B widths (random init, full depth, bf16 activations), format off vs
"mxfp8", plus the per-launch time of the four dl_gemv_mx8 calls of one layer at B = 1 (and of the dl_gemv launches they replace) with their streamed
bytes (codes + scales) as a fraction of the 8 TB/s spec and of the box's measured read-only stream ceiling.  Prints one JSON line.

    python tools/bench_mxfp8_decode.py [--widths 7b,13b] [--steps 64] [--batches 1,2,3]

With --max-batch N (set_decode_weight_format("mxfp8", max_batch=N)) the table is the batched one instead: for every batch size of --batches, "mxfp8" without max_batch
(the model-dtype kernels on W': what such a step ran before dl_gemm_mx8) against max_batch = N, --reps repetitions of each side taken alternately, the minimum and the
spread (max - min) of each side; a batch size counts as faster only if the candidate's minimum beats the baseline's by more than the larger spread.  Plus the per-launch
times of the four dl_gemm_mx8 calls of one layer at B = 8 and 32 beside the launches they replace.

    python tools/bench_mxfp8_decode.py --max-batch 32 --batches 4,8,16,24,32"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_llava_amd import hip_ops as ops  # noqa: E402
from dynamic_llava_amd.builder import build_random_model  # noqa: E402
from dynamic_llava_amd.config import DynamicLlavaConfig  # noqa: E402

SPEC_TBS = 8.0
READ_CEILING_TBS = 6.85  # read-only stream ceiling bench.py measured on this box model (BENCH_r06.json measured_ceilings)


def _cfg(width):
    if width == "7b":
        return DynamicLlavaConfig()
    return DynamicLlavaConfig(hidden_size=5120, intermediate_size=13824, num_hidden_layers=40, num_attention_heads=40, num_key_value_heads=40)


def _decode_ms(model, B, steps, feats, prompt):
    ids = prompt.expand(B, -1).contiguous()
    f = feats.expand(B, -1, -1).contiguous()

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate(ids, image_features=f, max_new_tokens=n, eos_token_id=None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    run(steps + 1), run(1)  # capture + warm
    t = min(run(steps + 1) for _ in range(3)) - min(run(1) for _ in range(3))
    return t / steps * 1e3


def _launch_us(fn, reps=200):
    for _ in range(10):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2]


def _per_launch(model):
    """B = 1, layer 0: dl_gemv_mx8 (format on) and dl_gemv on the same W' (what the format-off step streams in these four projections)."""
    l = model.model.layers[0]
    cfg = model.config
    H, I = cfg.hidden_size, cfg.intermediate_size
    dev, dt = model.device, model.dtype
    h = torch.randn(1, H, device=dev).to(dt)
    h2 = torch.empty_like(h)
    delta = torch.randn(1, H, device=dev).to(dt)
    nw = l.input_layernorm.weight
    xa = torch.randn(1, H, device=dev).to(dt)
    xg = torch.randn(1, I, device=dev).to(dt)
    out = {}
    A = ops.GEMV_ADDNORM
    cases = {
        "qkv": (l.w_qkv, l.mx8["qkv"], A, l.w_qkv.shape[0]),
        "o": (l.self_attn.o_proj.weight, l.mx8["o"], ops.GEMV_PLAIN, H),
        "gate_up": (l.w_gu, l.mx8["gu"], A | ops.GEMV_OUT_SILU_PAIR, I),
        "down": (l.mlp.down_proj.weight, l.mx8["down"], ops.GEMV_PLAIN, H),
    }
    for name, (w, (q, sc), mode, n_out) in cases.items():
        y = torch.empty(1, n_out, device=dev, dtype=dt)
        x = xg if name == "down" else xa
        kw = dict(mode=mode, h_in=h, h_out=h2, delta=delta, norm_w=nw, eps=1e-5) if mode & A else dict(x=x)
        us_mx = _launch_us(lambda: ops.gemv_mx8(q, sc, y, **kw))
        us_bf = _launch_us(lambda: ops.gemv(w, y, **kw))
        by_mx = q.numel() + sc.numel()
        by_bf = w.numel() * w.element_size()
        out[name] = {"N": int(q.shape[0]), "K": int(q.shape[1]), "mx8_us": round(us_mx, 2), "bf16_us": round(us_bf, 2), "mx8_bytes": by_mx, "bf16_bytes": by_bf,
                     "mx8_tbs": round(by_mx / us_mx / 1e6, 3), "mx8_frac_spec": round(by_mx / us_mx / 1e6 / SPEC_TBS, 3),
                     "mx8_frac_read_ceiling": round(by_mx / us_mx / 1e6 / READ_CEILING_TBS, 3), "bf16_frac_spec": round(by_bf / us_bf / 1e6 / SPEC_TBS, 3)}
    tot_us = sum(v["mx8_us"] for v in out.values())
    tot_by = sum(v["mx8_bytes"] for v in out.values())
    out["layer_total"] = {"mx8_us": round(tot_us, 2), "bf16_us": round(sum(v["bf16_us"] for v in out.values()), 2), "mx8_bytes": tot_by,
                          "mx8_frac_spec": round(tot_by / tot_us / 1e6 / SPEC_TBS, 3), "mx8_frac_read_ceiling": round(tot_by / tot_us / 1e6 / READ_CEILING_TBS, 3)}
    return out


def _set_max_batch(model, mb):
    """set_decode_weight_format("mxfp8", max_batch=mb) without its finalize() (the codes and W' stay as they are: only the decode state, whose route and graphs
    belong to the old setting, is dropped) -- the two sides of the batched table alternate many times."""
    from dynamic_llava_amd.mxfp8 import check_decode_weight_format

    check_decode_weight_format("mxfp8", mb, model.gemv_max_decode_batch)
    model.mx8_max_decode_batch = mb
    model._dstate = None


def _batched_table(model, batches, max_batch, steps, reps, feats, prompt):
    out = {}
    for B in batches:
        t = {None: [], max_batch: []}
        for mb in (None, max_batch):  # every shape of both sides warmed up before anything is timed
            _set_max_batch(model, mb)
            _decode_ms(model, B, 4, feats, prompt)
        for _ in range(reps):
            for mb in (None, max_batch):
                _set_max_batch(model, mb)
                t[mb].append(_decode_ms(model, B, steps, feats, prompt))
                st = model._dstate
                assert st.B == B and st.use_mx8_gemm == (mb is not None and B <= mb), "the side ran on the other route"
        b, c = t[None], t[max_batch]
        spread = max(max(b) - min(b), max(c) - min(c))
        out[f"B{B}"] = {"baseline_ms": round(min(b), 4), "baseline_spread": round(max(b) - min(b), 4), "candidate_ms": round(min(c), 4), "candidate_spread": round(max(c) - min(c), 4),
                        "speedup": round(min(b) / min(c), 4), "faster": bool(min(b) - min(c) > spread)}
    return out


def _graph_us(fns, reps=5):
    """us per launch of a captured graph that holds every fn once (one fn per decoder layer: the weights of each launch are cold, as in the step)."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fns:
            f()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / len(fns))
    return min(ts)


def _per_launch_batched(model, B):
    """B rows, every layer's weights in turn inside one captured graph: the four dl_gemm_mx8 calls of _decode_layer_gemm_mx8 (q|k|v with its reduce launch, gate|up
    with the dl_silu_mul_parts launch it needs) and the launches of _decode_step_gemm they replace (dl_gemm_smallm / dl_linear_packed / dl_linear_tiles on W', chosen
    as the step chooses them)."""
    from dynamic_llava_amd.decode import _DecodeState

    cfg, dev, dt = model.config, model.device, model.dtype
    H, I = cfg.hidden_size, cfg.intermediate_size
    Nq = model.model.layers[0].w_qkv.shape[0]
    _set_max_batch(model, 32)
    sm = _DecodeState(model, B, dev, dt, 1)
    _set_max_batch(model, None)
    sb = _DecodeState(model, B, dev, dt, 1)
    assert sm.use_mx8_gemm and not sb.use_mx8_gemm
    x = torch.randn(B, H, device=dev).to(dt)
    attn = torch.randn(B, H, device=dev).to(dt)
    act = torch.randn(B, I, device=dev).to(dt)
    ws = sm.mx8_ws
    lp = sb.use_lp_mlp
    x_pk = ops.pack_x_tiles(x) if lp else None
    act_pk = ops.pack_x_tiles(act) if lp else None
    l0 = model.model.layers[0]
    lp_q = lp and B >= model.packed_decode_qkv_min_batch and getattr(l0, "wp_qkv", None) is not None
    tiles_o = model.tiles_o_proj and sb.o_parts is not None and B >= model.tiles_o_proj_min_decode_batch and getattr(l0, "wp_o", None) is not None
    how = {"qkv": "dl_linear_packed" if lp_q else "dl_gemm_smallm", "o": "dl_linear_tiles" if tiles_o else "dl_gemm_smallm",
           "gate_up": "dl_linear_packed" if lp else "dl_gemm_smallm + dl_silu_mul_parts", "down": "dl_linear_packed" if lp else "dl_gemm_smallm"}
    nu_q, ks_q = model._lp_config(Nq // 16, False)
    nu_g, ks_g = model._lp_config(2 * I // 16, True)
    nu_d, ks_d = model._lp_config_parts(H // 16)
    shp, ks_o = model._tiles_o_config(B, H)
    lpw = lambda ks: model._lp_ws if ks > 1 else None

    def mx(l):
        m = l.mx8
        return {"qkv": lambda: ops.gemm_mx8(x, *m["qkv"], out=sm.qkv, workspace=ws), "o": lambda: ops.gemm_mx8_parts(attn, *m["o"], ws),
                "gate_up": lambda: ops.silu_mul_parts(ops.gemm_mx8_parts(x, *m["gu"], ws)[0], sm.act), "down": lambda: ops.gemm_mx8_parts(act, *m["down"], ws)}

    def base(l):
        d = {}
        if lp_q:
            d["qkv"] = lambda: ops.linear_packed(x_pk, l.wp_qkv, Nq, out=sb.qkv, units_per_workgroup=nu_q, k_split=ks_q, workspace=lpw(ks_q), err=model._lp_err, x_packed_mk=(B, H))
        else:
            d["qkv"] = lambda: ops.gemm_smallm(x, l.w_qkv, out=sb.qkv, workspace=sb.lin_ws, n_slices=model.smallm_wide_slices)
        if tiles_o:
            d["o"] = lambda: ops.linear_tiles(attn, l.wp_o, H, out=sb.o_parts[: ks_o * B * H], epilogue=ops.LT_PARTS, tile_shape=shp, k_split=ks_o)
        else:
            d["o"] = lambda: ops.gemm_smallm_parts(attn, l.self_attn.o_proj.weight, sb.lin_ws)
        if lp:
            d["gate_up"] = lambda: ops.linear_packed(x_pk, l.wp_gu, 2 * I, out=sb.act_pk, epilogue=ops.LP_SILU_PAIR, units_per_workgroup=nu_g, k_split=ks_g, workspace=lpw(ks_g), err=model._lp_err,
                                                     x_packed_mk=(B, H), y_packed=True)
            d["down"] = lambda: ops.linear_packed(act_pk, l.wp_down, H, out=sb.lp_parts, epilogue=ops.LP_PARTS, units_per_workgroup=nu_d, k_split=ks_d, x_packed_mk=(B, I))
        else:
            d["gate_up"] = lambda: ops.silu_mul_parts(ops.gemm_smallm_parts(x, l.w_gu, sb.lin_ws, n_slices=model.smallm_wide_slices)[0], sb.act)
            d["down"] = lambda: ops.gemm_smallm_parts(act, l.mlp.down_proj.weight, sb.lin_ws)
        return d

    out = {}
    for name in ("qkv", "o", "gate_up", "down"):
        q, sc = l0.mx8["gu" if name == "gate_up" else name]
        us_mx = _graph_us([mx(l)[name] for l in model.model.layers])
        us_b = _graph_us([base(l)[name] for l in model.model.layers])
        by_mx, by_b = q.numel() + sc.numel(), q.numel() * 2
        out[name] = {"N": int(q.shape[0]), "K": int(q.shape[1]), "mx8_us": round(us_mx, 2), "replaced_us": round(us_b, 2), "replaced": how[name], "mx8_bytes": by_mx, "replaced_bytes": by_b,
                     "mx8_tbs": round(by_mx / us_mx / 1e6, 3), "mx8_frac_spec": round(by_mx / us_mx / 1e6 / SPEC_TBS, 3), "mx8_frac_read_ceiling": round(by_mx / us_mx / 1e6 / READ_CEILING_TBS, 3),
                     "replaced_frac_spec": round(by_b / us_b / 1e6 / SPEC_TBS, 3)}
    tot_us, tot_by = sum(v["mx8_us"] for v in out.values()), sum(v["mx8_bytes"] for v in out.values())
    out["layer_total"] = {"mx8_us": round(tot_us, 2), "replaced_us": round(sum(v["replaced_us"] for v in out.values()), 2), "mx8_bytes": tot_by,
                          "mx8_frac_spec": round(tot_by / tot_us / 1e6 / SPEC_TBS, 3), "mx8_frac_read_ceiling": round(tot_by / tot_us / 1e6 / READ_CEILING_TBS, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="7b,13b")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batches", default="1,2,3")
    ap.add_argument("--max-batch", type=int, default=None, help="the batched table: 'mxfp8' without max_batch against max_batch = this")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--per-launch", default="8,32", help="batch sizes of the per-launch comparison of the batched table ('' = none)")
    a = ap.parse_args()
    import bench  # the headline's inputs (prompt + image), unchanged

    res = {"tool": "bench_mxfp8_decode", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "steps": a.steps, "spec_tbs": SPEC_TBS,
           "read_ceiling_tbs": READ_CEILING_TBS, "widths": {}}
    for width in a.widths.split(","):
        cfg = _cfg(width)
        model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
        prompt, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
        feats = torch.randn(1, 576, cfg.hidden_size, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)).to(torch.bfloat16)
        r = {"layers": cfg.num_hidden_layers, "decode_ms_per_token": {}}
        t0 = time.perf_counter()
        model.set_decode_weight_format("mxfp8")
        r["quantise_s"] = round(time.perf_counter() - t0, 3)
        r["decode_weight_bytes"] = model.decode_weight_bytes()["total"]
        if a.max_batch is not None:
            r.pop("decode_ms_per_token")
            r["max_batch"] = a.max_batch
            r["decode_ms_per_token_batched"] = _batched_table(model, list(map(int, a.batches.split(","))), a.max_batch, a.steps, a.reps, feats, prompt)
            print(json.dumps({"width": width, "decode_ms_per_token_batched": r["decode_ms_per_token_batched"]}), file=sys.stderr, flush=True)
            r["per_launch_batched"] = {f"B{B}": _per_launch_batched(model, B) for B in map(int, filter(None, a.per_launch.split(",")))}
            _set_max_batch(model, None)
            res["widths"][width] = r
            del model
            torch.cuda.empty_cache()
            continue
        for fmt in (None, "mxfp8"):
            model.set_decode_weight_format(fmt)  # (the weights stay W' throughout: the bf16 timing does not depend on their values)
            for B in map(int, a.batches.split(",")):
                r["decode_ms_per_token"][f"{fmt or 'bf16'}_B{B}"] = round(_decode_ms(model, B, a.steps, feats, prompt), 4)
        r["per_launch_b1"] = _per_launch(model)
        res["widths"][width] = r
        del model
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
