#!/usr/bin/env python
"""MXFP8 decoder weights: decode ms/token at B = 1, 2, 3 for the 7B and the 13B widths (random init, full depth, bf16 activations), format off vs
"mxfp8", plus the per-launch time of the four dl_gemv_mx8 calls of one layer at B = 1 (and of the dl_gemv launches they replace) with their streamed
bytes (codes + scales) as a fraction of the 8 TB/s spec and of the box's measured read-only stream ceiling.  Prints one JSON line.

    python tools/bench_mxfp8_decode.py [--widths 7b,13b] [--steps 64]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="7b,13b")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batches", default="1,2,3")
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
