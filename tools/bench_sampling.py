#!/usr/bin/env python
"""Sampled decoding, ms per step: greedy (dl_decode_advance in the graph), device-sampled (generate(do_sample=True, seed=...): dl_decode_sample in the
same graph) and today's loop (generator=: forward() per step, torch sort / softmax / cumsum / multinomial), alternated inside one process on the
7B-shaped random-init model of tools/bench_decode_batch.py.  B = 1 and B = 32, 64 new tokens, T = 0.2 and (T = 0.7, top_p = 0.9, top_k = 50).
ms/step = (time of 65 new tokens - time of 1 new token) / 64; every variant is repeated `--reps` times, min / median / max reported (the spread
is what "faster" is judged against).
    python tools/bench_sampling.py [--out profiles/sampling_decode_bench.json] [--batches 1 32] [--reps 5] [--trace-only]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamic_llava_amd.builder import build_random_model
from dynamic_llava_amd.config import DynamicLlavaConfig
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 32])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--trace-only", action="store_true", help="one warm greedy and one warm device-sampled request at B = 1 (for a kernel trace), no timing")
args = ap.parse_args()

cfg = DynamicLlavaConfig(num_hidden_layers=args.layers)
model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
prompt, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
feats = model.encode_images(images)
SETTINGS = {"T0.2": dict(temperature=0.2), "T0.7_p0.9_k50": dict(temperature=0.7, top_p=0.9, top_k=50)}


def run(B, n_new, variant, setting):
    ids = prompt.expand(B, -1).contiguous()
    f = feats.expand(B, -1, -1).contiguous()
    kw = dict(image_features=f, max_new_tokens=n_new, eos_token_id=None)
    if variant == "device":
        kw.update(do_sample=True, seed=1234, **SETTINGS[setting])
    elif variant == "loop":
        kw.update(do_sample=True, generator=torch.Generator(device="cuda").manual_seed(1234), **SETTINGS[setting])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    model.generate(ids, **kw)
    torch.cuda.synchronize(); return time.perf_counter() - t0


if args.trace_only:
    for variant in ("greedy", "device"):
        for _ in range(4):
            run(1, 33, variant, "T0.7_p0.9_k50")
    sys.exit(0)

result = {"model": f"7B-shaped random init, {args.layers} layers, bf16", "new_tokens": 64, "reps": args.reps, "knobs": {"device_sampling": model.knobs()["device_sampling"]}, "rows": []}
for B in args.batches:
    model._dstate = None
    for setting in SETTINGS:
        variants = ("greedy", "device", "loop")
        for v in variants:  # warm: first sighting, capture, replay
            for _ in range(3):
                run(B, 65, v, setting); run(B, 1, v, setting)
        ms = {v: [] for v in variants}
        for _ in range(args.reps):  # alternated: every repetition times all three
            for v in variants:
                ms[v].append((run(B, 65, v, setting) - run(B, 1, v, setting)) / 64 * 1e3)
        row = {"B": B, "setting": setting}
        for v in variants:
            row[v + "_ms_per_step"] = {"min": round(min(ms[v]), 4), "median": round(statistics.median(ms[v]), 4), "max": round(max(ms[v]), 4)}
        row["device_minus_greedy_ms"] = round(statistics.median(ms["device"]) - statistics.median(ms["greedy"]), 4)
        row["loop_over_device"] = round(statistics.median(ms["loop"]) / statistics.median(ms["device"]), 2)
        row["device_faster_than_loop_beyond_spread"] = bool(max(ms["device"]) < min(ms["loop"]) and (min(ms["loop"]) - max(ms["device"])) > (max(ms["loop"]) - min(ms["loop"])))
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
