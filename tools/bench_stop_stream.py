#!/usr/bin/env python
"""Stop sequences and token streaming, decode ms per step, on the 7B-shaped random-init model of bench.py (BASELINE configs[1] prompt: 631 tokens, bf16) at
B = 1 and B = 32 rows with 64 new tokens, three requests alternated inside each repetition:
  (a)  the plain greedy generate();
  (b)  the same with a stop list that never matches (8 sequences of 8 tokens: dl_decode_stop behind every step-closing launch, the loop reads the flags);
  (c)  (b) with a no-op streamer (put / end do nothing: what is timed is the feed -- the first token's blocking read, one more pinned copy per chunk).
  (d)  the launch alone: dl_decode_stop on [B, 128] tokens with the full table (bench.graph_time_ms: launches captured into one graph, so the figure includes
       the dependent-launch gap).
ms/step = (time with 65 tokens - time with 1 token) / 64, host clock around calls that end in a device synchronise; every request is warmed 3 times, then repeated
`--reps` (>= 10) times; min / median / max reported.
    python tools/bench_stop_stream.py [--out profiles/stop_stream_decode_bench.json] [--reps 10] [--layers 32] [--batches 1,32]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamic_llava_amd import hip_ops as ops
from dynamic_llava_amd.builder import build_random_model
from dynamic_llava_amd.config import DynamicLlavaConfig
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--batches", default="1,32")
args = ap.parse_args()
assert args.reps >= 10, "at least 10 timed repetitions"
if not torch.cuda.is_available():
    sys.exit("bench_stop_stream.py measures on the GPU: no HIP device visible")


class NoOpStreamer:
    def put(self, t):
        pass

    def end(self):
        pass


T = 64
cfg = DynamicLlavaConfig(num_hidden_layers=args.layers)
model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
prompt1, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
calib = bench.calibrate_text_predictor(model, prompt1, images, T)
feats1 = model.encode_images(images)
free = model.generate(prompt1, image_features=feats1, max_new_tokens=T + 1, eos_token_id=None).reshape(-1).tolist()
unused = [v for v in range(1000, cfg.vocab_size) if v not in set(free)][:8]  # every sequence ends in an id the run never emits: no tail can match
NEVER = [[3, 4, 5, 6, 7, 8, 9, u] for u in unused]
KW = {"a": {}, "b": dict(stop_sequences=NEVER), "c": dict(stop_sequences=NEVER, streamer=NoOpStreamer())}
routes = ("a", "b", "c")


def run(route, n, prompt, feats):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = model.generate(prompt, image_features=feats, max_new_tokens=n, eos_token_id=None, **KW[route])
    assert res.shape[1] == n  # (nothing stopped)
    res.sum().item()
    torch.cuda.synchronize(); return time.perf_counter() - t0


def save():  # (after every stage: a run that is cut short leaves what it measured)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


stat = lambda xs: {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}
result = {"model": f"7B-shaped random init, {args.layers} layers, bf16, prompt 631 tokens (BASELINE configs[1]), {T} new tokens", "text_predictor_calibrated_keep_fraction": calib,
          "method": f"ms/step = (t(65 tokens) - t(1 token)) / 64; {args.reps} repetitions after 3 warm-ups, the three requests alternated inside a repetition",
          "requests": {"a": "plain", "b": "8 never-matching stop sequences of 8 tokens", "c": "b + a no-op streamer"}, "decode_ms_per_step": {}}
for B in [int(b) for b in args.batches.split(",")]:
    prompt, feats = prompt1.repeat(B, 1), feats1.repeat(B, 1, 1)
    ms = {r: [] for r in routes}
    for r in routes:
        for _ in range(3):  # first sighting, capture, replay
            run(r, T + 1, prompt, feats); run(r, 1, prompt, feats)
    for _ in range(args.reps):
        for r in routes:
            ms[r].append((run(r, T + 1, prompt, feats) - run(r, 1, prompt, feats)) / T * 1e3)
    model.check_device_errors()
    med = {r: statistics.median(ms[r]) for r in ms}
    row = {r: stat(ms[r]) for r in ms}
    row["spread_max_minus_min"] = {r: round(max(ms[r]) - min(ms[r]), 4) for r in ms}
    row["b_minus_a"], row["c_minus_b"] = round(med["b"] - med["a"], 4), round(med["c"] - med["b"], 4)
    result["decode_ms_per_step"][f"B={B}"] = row
    print(f"B={B}: " + "  ".join(f"({r}) {med[r]:.4f}" for r in ms), flush=True)
    save()

# (d) the launch alone
result["launch_alone_us"] = {}
table = ops.stop_table_words(NEVER).cuda()
for B in [int(b) for b in args.batches.split(",")]:
    g = torch.Generator().manual_seed(B)
    out_ids = torch.randint(3, 1000, (B, 128), generator=g).cuda()
    step = torch.full((B,), 100, dtype=torch.int32, device="cuda")
    fin = torch.zeros(B, dtype=torch.int32, device="cuda")
    result["launch_alone_us"][f"B={B}"] = {"dl_decode_stop": round(bench.graph_time_ms(lambda: ops.decode_stop(out_ids, step, fin, table)) * 1e3, 2)}
    assert int(fin.sum()) == 0
    print(f"B={B} launch alone (us): {result['launch_alone_us'][f'B={B}']}", flush=True)

print(json.dumps(result))
save()
