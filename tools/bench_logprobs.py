#!/usr/bin/env python
"""Log-probabilities of generated tokens, decode ms per step, on the 7B-shaped random-init model of bench.py (BASELINE configs[1] prompt: 631 tokens, bf16) at
B = 1 and B = 32 rows with 64 new tokens:
  (a)  plain greedy generate(), in a block of its own: nothing but graph replays on the pooled KV slab;
  (a') the same with return_dict_in_generate=True: the caller keeps the cache, so every such call takes a fresh slab, runs its prefill eagerly and captures
       its decode graphs again -- what every route below also pays (a plain call that follows such a call pays it too, hence (a)'s own block);
  (b)  the only way to the numbers without the keyword: output_scores=True, then log_softmax / gather / top-k (8) on the returned [B, V] tensors;
  (c)  output_logprobs=True;  (d)  output_logprobs=True, top_logprobs=8  (dl_decode_logprobs inside the decode graphs);
  (e)  the launch alone: dl_decode_logprobs (n = 0, n = 8) beside dl_decode_score on the same [B, 32000] bf16 logits (bench.graph_time_ms: launches captured
       into one graph, so the figure includes the dependent-launch gap).
ms/step = (time with 65 tokens - time with 1 token) / 64, host clock around calls that end in a device synchronise; every route is warmed 3 times, then repeated
`--reps` (>= 10) times, (a') (b) (c) (d) alternating inside each repetition; min / median / max reported.  On a commit without the keyword (knobs() has no
device_logprobs) only (a), (a') and (b) run.
    python tools/bench_logprobs.py [--out profiles/logprobs_decode_bench.json] [--reps 10] [--layers 32] [--batches 1,32]"""
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
    sys.exit("bench_logprobs.py measures on the GPU: no HIP device visible")

T, N_TOP = 64, 8
cfg = DynamicLlavaConfig(num_hidden_layers=args.layers)
model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
prompt1, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
calib = bench.calibrate_text_predictor(model, prompt1, images, T)
feats1 = model.encode_images(images)
have = bool(model.knobs().get("device_logprobs", False))
routes = ("a_dict", "b") + (("c", "d") if have else ())  # the alternated block; (a) runs before it
KW = {"a": {}, "a_dict": dict(return_dict_in_generate=True), "b": dict(return_dict_in_generate=True, output_scores=True),
      "c": dict(return_dict_in_generate=True, output_logprobs=True), "d": dict(return_dict_in_generate=True, output_logprobs=True, top_logprobs=N_TOP)}


def run(route, n, prompt, feats):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = model.generate(prompt, image_features=feats, max_new_tokens=n, eos_token_id=None, **KW[route])
    if route == "b":  # what a caller has to do with the [B, V] tensors to get the same numbers
        lsm = torch.log_softmax(torch.stack(res["scores"], dim=1).float(), dim=-1)
        lp = lsm.gather(-1, res["sequences"][..., None])[..., 0]
        top = lsm.topk(N_TOP, dim=-1)
        sink = lp.sum() + top.values.sum() + top.indices.sum()
    elif route in ("c", "d"):
        sink = res["logprobs"].sum() + (res["top_logprobs"].sum() + res["top_logprob_ids"].sum() if route == "d" else 0)
    else:
        sink = (res["sequences"] if route == "a_dict" else res).sum()
    sink.item()
    torch.cuda.synchronize(); return time.perf_counter() - t0


def save():  # (after every stage: a run that is cut short leaves what it measured)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


stat = lambda xs: {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}
result = {"model": f"7B-shaped random init, {args.layers} layers, bf16, prompt 631 tokens (BASELINE configs[1]), {T} new tokens", "text_predictor_calibrated_keep_fraction": calib,
          "method": f"ms/step = (t(65 tokens) - t(1 token)) / 64; {args.reps} repetitions after 3 warm-ups; (a) in a block of its own, the others alternated inside a repetition", "device_logprobs": have, "decode_ms_per_step": {}}
for B in [int(b) for b in args.batches.split(",")]:
    prompt, feats = prompt1.repeat(B, 1), feats1.repeat(B, 1, 1)
    ms = {r: [] for r in ("a",) + routes}
    for i in range(3 + args.reps):  # (a) alone; the first three are the warm-up: first sighting, capture, replay
        d = (run("a", T + 1, prompt, feats) - run("a", 1, prompt, feats)) / T * 1e3
        if i >= 3:
            ms["a"].append(d)
    for r in routes:
        for _ in range(3):
            run(r, T + 1, prompt, feats); run(r, 1, prompt, feats)
    for _ in range(args.reps):
        for r in routes:
            ms[r].append((run(r, T + 1, prompt, feats) - run(r, 1, prompt, feats)) / T * 1e3)
    model.check_device_errors()
    med = {r: statistics.median(ms[r]) for r in ms}
    row = {r: stat(ms[r]) for r in ms}
    row["spread_max_minus_min"] = {r: round(max(ms[r]) - min(ms[r]), 4) for r in ms}
    if have:
        for r in ("c", "d"):
            row[f"{r}_minus_a"] = round(med[r] - med["a"], 4)
            row[f"{r}_minus_a_dict"] = round(med[r] - med["a_dict"], 4)
            row[f"b_minus_{r}"] = round(med["b"] - med[r], 4)
            row[f"{r}_below_b_by_more_than_the_spreads"] = bool(med["b"] - med[r] > max(row["spread_max_minus_min"]["b"], row["spread_max_minus_min"][r]))
    result["decode_ms_per_step"][f"B={B}"] = row
    print(f"B={B}: " + "  ".join(f"({r}) {med[r]:.4f}" for r in ms), flush=True)
    save()

# (e) the launches alone on the same logits: both read the same bytes
result["launch_alone_us"] = {}
for B in [int(b) for b in args.batches.split(",")]:
    g = torch.Generator().manual_seed(B)
    logits = (torch.randn((B, cfg.vocab_size), generator=g) * 4).to(torch.bfloat16).cuda()
    ids, cap = torch.randint(3, cfg.vocab_size, (B,), generator=g).cuda(), 4
    labels = ids[:, None].repeat(1, cap).contiguous()
    nll = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    zero, one = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.ones(B, dtype=torch.int32, device="cuda")
    nxt = torch.zeros(B, dtype=torch.int64, device="cuda")
    row = {"dl_decode_score": round(bench.graph_time_ms(lambda: ops.decode_score(logits, nxt, labels, nll, None, None, zero)) * 1e3, 2)}  # (no out_ids: the step stays at slot 0)
    if have:
        lp = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
        top_lp = torch.zeros((B, cap, N_TOP), dtype=torch.float32, device="cuda")
        top_ids = torch.zeros((B, cap, N_TOP), dtype=torch.int64, device="cuda")
        for n in (0, N_TOP):
            row[f"dl_decode_logprobs_n{n}"] = round(bench.graph_time_ms(lambda: ops.decode_logprobs(logits, ids, one, lp, n, top_lp, top_ids)) * 1e3, 2)
    result["launch_alone_us"][f"B={B}"] = row
    print(f"B={B} launch alone (us): {row}", flush=True)

print(json.dumps(result))
save()
