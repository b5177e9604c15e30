#!/usr/bin/env python
"""Guided decoding on paired rows: generate(guidance_scale=, negative_prompt_ids=) against what there was before, on the 7B-shaped random-init model of
tools/bench_sampling.py (bf16, the configs[1] prompt of bench.py, 64 new tokens, greedy).  For B in --batches, four requests, alternated inside one repetition:
  guided     B prompts, each with a text-only negative prompt (the prompt without its image placeholder): two prefills of B rows, decode at 2 B rows;
  plain_2b   the plain request of 2 B rows (what the added launches are measured against);
  plain_b    the plain request of B rows (two separate streams would cost two of these steps);
  plain_neg  the plain request of the B text-only negative prompts (the second of the two prefills a two-stream implementation pays for).
Per request: time to first token (record_timing's prefill event), ms per decode step, total wall time; median and (min .. max) over --reps.
--plain-only runs the three plain requests alone: the form that also runs on a commit without the keywords (alternate it with this commit on one box).
Then the new launches alone, `--launches` times back to back inside one captured graph: dl_logits_guide and dl_pair_follow at [2 B, V] bf16 logits, and
dl_kv_place beside dl_kv_fork at n = 1 on caches of the model's shape at the lengths the prompt leaves (us per launch, 2 x live bytes / time)."""
import argparse, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 16])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--new-tokens", type=int, default=64)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--scale", type=float, default=2.0)
ap.add_argument("--plain-only", action="store_true")
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamic_llava_amd import hip_ops as ops
from dynamic_llava_amd.builder import build_random_model
from dynamic_llava_amd.config import IMAGE_TOKEN_INDEX, DynamicLlavaConfig
import bench


def _stat(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}


cfg = DynamicLlavaConfig(num_hidden_layers=args.layers)
model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
prompt, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
negative = prompt[:, prompt[0] != IMAGE_TOKEN_INDEX].contiguous()  # the same text without the image: the language prior
model.record_timing = True
GREEDY = dict(max_new_tokens=args.new_tokens, eos_token_id=None)


def call(ids, rows, imgs=True, **more):
    """One generate() -> (time to first token, ms per decode step, total), ms."""
    kw = dict(GREEDY, **more)
    if imgs:
        kw["images"] = images.expand(rows, -1, -1, -1).contiguous()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = model.generate(ids.expand(rows, -1).contiguous(), **kw)
    torch.cuda.synchronize(); total = (time.perf_counter() - t0) * 1e3
    assert out.shape[1] == args.new_tokens
    ev = model.last_timing["ev"]
    return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]) / (args.new_tokens - 1), total


REQUESTS = {"guided": lambda B: call(prompt, B, guidance_scale=args.scale, negative_prompt_ids=negative), "plain_2b": lambda B: call(prompt, 2 * B),
            "plain_b": lambda B: call(prompt, B), "plain_neg": lambda B: call(negative, B, imgs=False)}
names = [n for n in REQUESTS if not (args.plain_only and n == "guided")]
result = {"model": f"7B-shaped random init, {args.layers} layers, bf16", "prompt": "bench.py configs[1]", "new_tokens": args.new_tokens, "reps": args.reps, "scale": args.scale,
          "rows": [], "kernel": []}
for B in args.batches:
    got = {n: [] for n in names}
    # every request in a phase of its own (requests of another row count replace the decode state and its graphs): warm -- first sighting, capture, replay -- then the repetitions;
    # the phases are run twice over, so that every request is timed early and late in the process
    for half in range(2):
        for n in names:
            for _ in range(3):
                REQUESTS[n](B)
            for _ in range((args.reps + 1 - half) // 2):
                got[n].append(REQUESTS[n](B))
    for n, xs in got.items():
        row = {"B": B, "request": n, "ttft_ms": _stat([x[0] for x in xs]), "ms_per_step": _stat([x[1] for x in xs]), "total_ms": _stat([x[2] for x in xs])}
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    if "guided" in got:
        med = lambda n, i: statistics.median(x[i] for x in got[n])
        spread = lambda n, i: max(x[i] for x in got[n]) - min(x[i] for x in got[n])
        verdict = {"B": B, "step_guided_minus_plain_2b_ms": round(med("guided", 1) - med("plain_2b", 1), 4), "plain_2b_step_spread_ms": round(spread("plain_2b", 1), 4),
                   "step_guided_over_two_plain_b": round(med("guided", 1) / (2 * med("plain_b", 1)), 4),
                   "ttft_guided_minus_two_plain_prefills_ms": round(med("guided", 0) - med("plain_b", 0) - med("plain_neg", 0), 4)}
        result["rows"].append(verdict)
        print(json.dumps(verdict), flush=True)


def timed(fn):
    """fn `--launches` times inside one captured graph -> us per launch over the repetitions."""
    s_ = torch.cuda.Stream(); s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        fn()
    torch.cuda.current_stream().wait_stream(s_)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(args.launches):
            fn()
    us = []
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / args.launches * 1e3)
    return _stat(us[1:])


if not args.plain_only:
    V = cfg.vocab_size
    for B in args.batches:
        logits = (torch.randn((2 * B, V), device="cuda") * 4).to(torch.bfloat16)
        out, params = torch.empty((2 * B, V), dtype=torch.float32, device="cuda"), ops.guide_params_block("cuda")
        params.copy_(ops.guide_params_words(args.scale, 0.1))
        nxt, out_ids = torch.zeros(2 * B, dtype=torch.int64, device="cuda"), torch.zeros((2 * B, args.new_tokens), dtype=torch.int64, device="cuda")
        step, fin = torch.ones(2 * B, dtype=torch.int32, device="cuda"), torch.zeros(2 * B, dtype=torch.int32, device="cuda")
        row = {"B": B, "dl_logits_guide_us": timed(lambda: ops.logits_guide(logits, out, params)), "dl_pair_follow_us": timed(lambda: ops.pair_follow(nxt, out_ids, step, fin))}
        result["kernel"].append(row)
        print(json.dumps(row), flush=True)
    # ---- dl_kv_place beside dl_kv_fork at n = 1 ----
    call(prompt, 1)
    lens = model.last_cache.lens.clone()
    lens[0] -= args.new_tokens - 1  # what the prefill left (bench_fork.py)
    lens_host = lens.cpu().tolist()
    SL, L, nKV, d = cfg.sparse_config["sparse_layer"], cfg.num_hidden_layers, cfg.num_key_value_heads, cfg.head_dim
    live = 2 * nKV * d * 2 * (min(SL, L) * lens_host[0][0] + max(0, L - SL) * lens_host[1][0])
    src = model._new_cache(1, 768)
    src.slab.normal_()
    src.lens.copy_(lens)
    dst1, dst2 = model._new_cache(1, 896), model._new_cache(2, 896)
    maps = ops.kv_place_maps([0], [1], 1, 2, "cuda")
    fork_us = timed(lambda: ops.kv_fork(src, dst1, 1, max_len=max(lens_host[0])))
    place_us = timed(lambda: ops.kv_place(src, dst2, *maps, max_len=max(lens_host[0])))
    tb = lambda st: round(2 * live / (st["median"] * 1e-6) / 1e12, 3)
    row = {"lens": [lens_host[0][0], lens_host[1][0]], "live_bytes": live, "dl_kv_fork_n1_us": fork_us, "dl_kv_fork_n1_tb_per_s": tb(fork_us), "dl_kv_place_us": place_us,
           "dl_kv_place_tb_per_s": tb(place_us)}
    result["kernel"].append(row)
    print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
