#!/usr/bin/env python
"""n sampled answers per prompt from one prefill: generate(do_sample=True, seed=, num_return_sequences=n) against the two ways there were before, on the 7B-shaped
random-init model of tools/bench_sampling.py (bf16, the configs[1] prompt of bench.py, 64 new tokens).  For n in --ns, three requests:
  fork        the forked request: one prefill at B = 1, dl_kv_fork into n decode rows;
  repeat      the same prompt and image n times in the batch, same seed (the parent commit runs this one: the baseline);
  sequential  n one-row calls, one after the other.
fork and repeat are alternated inside one phase (they share the n-row decode state and its graphs); sequential runs in a phase of its own, because a one-row call
replaces that state.  Per request: time to first token (record_timing's prefill event), ms per decode step, total wall time; median and (min .. max) over --reps.
Then dl_kv_fork alone, `--launches` times back to back inside one captured graph, on caches of the model's shape at the lengths the prompt leaves: us per launch
and (1 + n) x live bytes / time."""
import argparse, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--ns", type=int, nargs="*", default=[2, 4, 8, 16])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--new-tokens", type=int, default=64)
ap.add_argument("--launches", type=int, default=20)
args = ap.parse_args()

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamic_llava_amd import hip_ops as ops
from dynamic_llava_amd.builder import build_random_model
from dynamic_llava_amd.config import DynamicLlavaConfig
import bench


def _stat(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}


cfg = DynamicLlavaConfig(num_hidden_layers=args.layers)
model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
prompt, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
model.record_timing = True
SAMPLED = dict(do_sample=True, seed=1234, temperature=0.7, top_p=0.9, top_k=50, max_new_tokens=args.new_tokens, eos_token_id=None)


def call(rows, n_return):
    """One generate() -> (time to first token, ms per decode step, total), ms."""
    kw = dict(SAMPLED, num_return_sequences=n_return) if n_return > 1 else SAMPLED
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = model.generate(prompt.expand(rows, -1).contiguous(), images=images.expand(rows, -1, -1, -1).contiguous(), **kw)
    torch.cuda.synchronize(); total = (time.perf_counter() - t0) * 1e3
    assert out.shape == (rows * n_return, args.new_tokens)
    ev = model.last_timing["ev"]
    return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]) / (args.new_tokens - 1), total


REQUESTS = {"fork": lambda n: [call(1, n)], "repeat": lambda n: [call(n, 1)], "sequential": lambda n: [call(1, 1) for _ in range(n)]}


def measure(names, n):
    for name in names:  # warm: first sighting, capture, replay
        for _ in range(3):
            REQUESTS[name](n)
    got = {name: [] for name in names}
    for _ in range(args.reps):  # alternated: every repetition times every request of the phase
        for name in names:
            calls = REQUESTS[name](n)
            got[name].append((calls[0][0], statistics.mean(c[1] for c in calls), sum(c[2] for c in calls)))
    return got


result = {"model": f"7B-shaped random init, {args.layers} layers, bf16", "prompt": "bench.py configs[1]", "new_tokens": args.new_tokens, "reps": args.reps, "rows": [], "kernel": []}
for n in args.ns:
    got = dict(measure(["fork", "repeat"], n), **measure(["sequential"], n))
    for name, xs in got.items():
        row = {"n": n, "request": name, "ttft_ms": _stat([x[0] for x in xs]), "ms_per_step": _stat([x[1] for x in xs]), "total_ms": _stat([x[2] for x in xs])}
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    f, r = got["fork"], got["repeat"]
    spread = lambda xs, i: max(x[i] for x in xs) - min(x[i] for x in xs)
    med = lambda xs, i: statistics.median(x[i] for x in xs)
    verdict = {"n": n, "step_fork_minus_repeat_ms": round(med(f, 1) - med(r, 1), 4), "step_inside_repeat_spread": bool(min(x[1] for x in r) <= med(f, 1) <= max(x[1] for x in r)),
               "ttft_repeat_minus_fork_ms": round(med(r, 0) - med(f, 0), 4), "ttft_gain_exceeds_repeat_spread": bool(med(r, 0) - med(f, 0) > spread(r, 0))}
    result["rows"].append(verdict)
    print(json.dumps(verdict), flush=True)

# ---- dl_kv_fork alone ----
call(1, 1)
lens = model.last_cache.lens.clone()
lens[0] -= args.new_tokens - 1  # what the prefill left: the un-evicted group grew by one slot per decode step; the evicting group's rows are kept as they ended (an upper bound)
lens_host = lens.cpu().tolist()
SL, L, nKV, d = cfg.sparse_config["sparse_layer"], cfg.num_hidden_layers, cfg.num_key_value_heads, cfg.head_dim
live = 2 * nKV * d * 2 * (min(SL, L) * lens_host[0][0] + max(0, L - SL) * lens_host[1][0])
src = model._new_cache(1, 768)
src.slab.normal_()
src.lens.copy_(lens)
for n in args.ns:
    dst = model._new_cache(n, 896)
    fn = lambda: ops.kv_fork(src, dst, n, max_len=max(lens_host[0]))
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
    st = _stat(us[1:])
    row = {"n": n, "lens": [lens_host[0][0], lens_host[1][0]], "live_bytes": live, "us_per_launch": st, "tb_per_s": round((1 + n) * live / (st["median"] * 1e-6) / 1e12, 3), "copy_ceiling_tb_per_s": 6.29}
    result["kernel"].append(row)
    print(json.dumps(row), flush=True)
    del g, dst
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
