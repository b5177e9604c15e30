#!/usr/bin/env python
"""Logits processors in the decode graph, ms per step: generate() with the processors off / repetition penalty only / penalty + no-repeat n-gram +
bad words, greedy and device-sampled (seed=), alternated inside one process on the 7B-shaped random-init model of tools/bench_sampling.py.
B = 1 and B = 32, 64 new tokens.  ms/step = (time of 65 new tokens - time of 1 new token) / 64; every variant is repeated `--reps` times,
min / median / max reported (the spread is what a difference is judged against).

A/B against another build of the project (the parent commit, built in its own checkout): `--tree PATH` imports the package from PATH instead of
this checkout -- a tree without the processors runs the "off" settings only -- and `--merge` combines the `--out` files of alternated runs:
    python tools/bench_logits_process.py --label this --out a1.json;  python tools/bench_logits_process.py --tree ../parent --label parent --out b1.json;  ... (again)
    python tools/bench_logits_process.py --merge a1.json b1.json a2.json b2.json --with-kernels k.json --out profiles/logits_process_decode_bench.json
`--kernels` (no model) times the launches alone: dl_logits_process, and the two bookkeeping kernels on bf16 and on fp32 rows."""
import argparse, json, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--tree", default=None, help="import dynamic_llava_amd (and bench.make_inputs) from this checkout instead of the one this file is in")
ap.add_argument("--label", default="this")
ap.add_argument("--merge", nargs="*", default=None, help="--out files of alternated runs -> one table")
ap.add_argument("--with-kernels", default=None, help="with --merge: the --out file of a --kernels run, stored beside the table")
ap.add_argument("--batches", type=int, nargs="*", default=[1, 32])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--kernels", action="store_true", help="no model: the launches alone, us per launch back to back inside one captured graph (V = 32000)")
args = ap.parse_args()


def _stat(xs):
    return {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}


if args.merge is not None:
    runs = [json.load(open(p)) for p in args.merge]
    pooled = {}  # (label, B, mode, setting) -> every repetition of every run
    for r in runs:
        for row in r["rows"]:
            pooled.setdefault((r["label"], row["B"], row["mode"], row["setting"]), []).extend(row["ms"])
    table = {"model": runs[0]["model"], "new_tokens": 64, "runs": [{"label": r["label"], "reps": r["reps"]} for r in runs], "rows": [], "off_vs_parent": []}
    for (label, B, mode, setting), ms in sorted(pooled.items()):
        row = {"build": label, "B": B, "mode": mode, "setting": setting, "ms_per_step": _stat(ms), "n": len(ms)}
        off = pooled.get((label, B, mode, "off"))
        if setting != "off" and off:
            row["minus_off_ms"] = round(statistics.median(ms) - statistics.median(off), 4)
        table["rows"].append(row)
    for (label, B, mode, setting), ms in sorted(pooled.items()):
        par = pooled.get(("parent", B, mode, "off"))
        if label == "this" and setting == "off" and par:
            d = statistics.median(ms) - statistics.median(par)
            spread = max(par) - min(par)
            table["off_vs_parent"].append({"B": B, "mode": mode, "this_minus_parent_ms": round(d, 4), "parent_spread_ms": round(spread, 4), "inside_parent_spread": bool(abs(d) <= spread)})
    if args.with_kernels:
        table["launches_alone_us"] = json.load(open(args.with_kernels))
    print(json.dumps(table, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamic_llava_amd.builder import build_random_model
from dynamic_llava_amd.config import DynamicLlavaConfig
import bench

if args.kernels:
    # which launch carries the cost: dl_logits_process itself, or the bookkeeping kernel reading fp32 rows instead of the model dtype's
    from dynamic_llava_amd import hip_ops as ops

    V, N, out = 32000, 200, {"V": 32000, "launches_per_graph": 200, "rows": []}
    for B in args.batches:
        x = (torch.randn(B, V, device="cuda") * 3).bfloat16()
        xf, proc = x.float(), torch.empty((B, V), dtype=torch.float32, device="cuda")
        ids = torch.randint(0, V, (B, 64), device="cuda")
        nxt, fin = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        full = torch.full((B,), 40, dtype=torch.int32, device="cuda")  # a history of 40 tokens, never advanced: step is passed to the processors only
        prm, tab = ops.logits_params_block("cuda"), ops.bad_words_table([[5], [17, 29], [101, 7, 9]], "cuda")
        prm.copy_(ops.logits_params_words(1.3, 3, 3))
        sp_ = ops.sample_params_block("cuda")
        sp_.copy_(ops.sample_params_words(0.7, 50, 0.9, 1234, 0))
        cases = {"logits_process": lambda: ops.logits_process(x, proc, prm, ids, full, tab), "advance_bf16": lambda: ops.decode_advance(x, nxt, None, None, fin),
                 "advance_fp32": lambda: ops.decode_advance(xf, nxt, None, None, fin), "sample_bf16": lambda: ops.decode_sample(x, nxt, sp_, None, None, fin),
                 "sample_fp32": lambda: ops.decode_sample(xf, nxt, sp_, None, None, fin)}
        row = {"B": B}
        for name, fn in cases.items():
            s_ = torch.cuda.Stream(); s_.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s_):
                fn()
            torch.cuda.current_stream().wait_stream(s_)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(N):
                    fn()
            us = []
            for _ in range(args.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) / N * 1e3)
            row[name + "_us"] = _stat(us[1:])
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    sys.exit(0)

cfg = DynamicLlavaConfig(num_hidden_layers=args.layers)
model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
prompt, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
feats = model.encode_images(images)
has_proc = bool(model.knobs().get("device_logits_processors", False))
SETTINGS = {"off": {}}
if has_proc:
    SETTINGS["penalty"] = dict(repetition_penalty=1.3)
    SETTINGS["all_three"] = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, bad_words_ids=[[5], [17, 29], [101, 7, 9]] + [[1000 + i, 2000 + i] for i in range(13)])
MODES = {"greedy": {}, "sampled": dict(do_sample=True, seed=1234, temperature=0.7, top_p=0.9, top_k=50)}


def run(B, n_new, mode, setting):
    ids = prompt.expand(B, -1).contiguous()
    f = feats.expand(B, -1, -1).contiguous()
    kw = dict(image_features=f, max_new_tokens=n_new, eos_token_id=None, **MODES[mode], **SETTINGS[setting])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    model.generate(ids, **kw)
    torch.cuda.synchronize(); return time.perf_counter() - t0


result = {"label": args.label, "model": f"7B-shaped random init, {args.layers} layers, bf16", "new_tokens": 64, "reps": args.reps,
          "knobs": {"device_logits_processors": has_proc, "device_sampling": model.knobs().get("device_sampling")}, "rows": []}
for B in args.batches:
    model._dstate = None
    variants = [(m, s) for m in MODES for s in SETTINGS]
    for m, s in variants:  # warm: first sighting, capture, replay
        for _ in range(3):
            run(B, 65, m, s); run(B, 1, m, s)
    ms = {v: [] for v in variants}
    for _ in range(args.reps):  # alternated: every repetition times every variant
        for v in variants:
            ms[v].append((run(B, 65, *v) - run(B, 1, *v)) / 64 * 1e3)
    for (m, s) in variants:
        row = {"B": B, "mode": m, "setting": s, "ms": [round(x, 4) for x in ms[(m, s)]], "ms_per_step": _stat(ms[(m, s)])}
        if s != "off":
            row["minus_off_ms"] = round(statistics.median(ms[(m, s)]) - statistics.median(ms[(m, "off")]), 4)
        result["rows"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "ms"}), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
