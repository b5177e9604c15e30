#!/usr/bin/env python
"""Constrained decoding, decode ms per step, on the 7B-shaped random-init model of bench.py (BASELINE configs[1] prompt: 631 tokens, bf16) at B = 1 and B = 32
rows with 64 new tokens, five requests alternated inside each repetition:
  (a)  the plain greedy generate();
  (b)  guided_choice: two answers of 80 tokens that share their first 8 (a trie of 153 states; max_new_tokens cuts the rows off inside it, so every step is
       constrained): dl_logits_constrain in front of every step-closing launch, which then reads fp32 rows;
  (c)  repetition_penalty = 1.3 alone (dl_logits_process: the launch this one is expected to cost about as much as);
  (d)  (b) with repetition_penalty = 1.3: both launches, the second one in place;
  (e)  allowed_token_ids: a whitelist of all 32000 ids (one state with 32000 edges: every tile's mask is full).
  (f)  the launches alone: dl_logits_constrain on [B, 32000] bf16 logits in the states of (b) and of (e), and in place on fp32 (bench.graph_time_ms: launches
       captured into one graph, so the figure includes the dependent-launch gap).
`--plain-only` measures (a) and (c) only: the form that also runs on a commit without the keywords, for the comparison with the parent commit.
ms/step = (time with 65 tokens - time with 1 token) / 64, host clock around calls that end in a device synchronise; every request is warmed 3 times, then repeated
`--reps` (>= 10) times; min / median / max reported.
    python tools/bench_constrain.py [--out profiles/constrain_decode_bench.json] [--reps 10] [--layers 32] [--batches 1,32] [--plain-only]"""
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
ap.add_argument("--plain-only", action="store_true")
args = ap.parse_args()
assert args.reps >= 10, "at least 10 timed repetitions"
if not torch.cuda.is_available():
    sys.exit("bench_constrain.py measures on the GPU: no HIP device visible")

T = 64
cfg = DynamicLlavaConfig(num_hidden_layers=args.layers)
model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
prompt1, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
calib = bench.calibrate_text_predictor(model, prompt1, images, T)
feats1 = model.encode_images(images)
V = cfg.vocab_size
g = torch.Generator().manual_seed(0)
head, tails = torch.randint(3, V, (8,), generator=g).tolist(), [torch.randint(3, V, (72,), generator=g).tolist() for _ in range(2)]
tails[1][0] = tails[0][0] + 1 if tails[0][0] + 1 < V else 3  # the two answers part at token 8
CHOICES = [head + t for t in tails]
KW = {"a": dict(), "c": dict(repetition_penalty=1.3)}
if not args.plain_only:
    KW.update({"b": dict(guided_choice=CHOICES), "d": dict(guided_choice=CHOICES, repetition_penalty=1.3), "e": None})  # (e): made per batch, once the EOS id is known
routes = tuple(sorted(KW))
EOS = None  # chosen per batch below: an id no request emits, so that every request has an EOS id -- the decode loop then observes the rows' flags in all of them alike -- and no row ends


def run(route, n, prompt, feats):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = model.generate(prompt, image_features=feats, max_new_tokens=n, eos_token_id=EOS, **KW[route])
    assert res.shape[1] == n  # (no row finished)
    res.sum().item()
    torch.cuda.synchronize(); return time.perf_counter() - t0


def save():  # (after every stage: a run that is cut short leaves what it measured)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


stat = lambda xs: {"min": round(min(xs), 4), "median": round(statistics.median(xs), 4), "max": round(max(xs), 4)}
result = {"model": f"7B-shaped random init, {args.layers} layers, bf16, prompt 631 tokens (BASELINE configs[1]), {T} new tokens", "text_predictor_calibrated_keep_fraction": calib,
          "method": f"ms/step = (t(65 tokens) - t(1 token)) / 64; {args.reps} repetitions after 3 warm-ups, the requests alternated inside a repetition",
          "requests": {"a": "plain", "b": "guided_choice, two answers of 80 tokens", "c": "repetition_penalty 1.3", "d": "b + repetition_penalty 1.3", "e": f"allowed_token_ids, all {V} ids (the EOS id through its edge)",
                       "all": "eos_token_id = an id that no request emits"},
          "decode_ms_per_step": {}}
for B in [int(b) for b in args.batches.split(",")]:
    prompt, feats = prompt1.repeat(B, 1), feats1.repeat(B, 1, 1)
    used = {t for c in CHOICES for t in c}
    for r in ("a", "c"):
        used |= set(model.generate(prompt, image_features=feats, max_new_tokens=T + 1, eos_token_id=None, **KW[r]).reshape(-1).tolist())
    EOS = next(v for v in range(1000, V) if v not in used)
    if not args.plain_only:
        KW["e"] = dict(allowed_token_ids=[v for v in range(V) if v != EOS])  # with the EOS edge of its one accepting state: every id is allowed, the tokens are (a)'s
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
    row["c_minus_a"] = round(med["c"] - med["a"], 4)
    if not args.plain_only:
        row["b_minus_a"], row["d_minus_c"], row["e_minus_a"] = round(med["b"] - med["a"], 4), round(med["d"] - med["c"], 4), round(med["e"] - med["a"], 4)
    result["decode_ms_per_step"][f"B={B}"] = row
    print(f"B={B}: " + "  ".join(f"({r}) {med[r]:.4f}" for r in ms), flush=True)
    save()

# (f) the launches alone
if not args.plain_only:
    from dynamic_llava_amd import constraints

    result["launch_alone_us"] = {}
    tables = {"guided_choice": constraints.compile(constraints.TokenAutomaton.from_choices(CHOICES), (2,)), "allowed_all": constraints.compile(constraints.TokenAutomaton.from_allowed(list(range(V))), ())}
    for B in [int(b) for b in args.batches.split(",")]:
        gen = torch.Generator().manual_seed(B)
        x = (torch.randn(B, V, generator=gen) * 4).bfloat16().cuda()
        xf, out = x.float(), torch.empty((B, V), dtype=torch.float32, device="cuda")
        out_ids = torch.zeros((B, 128), dtype=torch.int64, device="cuda")
        step = torch.zeros(B, dtype=torch.int32, device="cuda")
        start, hist = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.full((B, 129), -1, dtype=torch.int32, device="cuda")
        row = {}
        for name, t in tables.items():
            tab = ops.constraint_table_write(ops.constraint_table_block("cuda"), *t.words())
            row[f"dl_logits_constrain[{name}]"] = round(bench.graph_time_ms(lambda: ops.logits_constrain(x, out, tab, start, hist, out_ids, step)) * 1e3, 2)
            row[f"dl_logits_constrain[{name}, fp32 in place]"] = round(bench.graph_time_ms(lambda: ops.logits_constrain(xf, xf, tab, start, hist, out_ids, step)) * 1e3, 2)
        prm, words = ops.logits_params_block("cuda"), ops.bad_words_table((), "cuda")
        prm.copy_(ops.logits_params_words(1.3, 0, 0))
        row["dl_logits_process[penalty]"] = round(bench.graph_time_ms(lambda: ops.logits_process(x, out, prm, out_ids, step, words)) * 1e3, 2)
        result["launch_alone_us"][f"B={B}"] = row
        print(f"B={B} launches alone (us): {row}", flush=True)

print(json.dumps(result))
save()
