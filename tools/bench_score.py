#!/usr/bin/env python
"""Teacher-forced scoring, ms per token: (a) greedy generate() (dl_decode_advance in the graph), (b) model.score() on 64 labels (dl_decode_score in the same
graph), (c) the route that was the only one before -- a forward() loop with an fp32 copy of the logits, F.cross_entropy and a host read per token -- alternated
inside one process on the 7B-shaped random-init model of the other tools/bench_*, BASELINE configs[1] shapes (631-token prompt, B = 1, T = 64).
ms/token = (time with 65 tokens - time with 1 token) / 64; every route is warmed 3 times, then repeated `--reps` (>= 10) times with the three routes alternating
inside each repetition; min / median / max reported -- the spread of (a) is what "(b) ~ (a)" is judged against.  The two bookkeeping launches are also timed
alone on the step's own logits buffer (bench.graph_time_ms: launches captured into one graph, so the figure includes the dependent-launch gap).
    python tools/bench_score.py [--out profiles/r07_score_vs_forward_loop.txt] [--reps 10] [--layers 32]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from dynamic_llava_amd import hip_ops as ops
from dynamic_llava_amd.builder import build_random_model
from dynamic_llava_amd.config import DynamicLlavaConfig
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--layers", type=int, default=32)
args = ap.parse_args()
assert args.reps >= 10, "at least 10 timed repetitions"

T = 64
cfg = DynamicLlavaConfig(num_hidden_layers=args.layers)
model = build_random_model(cfg, dtype=torch.bfloat16, device="cuda", seed=0, predictor_gain=50.0)
prompt, images = bench.make_inputs(cfg, torch.device("cuda"), torch.bfloat16)
feats = model.encode_images(images)
labels_all = torch.randint(3, cfg.vocab_size, (1, T + 1), generator=torch.Generator().manual_seed(5))


def run(route, n):
    lab = labels_all[:, :n].contiguous()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    if route == "generate":
        model.generate(prompt, image_features=feats, max_new_tokens=n, eos_token_id=None)
    elif route == "score":
        model.score(prompt, lab, image_features=feats)["nll"].sum().item()
    else:  # the forward() loop: logits of the last position -> fp32 -> cross-entropy on the host side of every step
        out = model(prompt, image_features=feats)
        pkv, total = out.past_key_values, 0.0
        for j in range(n):
            total += F.cross_entropy(out.logits[:, -1].float(), lab[:, j].cuda()).item()
            if j + 1 < n:
                out = model(lab[:, j : j + 1].cuda(), past_key_values=pkv)
                pkv = out.past_key_values
    torch.cuda.synchronize(); return time.perf_counter() - t0


routes = ("generate", "score", "loop")
for r in routes:  # warm: first sighting, capture, replay
    for _ in range(3):
        run(r, T + 1); run(r, 1)
ms = {r: [] for r in routes}
for _ in range(args.reps):  # alternated: every repetition times all three
    for r in routes:
        ms[r].append((run(r, T + 1) - run(r, 1)) / T * 1e3)

# the two bookkeeping launches alone, on the step's logits buffer (V = 32000, bf16, one row)
st = model._dstate
st.labels[:, :T].copy_(labels_all[:, :T])


def adv():
    st.step.zero_(); st.finished.zero_()
    ops.decode_advance(st.logits, st.cur_ids, st.out_ids, st.step, st.finished, -1, 0, None, None, None)


def scr():
    st.step.zero_(); st.finished.zero_()
    ops.decode_score(st.logits, st.cur_ids, st.labels, st.nll, st.top1, st.out_ids, st.step, st.finished, 0, None, None, None)


def rst():
    st.step.zero_(); st.finished.zero_()


t_rst = bench.graph_time_ms(rst) * 1e3
t_adv, t_scr = bench.graph_time_ms(adv) * 1e3 - t_rst, bench.graph_time_ms(scr) * 1e3 - t_rst

f = lambda xs: f"min {min(xs):.4f}  median {statistics.median(xs):.4f}  max {max(xs):.4f}"
med = {r: statistics.median(ms[r]) for r in routes}
spread_a = max(ms["generate"]) - min(ms["generate"])
lines = [
    f"model: 7B-shaped random init, {args.layers} layers, bf16, B = 1, prompt 631 tokens (configs[1]), T = {T}; {args.reps} repetitions after 3 warm-ups, routes alternated",
    f"(a) generate(max_new_tokens=64) greedy      ms/token: {f(ms['generate'])}",
    f"(b) score() on 64 labels                    ms/token: {f(ms['score'])}",
    f"(c) forward() loop + F.cross_entropy        ms/token: {f(ms['loop'])}",
    f"(b)/(a) = {med['score'] / med['generate']:.4f}   (b)-(a) = {med['score'] - med['generate']:+.4f} ms   spread of (a) (max - min) = {spread_a:.4f} ms   "
    f"(b) within (a)'s spread: {abs(med['score'] - med['generate']) <= spread_a}",
    f"(c)/(b) = {med['loop'] / med['score']:.3f}",
    f"bookkeeping launch alone (captured, dependent-launch gap included): dl_decode_advance {t_adv:.2f} us, dl_decode_score {t_scr:.2f} us",
]
print("\n".join(lines))
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
