#!/usr/bin/env python
"""MXFP8 KV cache (model.set_kv_cache_format("mxfp8")) against the same tree with the format off: DESIGN.md section 4h's tables.

  attention  the decode attention launch alone -- dl_attn_decode_rope_kv8 against dl_attn_decode_rope, scheduled as the step schedules them (split factor, waves,
             speculative chunk) -- as ONE hipGraph replay of a launch per layer over per-layer slabs (every launch reads cold K/V): us per launch, K/V bytes / time
             as a fraction of the 8 TB/s spec and of the 6.85 TB/s read ceiling.  Shapes: B = 1 x 40 heads x 2048 keys; B = 32 x 32 heads, ragged 200..900 keys;
             B = 32 x 32 heads x 2048 keys.
  decode     decode ms/step (random init, full depth, bf16) at those shapes for the 7B width (13B width: the first), and at B = 1 for a range of context lengths:
             where the mode starts to pay (it gives up the fused q|k|v + attention launch of batch 1).
             Every row carries the slab bytes of both formats for the same request.

Protocol (section 4f's): every shape warmed up on both sides, then the two sides alternately, --reps repetitions each; the minimum and the spread (max - min) of each side.
Writes profiles/kv8_decode_bench.json and prints it.

    python tools/bench_kv8_decode.py [--sections attention,decode] [--shapes NAME,...] [--widths 7b,13b] [--steps 32] [--reps 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dynamic_llava_amd import hip_ops as ops  # noqa: E402
from dynamic_llava_amd.builder import build_random_model  # noqa: E402
from dynamic_llava_amd.cache import KVSlabCache  # noqa: E402
from dynamic_llava_amd.config import DynamicLlavaConfig  # noqa: E402

SPEC_TBS = 8.0
READ_CEILING_TBS = 6.85  # read-only stream ceiling bench.py measured on this box model (BENCH_r06.json measured_ceilings)


def _cfg(width):
    if width == "7b":
        return DynamicLlavaConfig()
    return DynamicLlavaConfig(hidden_size=5120, intermediate_size=13824, num_hidden_layers=40, num_attention_heads=40, num_key_value_heads=40)


def _stats(ts):
    return {"min": round(min(ts), 3), "spread": round(max(ts) - min(ts), 3)}


# ---- the attention launch alone ----
def _attn_graph(fmt, B, nH, d, lens, L, dev):
    """-> (graph of L launches, one per layer's slab; K/V bytes one launch reads)"""
    nKV = nH
    T_cap = -(-(max(lens) + 2) // 128) * 128
    g = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(B, 3 * nH * d, device=dev, generator=g).to(torch.bfloat16)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    emb = torch.outer(torch.arange(T_cap + 8, device=dev, dtype=torch.float32), 1.0 / (10000.0 ** (torch.arange(0, d, 2, device=dev).float() / d)))
    emb = torch.cat((emb, emb), -1)
    cos, sin = emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)
    out = torch.empty(B, nH * d, dtype=torch.bfloat16, device=dev)
    ws = ops.attn_decode_workspace(B, nH, d, 32, dev)
    # the step's schedule (KVSlabCache.n_splits / keys_in_flight / spec_chunk) for rows of these lengths
    cap, want = max(lens) + 1, max(1, 256 // (B * nH))
    ns = 1 if cap <= 256 else max(1, min(32, want, -(-cap // 64)))
    kif, chunk = KVSlabCache.keys_in_flight(ns, B * nH), KVSlabCache.spec_chunk(ns)
    if fmt == "mxfp8":
        codes = torch.randint(0, 0x78, (L, 2, B, nKV, T_cap, d), dtype=torch.uint8, device=dev, generator=g)
        scales = torch.randint(118, 128, (L, 2, B, nKV, T_cap, d // 32), dtype=torch.uint8, device=dev, generator=g)
        fns = [lambda l=l: ops.attn_decode_rope_kv8(qkv, cos, sin, lens_d, lens_d, codes[l, 0], scales[l, 0], codes[l, 1], scales[l, 1], out, ws, ns, nH, nKV, d,
                                                   keys_in_flight=2 * kif, chunk_keys=chunk) for l in range(L)]
        row_bytes = d + d // 32
        keep = (codes, scales)
    else:
        slab = torch.empty((L, 2, B, nKV, T_cap, d), dtype=torch.bfloat16, device=dev)
        for l in range(L):
            slab[l].normal_(generator=g)
        fns = [lambda l=l: ops.attn_decode_rope(qkv, cos, sin, lens_d, lens_d, slab[l, 0], slab[l, 1], out, ws, ns, nH, nKV, d, keys_in_flight=kif, chunk_keys=chunk, call_tag=l & 0xFF)
               for l in range(L)]
        row_bytes = 2 * d
        keep = (slab,)
    for f in fns:
        f()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for f in fns:
            f()
    gr.replay()
    torch.cuda.synchronize()
    return gr, 2 * nKV * row_bytes * sum(lens), dict(n_splits=ns, keys_in_flight=(2 * kif if fmt == "mxfp8" else kif), chunk_keys=chunk), (keep, qkv, lens_d, cos, sin, out, ws)


def _attention_section(reps, dev):
    g = torch.Generator().manual_seed(0)
    shapes = [("B1_h40_T2048", 1, 40, [2048], 40), ("B32_h32_ragged200_900", 32, 32, torch.randint(200, 901, (32,), generator=g).tolist(), 32), ("B32_h32_T2048", 32, 32, [2048] * 32, 32)]
    res = {}
    for name, B, nH, lens, L in shapes:
        sides = {fmt: _attn_graph(fmt, B, nH, 128, lens, L, dev) for fmt in ("bf16", "mxfp8")}
        ts = {fmt: [] for fmt in sides}
        for _ in range(reps):
            for fmt, (gr, _, _, _) in sides.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gr.replay()
                b.record()
                torch.cuda.synchronize()
                ts[fmt].append(a.elapsed_time(b) * 1e3 / L)
        r = {"B": B, "heads": nH, "keys_min": min(lens), "keys_max": max(lens), "layers_in_graph": L}
        for fmt, (_, nbytes, sched, _) in sides.items():
            us = min(ts[fmt])
            r[fmt] = {"us": _stats(ts[fmt]), "kv_bytes": nbytes, "tbs": round(nbytes / us / 1e6, 3), "frac_spec": round(nbytes / us / 1e6 / SPEC_TBS, 3),
                      "frac_read_ceiling": round(nbytes / us / 1e6 / READ_CEILING_TBS, 3), **sched}
        r["speedup"] = round(min(ts["bf16"]) / min(ts["mxfp8"]), 3)
        res[name] = r
        print(json.dumps({name: r}), file=sys.stderr, flush=True)
        del sides
        torch.cuda.empty_cache()
    return res


# ---- decode ms/step through generate() ----
def _prompts(cfg, lens_full, dev):
    """rows whose full KV length after the prefill is lens_full[b] (576 image tokens included); right-padded ids + mask"""
    g = torch.Generator().manual_seed(0)
    n = max(lens_full) - 575
    ids, am = torch.zeros(len(lens_full), n, dtype=torch.long), torch.zeros(len(lens_full), n, dtype=torch.long)
    for b, T in enumerate(lens_full):
        w = T - 575
        row = torch.randint(3, cfg.vocab_size, (w,), generator=g)
        row[0], row[min(8, w - 1)] = 1, -200
        ids[b, :w], am[b, :w] = row, 1
    return ids.to(dev), am.to(dev)


def _decode_ms(model, ids, am, feats, steps):
    model.record_timing = True
    model.generate(ids, attention_mask=None if bool(am.all()) else am, image_features=feats, max_new_tokens=steps + 1, eos_token_id=None)
    torch.cuda.synchronize()
    tm = model.last_timing
    return tm["ev"][1].elapsed_time(tm["ev"][2]) / steps


def _decode_section(widths, steps, reps, dev, only=None):
    res = {}
    g = torch.Generator().manual_seed(0)
    ragged = torch.randint(200, 901, (32,), generator=g).tolist()
    for width in widths:
        cfg = _cfg(width)
        models = {"bf16": build_random_model(cfg, dtype=torch.bfloat16, device=dev, seed=0, predictor_gain=50.0),
                  "mxfp8": build_random_model(cfg, dtype=torch.bfloat16, device=dev, seed=0, predictor_gain=50.0).set_kv_cache_format("mxfp8")}
        shapes = [("B1_T704", [704]), ("B1_T1024", [1024]), ("B1_T2048", [2048]), ("B1_T3584", [3584])]
        if width == "7b":
            shapes += [("B32_T704", [704] * 32), ("B2_T2048", [2048] * 2), ("B8_T2048", [2048] * 8), ("B32_ragged200_900", [n + 576 for n in ragged]), ("B32_T2048", [2048] * 32)]
        r = {}
        for name, lens in shapes:
            if only and name not in only:
                continue
            ids, am = _prompts(cfg, lens, dev)
            feats = torch.randn(len(lens), 576, cfg.hidden_size, device=dev, generator=torch.Generator(device=dev).manual_seed(0)).to(torch.bfloat16)
            for m in models.values():  # every shape warmed up on both sides: first sighting (eager), capture, replay
                for _ in range(3):
                    _decode_ms(m, ids, am, feats, steps)
            ts = {k: [] for k in models}
            for _ in range(reps):
                for k, m in models.items():
                    ts[k].append(_decode_ms(m, ids, am, feats, steps))
            b, c = ts["bf16"], ts["mxfp8"]
            spread = max(max(b) - min(b), max(c) - min(c))
            r[name] = {"bf16_ms": _stats(b), "mxfp8_ms": _stats(c), "speedup": round(min(b) / min(c), 4), "faster": bool(min(b) - min(c) > spread), "slower": bool(min(c) - min(b) > spread),
                       "slab_bytes_bf16": models["bf16"].last_cache.nbytes(), "slab_bytes_mxfp8": models["mxfp8"].last_cache.nbytes()}
            assert models["mxfp8"].last_cache.kv_format == "mxfp8" and models["bf16"].last_cache.kv_format is None
            print(json.dumps({width: {name: r[name]}}), file=sys.stderr, flush=True)
        res[width] = r
        del models
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="attention,decode")
    ap.add_argument("--widths", default="7b,13b")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="", help="decode section: only these shapes (comma-separated names, e.g. B32_ragged200_900)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv8_decode_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"tool": "bench_kv8_decode", "device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "steps": a.steps, "reps": a.reps, "spec_tbs": SPEC_TBS,
           "read_ceiling_tbs": READ_CEILING_TBS}
    if os.path.exists(a.out):  # sections measured by an earlier call are kept
        with open(a.out) as f:
            res = {**json.load(f), **res}
    secs = a.sections.split(",")
    if "attention" in secs:
        res["attention_launch"] = _attention_section(a.reps, dev)
    if "decode" in secs:
        res["decode_ms_per_step"] = {**res.get("decode_ms_per_step", {}), **_decode_section(a.widths.split(","), a.steps, a.reps, dev, [x for x in a.shapes.split(",") if x])}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
