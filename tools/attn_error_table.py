"""Measured attention error table (docs/attention_error_budget.md): the launches of oracle/attn_cases.py -- the table tests/test_attn_routes_gpu.py
asserts on -- reported instead of asserted.  Per kernel x dtype x distribution: the worst err / tol under the per-element bound of
oracle/attn_truth.py, and the worst error in ULP of the element itself.

    python tools/attn_error_table.py [--skip-decode] > table.md        (needs the GPU)
    python tools/attn_error_table.py --digest [--library other.so]     SHA-256 of every prefill output of the same tables, one line per launch:
                                                                       run it on two builds and diff the listings (same bits or not)"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynamic_llava_amd import hip_ops as ops  # noqa: E402
from oracle import attn_cases as ac  # noqa: E402
from oracle import attn_truth as at  # noqa: E402

DT = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


def _merge(acc, key, r, ulps):
    old = acc.get(key, (0.0, 0.0))
    acc[key] = (max(old[0], r), max(old[1], ulps))


def _print(title, acc, dists):
    print(f"\n### {title}\n")
    print("| kernel | dtype | " + " | ".join(dists) + " |")
    print("|---|---|" + "---|" * len(dists))
    for kern, dt in sorted({(k[0], k[1]) for k in acc}):
        cells = [f"{acc[(kern, dt, d)][0]:.2f} ({acc[(kern, dt, d)][1]:.3g})" if (kern, dt, d) in acc else "-" for d in dists]
        print(f"| {kern} | {dt} | " + " | ".join(cells) + " |")
    sys.stdout.flush()


def digests():
    """The prefill launches of the two tables with every output tensor hashed instead of judged (ac.run_prefill / ac.run_cached hand the tensors back)."""

    def one(label, run):
        outs = []
        run(outs)
        print(label, *(hashlib.sha256(o.view(torch.uint8).numpy().tobytes()).hexdigest() for o in outs))
        sys.stdout.flush()

    for e in ac.PREFILL_TABLE:
        if e.route == "NONE":
            continue
        with ac.pf_env(e.env):
            for dtype in e.dtypes:
                assert ac.prefill_route(ops, e, dtype) == e.route, e.id
                for dist in at.DISTRIBUTIONS:
                    one(f"prefill {e.id} {DT[dtype]} {dist}", lambda outs: ac.run_prefill(ops, e, dist, dtype, outputs=outs))
    with ac.pf_env({}):
        for entry in ac.CACHED_TABLE:
            for dtype in ((torch.float32,) if entry[0] == "SIMPLE_F32" else (torch.bfloat16, torch.float16)):
                for dist in at.DISTRIBUTIONS:
                    one(f"cached {entry[0]}-h{entry[1]}kv{entry[2]}d{entry[3]} {DT[dtype]} {dist}", lambda outs: ac.run_cached(ops, entry, dist, dtype, outputs=outs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--digest", action="store_true", help="print the SHA-256 of every prefill output instead of the error table")
    ap.add_argument("--library", help="load this build of the library instead of the tree's")
    args = ap.parse_args()
    if args.library:
        ops.load_library(args.library)
    ops.require_gpu()
    if args.digest:
        return digests()
    print("Each cell: worst err / tol (worst error in ULP of the element).")
    acc = {}
    for e in ac.PREFILL_TABLE:
        if e.route == "NONE":
            continue
        with ac.pf_env(e.env):
            for dtype in e.dtypes:
                assert ac.prefill_route(ops, e, dtype) == e.route, e.id
                for dist in at.DISTRIBUTIONS:
                    r, ulps, _ = ac.run_prefill(ops, e, dist, dtype)
                    _merge(acc, (e.route, DT[dtype], dist), r, ulps)
    _print("dl_attn_prefill, by route", acc, at.DISTRIBUTIONS)
    acc = {}
    with ac.pf_env({}):
        for entry in ac.CACHED_TABLE:
            for dtype in ((torch.float32,) if entry[0] == "SIMPLE_F32" else (torch.bfloat16, torch.float16)):
                for dist in at.DISTRIBUTIONS:
                    r, ulps, _ = ac.run_cached(ops, entry, dist, dtype)
                    _merge(acc, (f"{entry[0]} d{entry[3]}", DT[dtype], dist), r, ulps)
    _print("dl_attn_prefill_cached (kv_len 0, 37, 200, 4000), by route", acc, at.DISTRIBUTIONS)
    acc = {}
    for nH, nKV, d, H in ac.QKV_ATTN_SHAPES:
        for dtype in (torch.bfloat16, torch.float16):
            for T_old in ac.QKV_ATTN_T_OLD:
                for dist in ac.QKV_ATTN_DISTS:
                    for ns, w in ac.run_qkv_attn(ops, dist, dtype, nH, nKV, d, H, T_old).items():
                        _merge(acc, (f"d{d} n_splits {ns}" if ns != "two launches" else f"d{d} (dl_gemv + dl_attn_decode_rope)", DT[dtype], dist), w[0], w[1])
    _print("dl_gemv_qkv_attn", acc, ac.QKV_ATTN_DISTS)
    if args.skip_decode:
        return
    acc = {}
    names = [x[0] for x in ac.DECODE_DISTS]
    for kernel in ("decode", "rope", "parts"):
        for nH, nKV, d in ac.DECODE_HEADS:
            for dtype in (torch.bfloat16, torch.float16):
                for de in ac.DECODE_DISTS:
                    for launch, w in ac.run_decode(ops, kernel, de, dtype, nH, nKV, d).items():
                        form = {"decode": "dl_attn_decode", "rope": f"dl_attn_decode_rope kif {launch[1]}", "parts": "dl_attn_decode_rope_parts"}[kernel]
                        _merge(acc, (f"{form} d{d}", DT[dtype], de[0]), w[0], w[1])
    _print("decode (worst over n_splits, chunk_keys, call_tag, head layouts)", acc, names)


if __name__ == "__main__":
    main()
