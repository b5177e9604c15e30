"""Measured attention error table (docs/attention_error_budget.md): the launches of oracle/attn_cases.py -- the table tests/test_attn_routes_gpu.py
asserts on -- reported instead of asserted.  Per kernel x dtype x distribution: the worst err / tol under the per-element bound of
oracle/attn_truth.py, and the worst error in ULP of the element itself.

    python tools/attn_error_table.py [--skip-decode] > table.md        (needs the GPU)
    python tools/attn_error_table.py --digest [--library other.so] [--sides decode]   SHA-256 of every output of the same tables (prefill, then decode with what each
                                                                       launch appended to the slab or the MXFP8 planes), one line per case:
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


def digests(sides):
    """The launches of the tables with every output tensor hashed instead of judged (the runners hand the tensors back)."""

    def one(label, run, fold=False):
        outs = []
        run(outs)
        hs = [hashlib.sha256(o.view(torch.uint8).numpy().tobytes()).hexdigest() for o in outs]
        if fold:  # a decode case is up to 39 launch forms x 3 tensors: the tensor count and the SHA-256 of their digests, in order
            hs = [str(len(hs)), hashlib.sha256("".join(hs).encode()).hexdigest()]
        print(label, *hs)
        sys.stdout.flush()

    for e in ac.PREFILL_TABLE if "prefill" in sides else ():
        if e.route == "NONE":
            continue
        with ac.pf_env(e.env):
            for dtype in e.dtypes:
                assert ac.prefill_route(ops, e, dtype) == e.route, e.id
                for dist in at.DISTRIBUTIONS:
                    one(f"prefill {e.id} {DT[dtype]} {dist}", lambda outs: ac.run_prefill(ops, e, dist, dtype, outputs=outs))
    with ac.pf_env({}):
        for entry in ac.CACHED_TABLE if "prefill" in sides else ():
            for dtype in ((torch.float32,) if entry[0] == "SIMPLE_F32" else (torch.bfloat16, torch.float16)):
                for dist in at.DISTRIBUTIONS:
                    one(f"cached {entry[0]}-h{entry[1]}kv{entry[2]}d{entry[3]} {DT[dtype]} {dist}", lambda outs: ac.run_cached(ops, entry, dist, dtype, outputs=outs))
    if "decode" not in sides:
        return
    # the decode side: per launch form the output slice and what the launch appended (slab rows, or the four planes' rows)
    for kernel in ("decode", "rope", "parts"):
        for nH, nKV, d in ac.DECODE_HEADS:
            fp32 = kernel != "parts" and (nH, nKV, d) in ((8, 2, 128), (4, 4, 64))  # where tests/test_attn_routes_gpu.py runs it
            for dtype in (torch.bfloat16, torch.float16) + ((torch.float32,) if fp32 else ()):
                for de in ac.DECODE_DISTS:
                    one(f"{kernel} h{nH}kv{nKV}d{d} {DT[dtype]} {de[0]}", lambda outs: ac.run_decode(ops, kernel, de, dtype, nH, nKV, d, outputs=outs), fold=True)
    kv8 = _kv8_cases()
    for nH, nKV, d in ac.DECODE_HEADS:
        for dtype in (torch.bfloat16, torch.float16) + ((torch.float32,) if (nH, nKV, d) == ac.DECODE_HEADS[1] else ()):  # fp32 where the tests run it
            for de in ac.DECODE_DISTS:
                one(f"kv8 h{nH}kv{nKV}d{d} {DT[dtype]} {de[0]}", lambda outs: kv8._run_hard(de, dtype, nH, nKV, d, outputs=outs), fold=True)
    for nH, nKV, d, H in ac.QKV_ATTN_SHAPES:
        for dtype in (torch.bfloat16, torch.float16):
            for T_old in ac.QKV_ATTN_T_OLD:
                for dist in ac.QKV_ATTN_DISTS:
                    one(f"qkv_attn h{nH}kv{nKV}d{d} {DT[dtype]} T_old {T_old} {dist}", lambda outs: ac.run_qkv_attn(ops, dist, dtype, nH, nKV, d, H, T_old, outputs=outs), fold=True)


def _kv8_cases():
    """tests/test_kv8_gpu.py as a module: its hard-input runner over every launch form of dl_attn_decode_rope_kv8"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("test_kv8_gpu", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "test_kv8_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-decode", action="store_true")
    ap.add_argument("--digest", action="store_true", help="print the SHA-256 of every output instead of the error table")
    ap.add_argument("--sides", default="prefill,decode", help="--digest: which families to hash (default: both)")
    ap.add_argument("--library", help="load this build of the library instead of the tree's")
    args = ap.parse_args()
    if args.library:
        ops.load_library(args.library)
    ops.require_gpu()
    if args.digest:
        return digests(args.sides.split(","))
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
