#!/usr/bin/env python
"""dl_gemv_qkv_attn (bf16 rows) against dl_gemv_qkv_attn_pk (12-bit packed rows) on the flagship's fused q|k|v + attention launch (7B: N = 12288,
K = 4096): T = 60, 200, 250 with one attention workgroup per head and T = 695 with the split count the product picks (KVSlabCache.fused_attn_splits).
tools/bench_gemv_pk.py's protocol: six distinct weight copies and K/V slabs (nothing comes from the caches), the two launches alternated in one process,
each captured in a graph, the median of five replays.  Beside each row: the bytes the packed launch saves and what they are worth at 6.3 TB/s.

usage: python tools/bench_qkv_attn_pk.py [--lib path/to/libdynllava_hip.so] [T ...]
--lib: measure another build of the library, e.g. one made with HIPCC_EXTRA=-DDL_QA_PK_R=1 (one row per wave in the packed projection; the product runs two)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamic_llava_amd import hip_ops as ops, bf16pack as bp
from oracle.ref_cpu import rope_table

args = sys.argv[1:]
if "--lib" in args:
    i = args.index("--lib")
    ops.load_library(os.path.abspath(args[i + 1]))
    print(f"library: {args[i + 1]}")
    del args[i:i + 2]
dev, dt = "cuda", torch.bfloat16
nH, d, H = 32, 128, 4096
N = 3 * H
NCOPY, REPS = 6, 10
g = torch.Generator(device=dev).manual_seed(N + H)
ws = [(torch.randn(N, H, generator=g, device=dev) * 0.02).to(dt) for _ in range(NCOPY)]
ps = [bp.pack(w) for w in ws]
saved = bp.raw_nbytes(ps[0]) - bp.packed_nbytes(ps[0])
print(f"q|k|v [{N},{H}]: packed / bf16 bytes = {bp.packed_nbytes(ps[0]) / bp.raw_nbytes(ps[0]):.4f}, {saved / 1e6:.1f} MB fewer per launch = {saved / 6.3e6:.2f} us at 6.3 TB/s", flush=True)
nw = torch.ones(H, device=dev, dtype=dt)
h0, delta, ho = torch.randn(1, H, device=dev).to(dt), torch.randn(1, H, device=dev).to(dt), torch.empty(1, H, device=dev, dtype=dt)
gran = ops.gemv_qkv_attn_workspace(nH, nH, d, dev)
err = torch.zeros(1, dtype=torch.int32, device=dev)

for T in ([int(a) for a in args] or [60, 200, 250, 695]):
    ns = 1 if T <= 256 else max(1, min(4, -(-T // 128)))  # KVSlabCache.fused_attn_splits with fused_single_keys = 256
    T_cap = T + 8
    cos, sin = (t.to(dev) for t in rope_table(d, T_cap + 8, 10000.0, dt))
    ks = [torch.randn(1, nH, T_cap, d, device=dev).to(dt) for _ in range(NCOPY)]
    vs = [torch.randn(1, nH, T_cap, d, device=dev).to(dt) for _ in range(NCOPY)]
    lens = torch.tensor([T - 1], dtype=torch.int32, device=dev)
    outs = {k: (torch.empty(1, N, device=dev, dtype=dt), torch.empty(1, H, device=dev, dtype=dt)) for k in ("bf16", "pk")}
    tag = [0]

    def run(label, i):
        tag[0] = (tag[0] + 1) % 251
        fn, wt = (ops.gemv_qkv_attn, ws[i]) if label == "bf16" else (ops.gemv_qkv_attn_pk, ps[i])
        qkv, out = outs[label]
        fn(wt, qkv, h0, ho, delta, nw, 1e-5, cos, sin, lens, lens, ks[i], vs[i], out, gran, tag[0], nH, nH, d, err=err, n_splits=ns)

    run("bf16", 0); run("pk", 0)
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(outs["bf16"], outs["pk"]))
    s = torch.cuda.Stream()
    graphs = {}
    with torch.cuda.stream(s):
        for label in ("bf16", "pk"):
            for i in range(NCOPY): run(label, i)
            s.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                for _ in range(REPS):
                    for i in range(NCOPY): run(label, i)
            gr.replay(); s.synchronize()
            graphs[label] = gr
        res = {"bf16": [], "pk": []}
        for _ in range(5):  # alternated: bf16, pk, bf16, pk, ...
            for label in ("bf16", "pk"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s); graphs[label].replay(); e1.record(s); s.synchronize()
                res[label].append(e0.elapsed_time(e1) * 1000 / (REPS * NCOPY))
    b, p = sorted(res["bf16"]), sorted(res["pk"])
    gain = b[2] - p[2]
    print(f"T={T:4d} n_splits={ns} bits_equal={same} err={int(err.item())} | bf16 us med={b[2]:.2f} (min {b[0]:.2f} max {b[4]:.2f}) | pk us med={p[2]:.2f} (min {p[0]:.2f} max {p[4]:.2f}) | "
          f"saved {gain:+.2f} us = {100 * gain / (saved / 6.3e6):.0f} % of the {saved / 6.3e6:.2f} us the bytes are worth", flush=True)
    del ks, vs
