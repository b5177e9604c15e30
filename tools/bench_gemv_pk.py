"""dl_gemv vs dl_gemv_pk on the flagship's batch-1 launch shapes: captured graphs over rotating weight copies (no cache reuse)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dynamic_llava_amd import hip_ops as ops, bf16pack as bp

A, PAIR = ops.GEMV_ADDNORM, ops.GEMV_OUT_SILU_PAIR
SHAPES = [("o", 4096, 4096, 0), ("gate|up", 22016, 4096, A | PAIR), ("down", 4096, 11008, 0), ("down 13B", 5120, 13824, 0), ("lm_head", 32000, 4096, A)]
NCOPY = 6
REPS = 10
for name, N, K, mode in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(N + K)
    ws = [(torch.randn(N, K, generator=g, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(NCOPY)]
    ps = [bp.pack(w) for w in ws]
    x = torch.randn(1, K, device="cuda").to(torch.bfloat16)
    d = torch.randn(1, K, device="cuda").to(torch.bfloat16)
    nw = torch.ones(K, device="cuda", dtype=torch.bfloat16)
    ho = torch.empty_like(x)
    ny = N // 2 if mode & PAIR else N
    y0 = torch.empty(1, ny, dtype=torch.bfloat16, device="cuda")
    y1 = torch.empty(1, ny, dtype=torch.bfloat16, device="cuda")
    def run(fn, wt, y):
        if mode == 0:
            fn(wt, y, x=x)
        else:
            fn(wt, y, mode=mode, h_in=x, h_out=ho, delta=d, norm_w=nw, eps=1e-5)
    run(ops.gemv, ws[0], y0); run(ops.gemv_pk, ps[0], y1)
    torch.cuda.synchronize()
    same = torch.equal(y0.view(torch.int16), y1.view(torch.int16))
    res = {}
    for label, fn, wts, y in (("bf16", ops.gemv, ws, y0), ("pk", ops.gemv_pk, ps, y1)):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for wt in wts: run(fn, wt, y)
            s.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                for _ in range(REPS):
                    for wt in wts: run(fn, wt, y)
            gr.replay(); s.synchronize()
            ts = []
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s); gr.replay(); e1.record(s); s.synchronize()
                ts.append(e0.elapsed_time(e1) * 1000 / (REPS * NCOPY))
        res[label] = sorted(ts)
    ratio = bp.packed_nbytes(ps[0]) / bp.raw_nbytes(ps[0])
    pkb = bp.packed_nbytes(ps[0])
    print(f"{name:8s} [{N},{K}] bits_equal={same} bytes_ratio={ratio:.4f} bf16 us med={res['bf16'][2]:.2f} (min {res['bf16'][0]:.2f}) pk us med={res['pk'][2]:.2f} (min {res['pk'][0]:.2f}) "
          f"pk_bytes/6.3TB/s={pkb / 6.3e6:.2f} us", flush=True)
    del ws, ps
