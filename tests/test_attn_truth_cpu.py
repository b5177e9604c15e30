"""CPU: the attention truth, its per-element bound and the hard input distributions of oracle/attn_truth.py.

What is shown here, without a GPU:
  * every distribution has the property it was built for (sink mass, the running max moving in the last tile, ...);
  * a tiled emulation of the documented arithmetic (fp32 scores and statistics, P rounded to the 16-bit type before P V, one output
    rounding) stays inside the bound on every distribution, dtype and shape -- the worst ratios are printed (pytest -s) and recorded in
    docs/attention_error_budget.md;
  * every mutant of that emulation (a bug of the kind the HIP kernels can have) is outside the bound on at least one distribution, named
    in KILLED_BY -- which is also why no distribution can be dropped;
  * the absolute 6 ulp tolerance of tests/test_kernels_gpu.py::test_attn_prefill does not see an off-by-one causal mask on a row with an
    attention sink; the per-element bound does;
  * dl_attn_prefill_route (a pure host function of the built library) returns, with no DL_PF_* switch set, the dispatch of the launch as it was
    before the choice was factored out into one function: PARENT_ROUTE restates that code."""
import math

import pytest
import torch

from oracle import attn_truth as at

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (Lq, Lk, d, nH, nKV, causal): self-attention (Lq == Lk), a chunk on a cache (Lq < Lk, causal: kv_offset = Lk - Lq) and a decode row (Lq = 1)
SHAPES = [(170, 170, 128, 2, 1, True), (577, 577, 64, 2, 2, False), (300, 300, 128, 4, 2, True), (129, 129, 64, 4, 2, False), (70, 270, 128, 2, 1, True), (1, 632, 128, 4, 2, False), (65, 65, 32, 2, 2, True)]


def _mask(Lq, Lk, causal):
    return dict(causal=causal, kv_offset=(Lk - Lq) if causal else 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("name", at.DISTRIBUTIONS + at.DECODE_ONLY)
def test_emulation_is_inside_the_bound_and_properties_hold(name, dtype):
    worst = 0.0
    for i, (Lq, Lk, d, nH, nKV, causal) in enumerate(SHAPES):
        if name in at.DECODE_ONLY and Lq != 1:
            continue
        q, k, v = at.make_case(name, Lq, Lk, d, dtype, seed=i, nH=nH, nKV=nKV)
        m = _mask(Lq, Lk, causal)
        if not (name == "big" and Lq == 1):  # (one decode row has too few scores for its largest to pass 500)
            what = at.check_property(name, q, k, v, dtype=dtype, **m)
        t = at.truth(q, k, v, **m)
        r, ulps, _ = at.worst_ratio(at.emulate(q, k, v, **m), t, d, dtype)
        print(f"{name:14s} {str(dtype)[6:]:9s} Lq={Lq:4d} Lk={Lk:4d} d={d:3d} causal={int(causal)}  err/tol {r:6.3f}  ({what})")
        assert r < 1.0, (name, dtype, Lq, Lk, d, r)
        worst = max(worst, r)
    print(f"WORST {name} {dtype}: {worst:.3f}")


# mutant -> a distribution that is REQUIRED to expose it (chosen by the reasoning in the comments, then checked), the mask it needs
KILLED_BY = {
    "mask_off_by_one_last_tile": "sink",   # the wrongly visible key takes a share from a row whose output is tiny (|v_0| small): invisible to an absolute bound
    "l_not_rescaled": "late_peak",         # the running max moves in the last tile: the sum collected before it is e^(m_new - m_old) too large
    "read_past_lk": "sink",                # the key behind the row is the next request's sink: it halves every other key's share
    "gqa_off_by_one_group": "gauss",       # another group's K / V: wrong everywhere
    "max_not_carried": "big",              # exp() of a positive difference of scores in the hundreds overflows
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("mutant", at.MUTANTS)
def test_every_mutant_is_outside_the_bound_somewhere(mutant, dtype):
    causal = mutant != "read_past_lk"  # (a causal mask hides the key behind the row)
    Lq = Lk = 170
    d, nH, nKV = 128, 4, 2
    caught = {}
    for name in at.DISTRIBUTIONS:
        q, k, v = at.make_case(name, Lq, Lk, d, dtype, seed=11, nH=nH, nKV=nKV)
        t = at.truth(q, k, v, causal=causal)
        assert at.worst_ratio(at.emulate(q, k, v, causal=causal), t, d, dtype)[0] < 1.0
        caught[name] = at.worst_ratio(at.emulate(q, k, v, causal=causal, mutant=mutant), t, d, dtype)[0]
    names = [n for n, r in caught.items() if r > 1.0]
    print(f"{mutant} {dtype}: outside the bound on {names}; ratios " + ", ".join(f"{n} {r:.3g}" for n, r in caught.items()))
    assert KILLED_BY[mutant] in names, (mutant, caught)


def test_l_not_rescaled_needs_the_other_distributions():
    """An `l` that is not rescaled when the max moves is invisible where the first tile already holds the row's maximum (sink: key 0; plateau: the
    higher key sits in an early tile or the scores are equal): the distributions need each other."""
    for dtype in (torch.bfloat16, torch.float16):
        for name, expect_caught in (("sink", False), ("late_peak", True), ("ramp", True)):
            q, k, v = at.make_case(name, 170, 170, 128, dtype, seed=11, nH=2, nKV=1)
            t = at.truth(q, k, v, causal=True)
            r = at.worst_ratio(at.emulate(q, k, v, causal=True, mutant="l_not_rescaled"), t, 128, dtype)[0]
            assert (r > 1.0) == expect_caught, (name, dtype, r)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_old_absolute_tolerance_is_blind_to_a_mask_off_by_one_on_a_sink_row(dtype):
    Lq = Lk = 170
    d = 128
    q, k, v = at.make_case("sink", Lq, Lk, d, dtype, seed=11, nH=4, nKV=2)
    t = at.truth(q, k, v, causal=True)
    out = at.emulate(q, k, v, causal=True, mutant="mask_off_by_one_last_tile")
    err = float((out.double() - t.O).abs().max())
    ratio = at.worst_ratio(out, t, d, dtype)[0]
    print(f"{dtype}: max abs err {err:.3g} = {err / (6 * at.ULP[dtype]):.2f} of 6 ULP; {ratio:.1f} x the per-element bound")
    assert err < 6 * at.ULP[dtype], "the present tolerance of test_attn_prefill would have passed this bug"
    assert ratio > 1.0, "the per-element bound does not"


# ---- the route query against a restatement of the dispatch at the parent commit (launch_mfma / attn_prefill_impl before the refactor) ----
def PARENT_ROUTE(B, L, nH, d, causal, cached, q_rs, kv_rs, out_rs, dtype):
    if L == 0:
        return "NONE"
    if dtype == torch.float32:
        return "SIMPLE_F32"
    nw = 2 if L <= 256 else 4
    pipe = L > 256 and d == 128
    strides_ok = q_rs % 8 == 0 and kv_rs % 8 == 0 and out_rs % 4 == 0 and L * kv_rs * 2 < 2**31
    if d == 64 and not causal and not cached and 256 < L <= 608 and strides_ok:
        return "HEAD_D64" if B * nH >= 256 else "WHOLE_ROW_D64_KW4"
    if d == 128 and causal and not cached and 64 < L <= 256 and B * nH >= 1 and strides_ok:
        return "WHOLE_D128_Z2" if B * nH <= 128 else "WHOLE_D128_Z1"
    if d == 128 and causal and not cached and 64 < L <= 192 and B * nH * ((L + 31) // 32) <= 256:
        return "KSPLIT_D128_K2" if L <= 128 else "KSPLIT_D128_K3"
    if d == 64 and not causal and not cached and L > 128 and B * nH * ((L + 63) // 64) <= 256:
        return "KSPLIT_D64"
    if pipe:
        return "PIPE_4W" if nw == 4 else "PIPE_2W"
    if nw == 4:
        return "PLAIN_4W_K128" if (d == 64 and L > 128) else "PLAIN_4W"
    return "PLAIN_2W"


# tests/test_kernels_gpu.py::test_attn_prefill's shapes (nH, nKV, d, lens) and a few on the thresholds
PREFILL_SHAPES = [(4, 4, 128, [170, 1, 64, 65, 200]), (8, 8, 64, [576, 36]), (16, 16, 64, [577]), (4, 2, 64, [129, 300]), (4, 2, 128, [129]), (32, 32, 128, [170]),
                  (4, 4, 128, [117, 65, 192, 3]), (4, 4, 128, [128, 66]), (4, 2, 128, [300, 631, 17, 257]), (2, 2, 32, [37, 150, 5]),
                  (32, 32, 128, [170, 214, 158, 256, 65, 1, 16, 17, 33, 255]), (32, 8, 128, [200, 64, 129, 96, 31, 241, 2, 160]), (64, 64, 128, [97, 224, 5, 180]),
                  (16, 16, 64, [577] * 14 + [300, 608, 257, 590]), (32, 8, 64, [577, 576, 290, 601, 333, 480, 259, 512]),
                  (4, 4, 128, [64]), (4, 4, 128, [256]), (4, 4, 128, [257]), (4, 4, 64, [128]), (4, 4, 64, [256]), (4, 4, 64, [257]), (4, 4, 64, [608]), (4, 4, 64, [609]),
                  (4, 4, 128, [4096]), (33, 33, 128, [100] * 4), (2, 2, 32, [300])]


def test_route_query_is_the_parent_commits_dispatch(monkeypatch):
    from dynamic_llava_amd import hip_ops

    for var in ("DL_PF_NW", "DL_PF_PIPE", "DL_PF_WHOLE", "DL_PF_WHOLE_KW", "DL_PF_WHOLE128", "DL_PF_KSPLIT", "DL_PF_HEAD64_MIN", "DL_PF_WHOLE128_MIN", "DL_PF_WHOLE128_ZPAIRS"):
        monkeypatch.delenv(var, raising=False)
    rows = []
    for nH, nKV, d, lens in PREFILL_SHAPES:
        W = (nH + 2 * nKV) * d
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            for causal in (True, False):
                for out_rs in (nH * d, nH * d + 6):  # (+ 6: an output row stride the whole-row kernels refuse)
                    got = hip_ops.attn_prefill_route(len(lens), max(lens), 0, nH, nKV, d, causal, False, W, W, out_rs, dtype)
                    want = PARENT_ROUTE(len(lens), max(lens), nH, d, causal, False, W, W, out_rs, dtype)
                    rows.append((nH, nKV, d, max(lens), len(lens), str(dtype)[6:], int(causal), out_rs, want, got))
                    assert got == want, rows[-1]
            got = hip_ops.attn_prefill_route(len(lens), max(lens), max(lens) + 200, nH, nKV, d, False, True, W, 12345, nH * d, dtype)
            assert got == PARENT_ROUTE(len(lens), max(lens), nH, d, True, True, W, d, nH * d, dtype), (nH, d, lens, dtype, got)
    seen = {r[-1] for r in rows}
    print("\n".join(f"nH={r[0]:2d} nKV={r[1]:2d} d={r[2]:3d} max_seqlen={r[3]:4d} B={r[4]:2d} {r[5]:8s} causal={r[6]} out_rs={r[7]:5d}  parent {r[8]:18s} now {r[9]}" for r in rows if r[7] % 4 == 0))
    assert {"SIMPLE_F32", "PLAIN_2W", "PLAIN_4W_K128", "PIPE_4W", "KSPLIT_D64", "WHOLE_ROW_D64_KW4", "HEAD_D64", "WHOLE_D128_Z1", "WHOLE_D128_Z2", "KSPLIT_D128_K2", "KSPLIT_D128_K3"} <= seen
    # arguments the launch refuses; an empty launch
    r = hip_ops.attn_prefill_route
    assert r(1, 10, 0, 4, 3, 128, True, False, 512, 512, 512, torch.bfloat16) is None      # n_heads % n_kv_heads
    assert r(1, 10, 0, 4, 4, 96, True, False, 512, 512, 512, torch.bfloat16) is None       # head_dim
    assert r(1, 10, 0, 4, 4, 128, True, False, 516, 512, 512, torch.bfloat16) is None      # row stride
    assert r(1, 10, 9000, 4, 4, 128, True, True, 512, 512, 512, torch.float32) is None     # fp32: 8192 keys
    assert r(1, 10, 5, 4, 4, 128, True, True, 512, 512, 512, torch.bfloat16) is None       # cached: max_kv_len < max_seqlen
    assert r(1, 0, 0, 4, 4, 128, True, False, 512, 512, 512, torch.bfloat16) == "NONE"
    assert len(hip_ops.PF_ROUTES) == 16


def test_route_names_match_the_header():
    import os
    import re

    from dynamic_llava_amd import hip_ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dynllava.h")).read()
    names = dict((n, int(v)) for n, v in re.findall(r"\bDL_PF_([A-Z0-9_]+) = (\d+)", hdr))
    assert names.pop("ROUTE_COUNT") == len(hip_ops.PF_ROUTES)
    assert [n for n, _ in sorted(names.items(), key=lambda kv: kv[1])] == list(hip_ops.PF_ROUTES)
