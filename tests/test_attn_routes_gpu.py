"""GPU: every attention kernel the library can dispatch to, on hard inputs, against an fp64 truth under a per-element bound.

tests/test_kernels_gpu.py draws q, k, v from N(0, 1) and holds the result to an absolute tolerance; that is blind where outputs are small
(tests/test_attn_truth_cpu.py shows an off-by-one mask passing it) and cannot take inputs with large values at all.  Here
  * the inputs are the distributions of oracle/attn_truth.py (attention sink, late peak, ramps, plateau, scores in the hundreds, value
    outliers, a dominant / negligible appended token, the dominant slab key placed on split and trip boundaries);
  * the bound is that module's derived per-element tolerance (no fitted constant; measured ratios: docs/attention_error_budget.md);
  * every launch first asserts, through dl_attn_prefill_route, that the shape reaches the kernel the entry was written for, and a closing test
    asserts that every value of the route enum is driven.  Kernels that only a DL_PF_* switch reaches (the fall-backs the tuning tools A/B
    against) are driven through that switch; the three thresholds the library caches on first use are crossed by shape.
max_seqlen may overstate the longest row (model.py sizes the device-layout prefill for a width bucket): entries with `over` run a second
time with an overstated bound and must return the same bits.  The tables live in oracle/attn_cases.py (shared with tools/attn_error_table.py)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attn_cases as ac  # noqa: E402
from oracle import attn_truth as at  # noqa: E402

DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


@pytest.fixture(scope="module")
def ops():
    from dynamic_llava_amd import hip_ops

    hip_ops.require_gpu()
    for var in ac.PF_CACHED_THRESHOLDS:
        assert var not in os.environ, f"{var} is cached by the library on first use: unset it for the test run"
    return hip_ops


def _report(what, r, ulps, where):
    print(f"{what}: err/tol {r:.3f}, {ulps:.3g} ULP of the element, worst at {where}")


@pytest.mark.parametrize("entry", ac.PREFILL_TABLE, ids=[e.id for e in ac.PREFILL_TABLE])
def test_prefill_route(ops, entry, monkeypatch):
    bad = []
    with ac.pf_env(entry.env, monkeypatch.setenv, monkeypatch.delenv):
        for dtype in entry.dtypes:
            assert ac.prefill_route(ops, entry, dtype) == entry.route
            if entry.over:
                assert ac.prefill_route(ops, entry, dtype, max_seqlen=max(entry.lens) + entry.over) == entry.route
            for dist in at.DISTRIBUTIONS:
                r, ulps, where = ac.run_prefill(ops, entry, dist, dtype)
                _report(f"{entry.id} {DT_ID[dtype]} {dist}", r, ulps, where)
                if not r < 1.0:
                    bad.append((DT_ID[dtype], dist, r, where))
    assert not bad, bad


def test_every_prefill_route_is_driven(ops):
    """Every value of the route enum has a table entry (whose test asserts that the launch really takes it)."""
    assert {e.route for e in ac.PREFILL_TABLE} == set(ops.PF_ROUTES)
    n = ops.lib().dl_attn_prefill_route  # and the enum has no value the binding does not name
    assert len(ops.PF_ROUTES) == 16 and n is not None


@pytest.mark.parametrize("entry", ac.CACHED_TABLE, ids=[f"{e[0]}-h{e[1]}kv{e[2]}d{e[3]}-chunk{max(e[4])}" for e in ac.CACHED_TABLE])
def test_prefill_cached(ops, entry, monkeypatch):
    bad = []
    with ac.pf_env({}, monkeypatch.setenv, monkeypatch.delenv):
        for dtype in ((torch.float32,) if entry[0] == "SIMPLE_F32" else (torch.bfloat16, torch.float16)):
            for dist in at.DISTRIBUTIONS:
                r, ulps, where = ac.run_cached(ops, entry, dist, dtype)
                _report(f"cached {entry[0]} d{entry[3]} {DT_ID[dtype]} {dist}", r, ulps, where)
                if not r < 1.0:
                    bad.append((DT_ID[dtype], dist, r, where))
    assert not bad, bad


def _decode_params():
    out = []
    for kernel in ("decode", "rope", "parts"):
        for nH, nKV, d in ac.DECODE_HEADS:
            for dtype in (torch.bfloat16, torch.float16, torch.float32):
                if dtype == torch.float32 and (kernel == "parts" or (nH, nKV, d) not in ((8, 2, 128), (4, 4, 64))):
                    continue  # (the partial-sum launch is 16-bit only; fp32 has one code path per head_dim)
                out.append(pytest.param(kernel, nH, nKV, d, dtype, id=f"{kernel}-h{nH}kv{nKV}d{d}-{DT_ID[dtype]}"))
    return out


@pytest.mark.parametrize("kernel,nH,nKV,d,dtype", _decode_params())
def test_decode(ops, kernel, nH, nKV, d, dtype):
    """dl_attn_decode / dl_attn_decode_rope / dl_attn_decode_rope_parts over keys_in_flight {64, 128 (the eight-wave kernel), 256} x chunk_keys {0, 256, 100} x
    n_splits {1, 3, 4, 32} x call_tag {-1, 5}: rows of kv_len 0, 1, 63, 64, 127, 128, 129, 255, 256, 1023 in one batch, NaN behind kv_len."""
    launches = ac.decode_launches(kernel)
    if kernel == "rope":
        assert (1, 128, 256, -1) in launches, "the production pairing of small decode batches"
    bad = []
    for dist_entry in ac.DECODE_DISTS:
        res = ac.run_decode(ops, kernel, dist_entry, dtype, nH, nKV, d)
        launch, (r, ulps, where) = max(res.items(), key=lambda kv: kv[1][0])
        _report(f"{kernel} h{nH}kv{nKV}d{d} {DT_ID[dtype]} {dist_entry[0]} (worst of {len(res)} launches: n_splits, keys_in_flight, chunk_keys, call_tag = {launch})", r, ulps, where)
        bad += [(dist_entry[0], l, w) for l, w in res.items() if not w[0] < 1.0]
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("nH,nKV,d,H", ac.QKV_ATTN_SHAPES)
def test_gemv_qkv_attn(ops, dtype, nH, nKV, d, H):
    bad = []
    for T_old in ac.QKV_ATTN_T_OLD:
        for dist in ac.QKV_ATTN_DISTS:
            res = ac.run_qkv_attn(ops, dist, dtype, nH, nKV, d, H, T_old)
            ns, (r, ulps, where) = max(res.items(), key=lambda kv: kv[1][0])
            _report(f"gemv_qkv_attn h{nH}kv{nKV}d{d} {DT_ID[dtype]} T_old {T_old} {dist} (worst: {ns})", r, ulps, where)
            bad += [(T_old, dist, n, w) for n, w in res.items() if not w[0] < 1.0]
    assert not bad, bad
