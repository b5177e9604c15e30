"""CPU: the standard behind tests/test_predictor_exact_gpu.py discriminates, and reaches every branch it was built for.

  * the premises of the lattice class and the measured constant are re-derived here;
  * the thresholds of csrc/tp_body.h, csrc/predictors.hip, csrc/advance.hip and csrc/gemv.hip are parsed out of the sources, and every branch they open has a table entry;
  * every runner of oracle/predictor_cases.py is dry-run on the documented arithmetic in a summation order of no kernel (EmuAdaptor): zero elements outside;
  * each mutant of docs/predictor_exactness.md puts at least one element outside on the class the document names;
  * the same mutants are put through the assertions of tests/test_kernels_gpu.py on its shapes (the table of the document)."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import predictor_cases as pc
from oracle import predictor_truth as pt
from oracle import rowwise_truth as rt

BF16, F16, F32 = rt.BF16, rt.F16, rt.F32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynamic_llava_amd", "csrc")


def test_lattice_premises():
    """fp32 gelu_erf(k) == k for integers k >= 6 up to the largest lattice value, gelu(0) == 0; RNE_T(k rsqrt(1 + 1e-5)) == k for k <= 128 in bf16 and fp16."""
    k = torch.arange(6, 2049, dtype=torch.float32)
    assert torch.equal(F.gelu(k), k) and float(F.gelu(torch.zeros(1))) == 0.0
    r = torch.rsqrt(torch.tensor(1.0 + 1e-5, dtype=torch.float32))
    for dt in (BF16, F16):
        k = torch.arange(1, 129, dtype=torch.float32)
        assert torch.equal((k * r).to(dt).float(), k)
    assert abs(pt.GELU_XMIN + 0.7517916) < 1e-6 and abs(pt.GELU_MIN + 0.1699712) < 1e-6


def test_rho_score_is_four_times_the_measurement():
    worst = max(pt.measure_rho_score(dt) for dt in (BF16, F16))
    print(f"largest |fp32 - fp64| / (1 + |s|) of the score expression: {worst:.3e}; RHO_SCORE = {pt.RHO_SCORE:.2e}")
    assert 4 * worst <= pt.RHO_SCORE <= 4 * worst * 1.05


def test_score_needs_its_absolute_term():
    """A purely relative bound of the size of RHO_ACT does not cover the fp32 expression: for l0 >> l1 the score is far below an ulp of 1 + exp(l1 - l0)."""
    l0, l1 = torch.tensor([20.0]), torch.tensor([0.0])
    s32, s64 = pt.score_fp32(l0, l1).double(), pt.score64(l0.double(), l1.double())
    assert float(((s32 - s64).abs() / s64.abs())) > 100 * rt.RHO_ACT


def test_every_branch_has_a_case():
    br = pc.branches_in_sources(CSRC)
    assert br["max_chunks"] == pt.K_TP1_MAX_CHUNKS and br["pb"] == 2 and (br["k5_vecs"], br["max_passes"]) == (64, 8) and br["trip_chunks"] == pt.TRIP_CHUNKS
    assert br["h_max"] == pc.H_MAX and br["fused_maxc"] == pt.FUSED_MAXC
    cov = pc.coverage(br)
    for k, ids in cov.items():
        print(f"{k}: {ids[:3]}")
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    for dt, V in ((BF16, 8), (F32, 4)):  # the refused H is the first past the largest, in vectors
        assert pc.H_REFUSED[dt] == pc.H_MAX + V
    # the layout restated in predictor_truth equals the library's (a host query: no GPU)
    from dynamic_llava_amd import hip_ops

    for dt in pc.ALL:
        for (B, n, H, D, FF) in ((3, 577, 256, 128, 256), (1, 2049, 256, 128, 256), (2, 36, 4096, 512, 2048)):
            assert pt.vp_layout(B, n, H, D, FF, dt)["total"] == int(hip_ops.lib().dl_vision_predictor_workspace_bytes(B, n, H, D, FF, hip_ops.dtype_code(dt)))


def _dry(table, entry, order=1, mutant=None):
    R = pc.Runner(pc.EmuAdaptor(order, mutant))
    pc.TABLES[table][1](R, entry)
    R.finish()
    return R


@pytest.mark.parametrize("table", list(pc.TABLES))
def test_unmutated_emulation_is_inside(table):
    """Every entry, in a summation order that belongs to no kernel; the first entry of every dtype also in torch's own order."""
    seen = set()
    for e in pc.TABLES[table][0]:
        orders = (1, 0) if e["dtype"] not in seen else (1,)
        seen.add(e["dtype"])
        for order in orders:
            R = _dry(table, e, order)
            assert R.n > 0 and not R.bad, (e["id"], order, R.bad[:3])


# mutant -> (table, entry, what a flagged tag must contain): the class the document names
MUTANTS = {
    "last_chunk_dropped": ("text_predictor", "tp-bf16-H5128-D96-B3-pad0", "lattice stage 1"),
    "neighbour_bias": ("text_predictor", "tp-bf16-H5128-D96-B3-pad0", "lattice stage 1"),
    "no_rounding_before_gelu": ("text_predictor", "tp-f16-H520-D256-B3-pad0", "generic stage 2a"),
    "ln_eps_lost": ("text_predictor", "tp-bf16-H5128-D96-B3-pad0", "lattice stage 1"),
    "ln_row_at_stride_h": ("text_predictor", "tp-bf16-H520-D384-B32-pad16", "lattice stage 1"),
    "pass_reuses_weights": ("text_predictor", "tp-f16-H520-D256-B3-pad0", "lattice stage 2b logits"),
    "decision_ge": ("text_predictor", "tp-bf16-H5128-D96-B3-pad0", "lattice tie decision == (logit0 > logit1)"),
    "unrounded_n": ("vision_predictor", "vp-bf16-D256-n257-B3-L2", "lattice pool_concat"),
    "unrounded_tot": ("vision_predictor", "vp-bf16-D256-n577-B1-L0", "lattice pool_concat"),
    "tokens_past_16_dropped": ("vision_predictor", "vp-f16-D128-n2049-B1-L0", "lattice pool_concat"),
    "score_from_unrounded_logits": ("vision_predictor", "vp-bf16-D256-n577-B1-L0", "generic layers 0 score"),
    "img_start_of_row0": ("vision_predictor", "vp-bf16-D256-n257-B3-L2", "row_index"),
    "highest_index_on_ties": ("decode_advance", "advance-bf16-V32771", "aligned eos 0 next_ids"),
    "tail_skipped": ("decode_advance", "advance-bf16-V32771", "aligned eos 0 next_ids"),
    "second_trip_skipped": ("decode_advance", "advance-f32-V16388", "aligned eos 0 next_ids"),
    "banned_id_wins": ("decode_advance", "advance-bf16-V32771", "eos 3 next_ids"),
    "write_at_out_cap": ("decode_advance", "advance-bf16-V32771", "out_ids"),
}


def test_the_mutant_list_is_complete():
    assert set(MUTANTS) == set(pt.TP_MUTANTS + pt.POOL_MUTANTS + pt.HEAD_MUTANTS + pt.INDEX_MUTANTS + pt.ADVANCE_MUTANTS)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_is_outside(mutant):
    table, eid, where = MUTANTS[mutant]
    e = [e for e in pc.TABLES[table][0] if e["id"] == eid][0]
    R = _dry(table, e, 1, mutant)
    hits = [b["tag"] for b in R.bad if where in b["tag"]]
    assert hits, (mutant, [b["tag"] for b in R.bad][:8])


def test_unrounded_tot_is_invisible_where_rne_n_is_a_power_of_two():
    """bf16 n = 257 rounds to 256: dividing by a power of two commutes with the rounding -- why the table names n = 577 for that mutant."""
    e = [e for e in pc.VP_TABLE if e["id"] == "vp-bf16-D256-n257-B3-L2"][0]
    assert not _dry("vision_predictor", e, 1, "unrounded_tot").bad


# ------------------------------------------------------------------------------------------------------------------------------
# the older assertions (tests/test_kernels_gpu.py) on their shapes, fed the same mutants
# ------------------------------------------------------------------------------------------------------------------------------
ULP = {BF16: 2.0**-7, F16: 2.0**-10}


def _old_tp_passes(dt, H, D, B, mutant):
    """test_text_predictor_vs_oracle's assertions with the (mutated) emulation in the kernel's place: randn rows, contiguous."""
    g = torch.Generator().manual_seed(14)
    W = pc._generic_weights(H, D, dt, 13)
    x = torch.randn(B, H, generator=g).to(dt)

    def eager(Wd, xd):
        z = F.layer_norm(xd, (H,), Wd["ln_w"], Wd["ln_b"], 1e-5)
        for k in ("l1", "l3", "l5"):
            z = F.gelu(F.linear(z, Wd[k + "_w"], Wd[k + "_b"]))
        return F.linear(z, Wd["l7_w"], Wd["l7_b"])

    ref = eager(W, x)
    ref32 = eager({k: v.float() for k, v in W.items()}, x.float())
    o = pt.emulate_tp(x, None, W, 1, mutant)
    lg, dec = o["logits"], o["decision"]
    err, noise, scale = float((lg - ref32).abs().max()), float((ref.float() - ref32).abs().max()), float(ref32.abs().max())
    ok = err <= 2.0 * noise + 4 * ULP[dt] * scale
    ok = ok and torch.equal(dec.bool(), lg[:, 0] > lg[:, 1])
    sure = (ref32[:, 0] - ref32[:, 1]).abs() > 4 * (err + noise)
    return bool(ok and torch.equal(dec.bool()[sure], (ref[:, 0] > ref[:, 1])[sure]))


def _old_vp_passes(dt, mutant):
    """test_vision_predictor_vs_oracle's assertions (H 256, D 128, 36 tokens, B 3, uniform img_start) on the emulated pipeline."""
    H, D, FF, n, B, nhead = 256, 128, 256, 36, 3, 2
    c = pc.vp_case("generic", dt, H, D, FF, n, B, 2)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B * n, H, generator=g).to(dt)
    cu, st = torch.arange(0, (B + 1) * n, n, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    ws = torch.zeros(pt.vp_layout(B, n, H, D, FF, dt)["total"], dtype=torch.uint8)
    lg, sc = pc.EmuAdaptor(1, mutant).vp(x, cu, st, n, c.W, D, nhead, FF, ws, 2)

    def eager(W, xd):
        h = F.gelu(F.linear(F.layer_norm(xd, (H,), W["ln_w"], W["ln_b"], 1e-5), W["down_w"], W["down_b"])).view(B, n, D)
        h = pc.block_chain(h, W["blocks"], nhead)[-1]
        z = torch.cat([h[:, :, : D // 2], (h[:, :, D // 2 :].sum(1, keepdim=True) / torch.full((B, 1, 1), float(n), dtype=h.dtype)).expand(B, n, D // 2)], -1)
        z = F.gelu(F.linear(F.gelu(F.linear(z, W["out0_w"], W["out0_b"])), W["out2_w"], W["out2_b"]))
        return F.linear(z, W["out4_w"], W["out4_b"])

    f32 = lambda d: {k: (v.float() if torch.is_tensor(v) else [f32(b) for b in v]) for k, v in d.items()}
    ref, ref32 = eager(c.W, x), eager(f32(c.W), x.float())
    err, noise, scale = float((lg.float() - ref32).abs().max()), float((ref.float() - ref32).abs().max()), float(ref32.abs().max())
    ok = err <= 2.0 * noise + 4 * ULP[dt] * scale
    ref_score = F.log_softmax(lg.float(), dim=-1)[..., 0].to(dt)
    tol = 1.0 * ULP[dt] * ref_score.float().abs() + 1e-6
    return bool(ok and ((sc.float() - ref_score.float()).abs() <= tol).all())


def _old_advance_passes(ldt, mutant):
    """test_decode_advance's case (V = 32000, B = 5) and its assertions."""
    g = torch.Generator().manual_seed(15)
    B, V = 5, 32000
    logits = torch.randn(B, V, generator=g).to(ldt)
    logits[1, 777] = logits[1, 12345] = 50.0
    logits[3, 2] = 60.0
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    o = pt.emulate_advance(logits, i32([0, 1, 2, 3, 0]), i32([0, 0, 0, 0, 1]), torch.zeros(B, 4, dtype=torch.int64), (2, -1, -1), 0, i32([10, 20, 30, 40, 50]), i32([5, 6, 7, 8, 9]),
                           i32([1, 0, 1, 0, 1]), 0, True, mutant)
    ref = logits.float().argmax(-1)
    out = o["out_ids"]
    return bool(o["next_ids"].tolist() == [int(ref[0]), 777, int(ref[2]), 2, 0] and o["finished"].tolist() == [0, 0, 0, 1, 1] and o["step"].tolist() == [1, 2, 3, 4, 1]
                and o["kv_full"].tolist() == [11, 21, 31, 41, 51] and o["kv_sparse"].tolist() == [6, 6, 8, 8, 10]
                and out[0, 0] == ref[0] and out[1, 1] == 777 and out[2, 2] == ref[2] and out[3, 3] == 2 and out[4, 0] == 0)


# the last column of the mutant table in docs/predictor_exactness.md: twelve of the seventeen go unnoticed
OLD_ASSERTIONS_PASS = {
    "last_chunk_dropped": True, "neighbour_bias": False, "no_rounding_before_gelu": True, "ln_eps_lost": True, "ln_row_at_stride_h": True, "pass_reuses_weights": False,
    "decision_ge": True, "unrounded_n": True, "unrounded_tot": True, "tokens_past_16_dropped": False, "score_from_unrounded_logits": False, "img_start_of_row0": True,
    "highest_index_on_ties": False, "tail_skipped": True, "second_trip_skipped": True, "banned_id_wins": True, "write_at_out_cap": True,
}


def test_old_assertions_on_old_shapes():
    """The table of docs/predictor_exactness.md: which mutants the older assertions let through (printed, and asserted per mutant)."""
    passed = {}
    for m in pt.TP_MUTANTS:
        passed[m] = all(_old_tp_passes(dt, H, D, B, m) for dt in (BF16, F16) for (H, D, B) in ((256, 128, 3), (4096, 512, 1)))
    for m in pt.POOL_MUTANTS + pt.HEAD_MUTANTS + pt.INDEX_MUTANTS:
        passed[m] = all(_old_vp_passes(dt, m) for dt in (BF16, F16))
    for m in pt.ADVANCE_MUTANTS:
        passed[m] = _old_advance_passes(BF16, m)
    assert _old_tp_passes(BF16, 256, 128, 3, None) and _old_vp_passes(BF16, None) and _old_advance_passes(BF16, None)
    for m, p in passed.items():
        print(f"{m:32s} older assertions: {'pass' if p else 'FAIL'}")
    assert passed == OLD_ASSERTIONS_PASS, {m: p for m, p in passed.items() if p != OLD_ASSERTIONS_PASS[m]}
