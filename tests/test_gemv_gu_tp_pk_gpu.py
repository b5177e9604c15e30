"""GPU: dl_gemv_gu_tp_pk (the gate|up + text predictor launch with the projection rows streamed as lossless 12-bit packed bf16) must return
dl_gemv_gu_tp's bits on the unpacked matrix: activation row, h_out, predictor logits, decision and workspace."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import bf16pack as bp  # noqa: E402
from dynamic_llava_amd import hip_ops as ops  # noqa: E402

BF = torch.bfloat16
EPS = 1e-5


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int16) if t.dtype == BF else t)


def _operands(H, I, D, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *shape, s=0.02: (torch.randn(*shape, device="cuda", generator=g) * s).to(BF)
    Wgu, nw = rnd(2 * I, H), 1 + rnd(H, s=0.1)
    w = ops.TpWeights()
    keep = [1 + rnd(H, s=0.1), rnd(H, s=0.1), rnd(D, H, s=0.05), rnd(D, s=0.1), rnd(D // 2, D, s=0.1), rnd(D // 2, s=0.1), rnd(D // 4, D // 2, s=0.2), rnd(D // 4, s=0.1),
            rnd(2, D // 4, s=0.5), rnd(2, s=0.1)]
    (w.ln_w, w.ln_b, w.l1_w, w.l1_b, w.l3_w, w.l3_b, w.l5_w, w.l5_b, w.l7_w, w.l7_b) = [t.data_ptr() for t in keep]
    return rnd, Wgu, nw, w, keep


@pytest.mark.parametrize("H,I,D", [(1024, 2816, 256), (4096, 11008, 1024)])
def test_bit_equal_to_the_bf16_fused_launch(H, I, D):
    """Eight steps, two call tags, on one granule buffer.  Escapes are planted in a gate row and in its partner up row (the two rows a wave reads
    together), in the first group, in the last and in between."""
    rnd, Wgu, nw, w, keep = _operands(H, I, D)
    for gate_row in (0, 1234, I - 1):
        Wgu[gate_row, 7] = 0.0
        Wgu[gate_row, H - 1] = -1.0e-30
        Wgu[I + gate_row, 513] = 2.0e4  # the partner: another span of the same pass
        Wgu[I + gate_row, 1023] = -0.0
    p = bp.pack(Wgu, force=True)
    assert torch.equal(bp.unpack(p).view(torch.int16), Wgu.view(torch.int16))
    assert int(p.hdr[0, 0]) & 1 and int(p.hdr[I, 0]) & 2 and int(p.hdr[I - 1, 0]) & 1 and int(p.hdr[2 * I - 1, 0]) & 2
    gran = ops.gemv_gu_tp_workspace(D, "cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws_r, ws_f = ops.text_predictor_workspace(1, D, "cuda"), ops.text_predictor_workspace(1, D, "cuda")
    for step in range(8):
        h0, delta = rnd(1, H, s=1.0), rnd(1, H, s=1.0)
        pos = torch.tensor([50 + step // 2], dtype=torch.int32, device="cuda")
        y_r, ho_r = torch.zeros(1, I, dtype=BF, device="cuda"), torch.zeros(1, H, dtype=BF, device="cuda")
        lg_r, dec_r = torch.zeros(1, 2, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.gemv_gu_tp(Wgu, y_r, h0, ho_r, delta, nw, EPS, w, D, ws_r, lg_r, dec_r, pos, gran, 2 + (step & 1), err=err)
        y_f, ho_f = torch.full_like(y_r, 3.0), torch.full_like(ho_r, 5.0)
        lg_f, dec_f = torch.full_like(lg_r, 7.0), torch.full_like(dec_r, 5)
        ops.gemv_gu_tp_pk(p, y_f, h0, ho_f, delta, nw, EPS, w, D, ws_f, lg_f, dec_f, pos, gran, step & 1, err=err)
        for name, a, b in (("activation row", y_f, y_r), ("h_out", ho_f, ho_r), ("logits", lg_f, lg_r), ("decision", dec_f, dec_r), ("workspace", ws_f, ws_r)):
            assert torch.equal(_bits(a), _bits(b)), (step, name)
    assert torch.isfinite(y_r.float()).all()
    assert int(err.item()) == 0


def test_short_rows_are_refused():
    """H = 512: no whole pair of spans in a row -- DL_ERR_ARG, nothing launched."""
    H, I, D = 512, 1536, 64
    rnd, Wgu, nw, w, keep = _operands(H, I, D)
    p = bp.pack(Wgu, force=True)
    y, ho = torch.full((1, I), 3.0, dtype=BF, device="cuda"), torch.full((1, H), 5.0, dtype=BF, device="cuda")
    lg, dec = torch.full((1, 2), 7.0, device="cuda"), torch.full((1,), 5, dtype=torch.int32, device="cuda")
    pos = torch.tensor([50], dtype=torch.int32, device="cuda")
    with pytest.raises(ops.HipOpsError, match="dl_gemv_gu_tp_pk"):
        ops.gemv_gu_tp_pk(p, y, rnd(1, H, s=1.0), ho, rnd(1, H, s=1.0), nw, EPS, w, D, ops.text_predictor_workspace(1, D, "cuda"), lg, dec, pos, ops.gemv_gu_tp_workspace(D, "cuda"), 0)
    torch.cuda.synchronize()
    assert bool((y == 3.0).all() and (ho == 5.0).all() and (lg == 7.0).all() and (dec == 5).all())
