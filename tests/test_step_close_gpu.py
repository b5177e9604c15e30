"""The step-closing contract (csrc/step_close.h), once, through the three entries that end a decode step: dl_decode_advance (argmax), dl_decode_sample with
top_k = 1 (the draw can only be the maximum) and dl_decode_score with the row's argmax as its label.  On a row with a unique finite maximum all three pick
the same token, so everything they do with it -- pad for a finished row, the EOS flag, the append while step < out_cap, the step counter, both KV
lengths -- must equal oracle.predictor_truth.advance_ref exactly (the scorer: the reference without an EOS set; its label sequence ends a row, not a token).

Rows: step in {0, 1, out_cap - 1, out_cap, out_cap + 1} x finished in {0, 1}, both decisions under every step and every flag, distinct lengths.  Shapes: the
smallest that reach both load paths of each kernel -- 16-bit V = 9 on a 16-byte addressable stride (one whole chunk + a tail) and V = 41 on an odd stride
(scalar loads only); fp32 V = 5 (one chunk + a tail).  Every optional pointer set is removed in turn.  Everything compared is an integer: no tolerance."""
import pytest
import torch

from oracle import predictor_truth as pt

B, OUT_CAP, LABEL_CAP, PAD, G = 10, 4, 6, 2, 64
STEP = [0, 1, OUT_CAP - 1, OUT_CAP, OUT_CAP + 1] * 2
FIN = [0] * 5 + [1] * 5
DEC = [1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
KV_FULL = [100 + 7 * b for b in range(B)]
KV_SPARSE = [40 + 3 * b for b in range(B)]
# (dtype, V, row stride, argmax of row b = (mul * b + off) % V: every chunk and the tail hold one)
CONFIGS = {"bf16-V9": (torch.bfloat16, 9, 16, 7, 8), "f16-V9": (torch.float16, 9, 16, 7, 8), "bf16-V41-odd": (torch.bfloat16, 41, 43, 9, 40),
           "f16-V41-odd": (torch.float16, 41, 43, 9, 40), "f32-V5": (torch.float32, 5, 8, 3, 1)}
DROPS = {"all": (), "no-out_ids": ("out_ids",), "no-step": ("step",), "no-finished": ("finished",), "no-kv": ("kv_full", "kv_sparse"), "no-decision": ("decision",)}


def table(name):
    """-> logits [B, V] on the CPU (quarters in [-8, 8): exact in every dtype; one -inf per row; the maximum 20.0 once), the rows' argmax, the EOS set: three of
    the argmax values, so that some unfinished rows end on each id and others do not end."""
    dtype, V, _, mul, off = CONFIGS[name]
    g = torch.Generator().manual_seed(V)
    x = (torch.randint(-32, 32, (B, V), generator=g).float() / 4).to(dtype)
    amax = [(mul * b + off) % V for b in range(B)]
    for b in range(B):
        x[b, (amax[b] + 2) % V] = float("-inf")
        x[b, amax[b]] = 20.0
    assert x.float().argmax(1).tolist() == amax and all(int((x[b].float() == 20.0).sum()) == 1 for b in range(B))
    return x, amax, (amax[1], amax[3], amax[4])


def state(drop=()):
    s = dict(step=torch.tensor(STEP, dtype=torch.int32), finished=torch.tensor(FIN, dtype=torch.int32), out_ids=torch.full((B, OUT_CAP), -7, dtype=torch.int64),
             kv_full=torch.tensor(KV_FULL, dtype=torch.int32), kv_sparse=torch.tensor(KV_SPARSE, dtype=torch.int32), decision=torch.tensor(DEC, dtype=torch.int32))
    return {k: (None if k in drop else v) for k, v in s.items()}


def expected(x, eos, drop=()):
    s = state(drop)
    return pt.advance_ref(x, s["step"], s["finished"], s["out_ids"], eos, PAD, s["kv_full"], s["kv_sparse"], s["decision"], 0)


def test_reference_gives_what_the_table_expects():
    """advance_ref itself, on hand-written expectations (CPU): a finished row gives pad, a row at out_cap gets no write but its step advances, an EOS token
    sets the flag, kv_len_full advances by 1 and kv_len_sparse by the decision."""
    x, amax, eos = table("f32-V5")
    assert amax == [1, 4, 2, 0, 3, 1, 4, 2, 0, 3] and eos == (4, 0, 3)
    w = expected(x, eos)
    assert w["next_ids"].tolist() == [1, 4, 2, 0, 3] + [PAD] * 5
    assert w["finished"].tolist() == [0, 1, 0, 1, 1] + [1] * 5  # rows 1, 3, 4 emit an EOS id
    assert w["step"].tolist() == [1, 2, 4, 5, 6] * 2
    assert w["out_ids"].tolist() == [[1, -7, -7, -7], [-7, 4, -7, -7], [-7, -7, -7, 2], [-7] * 4, [-7] * 4,
                                     [PAD, -7, -7, -7], [-7, PAD, -7, -7], [-7, -7, -7, PAD], [-7] * 4, [-7] * 4]
    assert w["kv_full"].tolist() == [n + 1 for n in KV_FULL] and w["kv_sparse"].tolist() == [n + d for n, d in zip(KV_SPARSE, DEC)]
    n = expected(x, (-1, -1, -1), ("finished", "decision"))  # no flags: every row emits its argmax; no decision: the sparse length advances by 1
    assert n["next_ids"].tolist() == amax and n["finished"] is None and n["kv_sparse"].tolist() == [k + 1 for k in KV_SPARSE]
    assert expected(x, eos, ("step",))["out_ids"].tolist() == [[-7] * 4] * B  # out_ids is written through step only


def banded(shape, fill, dtype):
    n = shape[0] * shape[1]
    buf = torch.full((G + n + G,), fill, dtype=dtype, device="cuda")
    return buf, buf[G : G + n].view(shape)


def run(ops, entry, xd, amax, eos, drop):
    """One launch of `entry` on a fresh state -> every tensor it may write, on the CPU (guard bands included)."""
    s = {k: (None if v is None else v.cuda()) for k, v in state(drop).items()}
    bufs = {}
    if s["out_ids"] is not None:
        bufs["out_ids"], s["out_ids"] = banded((B, OUT_CAP), -7, torch.int64)
    nxt = torch.full((B,), -5, dtype=torch.int64, device="cuda")
    tail = (s["kv_full"], s["kv_sparse"], s["decision"])
    if entry == "advance":
        ops.decode_advance(xd, nxt, s["out_ids"], s["step"], s["finished"], eos, PAD, *tail)
    elif entry == "sample":
        prm = ops.sample_params_block("cuda")
        prm.copy_(ops.sample_params_words(1.0, top_k=1, seed=11))
        ops.decode_sample(xd, nxt, prm, s["out_ids"], s["step"], s["finished"], eos, PAD, *tail)
    else:
        slot = STEP if s["step"] is not None else [0] * B  # the label the scorer reads: slot step[b]; the other slots hold another (valid) token
        labels = torch.tensor([[amax[b] if j == slot[b] else (amax[b] + 1) % xd.shape[1] for j in range(LABEL_CAP)] for b in range(B)], dtype=torch.int64).cuda()
        bufs["nll"], nll = banded((B, LABEL_CAP), -1.0, torch.float32)
        bufs["top1"], top1 = banded((B, LABEL_CAP), -9, torch.int64)
        ops.decode_score(xd, nxt, labels, nll, top1, s["out_ids"], s["step"], s["finished"], PAD, *tail)
    torch.cuda.synchronize()
    got = {k: (None if v is None else v.cpu()) for k, v in s.items() if k != "decision"}
    got["next_ids"] = nxt.cpu()
    return got, {k: v.cpu() for k, v in bufs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("drop", list(DROPS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_three_entries_close_a_step_alike(name, drop):
    from dynamic_llava_amd import hip_ops as ops

    ops.require_gpu()
    dtype, V, stride, _, _ = CONFIGS[name]
    x, amax, eos = table(name)
    xd = torch.zeros((B, stride), dtype=dtype, device="cuda")[:, :V]
    xd.copy_(x)
    assert xd.stride(0) == stride
    for entry in ("advance", "sample", "score"):
        want = expected(x, (-1, -1, -1) if entry == "score" else eos, DROPS[drop])
        (got, bufs), (again, bufs2) = run(ops, entry, xd, amax, eos, DROPS[drop]), run(ops, entry, xd, amax, eos, DROPS[drop])
        for k in ("next_ids", "out_ids", "step", "finished", "kv_full", "kv_sparse"):
            tag = f"{name} {drop} {entry} {k}"
            if want[k] is None:
                assert got[k] is None, tag
                continue
            print(f"{tag}: got {got[k].flatten().tolist()} want {want[k].flatten().tolist()}")
            assert torch.equal(got[k].to(want[k].dtype), want[k]), tag
            assert torch.equal(got[k], again[k]), tag + " (second launch)"
        for k, fill in (("out_ids", -7), ("nll", -1.0), ("top1", -9)):
            if k in bufs:
                assert bool((bufs[k][:G] == fill).all()) and bool((bufs[k][-G:] == fill).all()), f"{name} {drop} {entry}: guard band of {k}"
                assert torch.equal(bufs[k], bufs2[k]), f"{name} {drop} {entry} {k} (second launch)"
        if entry == "score":  # the slot of a live row holds the row's top1 and a finite nll; every other slot keeps its sentinel
            nll, top1 = bufs["nll"][G:-G].view(B, LABEL_CAP), bufs["top1"][G:-G].view(B, LABEL_CAP)
            for b in range(B):
                slot = STEP[b] if "step" not in DROPS[drop] else 0
                live = not FIN[b] or "finished" in DROPS[drop]
                assert top1[b].tolist() == [amax[b] if (live and j == slot) else -9 for j in range(LABEL_CAP)], (name, drop, b)
                assert all((bool(torch.isfinite(nll[b, j])) and float(nll[b, j]) >= 0.0) if (live and j == slot) else float(nll[b, j]) == -1.0 for j in range(LABEL_CAP)), (name, drop, b)
