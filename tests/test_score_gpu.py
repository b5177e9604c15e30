"""GPU: the device scorer (dl_decode_score, through the C ABI) against the rule in dynamic_llava_amd/scoring.py.

Tolerance.  Kernel and host rule see the same logits: the maximum, top1, the label's logit and both subtractions are exact in both, so the two can
differ only through their exponentials and logarithms (device expf / logf: 1 ulp each in the HIP math API's single-precision table; torch's CPU exp / log
are within the same).  Per element, with lse_ref / nll_ref the host rule's values (score_cases.device_tol):

    tol = (2 * 2^-23 + V * 2^-40 + 2^-23) + 2 * ulp32(lse_ref) + ulp32(nll_ref)

two exponentials on the summed masses, one floor unit per token relative to M >= 2^40, the fp32 rounding of M, the two logarithms, the final addition.
Everything that is an integer (top1, tokens, steps, lengths) and every comparison between two launch forms is exact."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import score_cases as cs  # noqa: E402
from dynamic_llava_amd import scoring as sc  # noqa: E402

PAD = 3


def _state(B, cap, dev, step0=0, fin=None):
    return dict(next=torch.full((B,), -5, dtype=torch.int64, device=dev), out=torch.full((B, cap), -7, dtype=torch.int64, device=dev),
                step=torch.full((B,), step0, dtype=torch.int32, device=dev), fin=torch.zeros(B, dtype=torch.int32, device=dev) if fin is None else fin.clone().to(dev),
                full=torch.full((B,), 100, dtype=torch.int32, device=dev), sparse=torch.full((B,), 50, dtype=torch.int32, device=dev))


def _launch(logits_dev, labels, steps, decision=None, want_top1=True):
    """`steps` launches on the same logits (the kernel advances `step` itself) -> nll, top1, state (all on the CPU)."""
    from dynamic_llava_amd import hip_ops as ops

    B = logits_dev.shape[0]
    dev = logits_dev.device
    cap = labels.shape[1]
    lab = labels.to(dev).contiguous()
    nll = torch.full((B, cap), -1.0, dtype=torch.float32, device=dev)
    top1 = torch.full((B, cap), -9, dtype=torch.int64, device=dev) if want_top1 else None
    st = _state(B, cap, dev)
    for _ in range(steps):
        ops.decode_score(logits_dev, st["next"], lab, nll, top1, st["out"], st["step"], st["fin"], PAD, st["full"], st["sparse"], decision)
    torch.cuda.synchronize()
    return nll.cpu(), (top1.cpu() if want_top1 else None), {k: v.cpu() for k, v in st.items()}


def _batch(V, dtype, B, name):
    """[B, V]: row b is family `name` drawn with seed b; labels [B, 4]: four of (argmax, minimum, 0, V - 1, random), rotating with the row."""
    rows, labs = [], []
    for b in range(B):
        row = dict(cs.families(V, dtype, seed=b))[name]
        five = cs.labels_for(row, seed=b)
        rows.append(row)
        labs.append([five[(b + j) % 5] for j in range(4)])
    return torch.stack(rows), torch.tensor(labs, dtype=torch.int64)


def _close(got, ref, lse_ref, V):
    if torch.isinf(ref):
        return bool(got == ref)
    return abs(float(got) - float(ref)) <= cs.device_tol(V, float(lse_ref), float(ref))


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", cs.VOCABS)
def test_kernel_matches_the_rule(V, dtype):
    """Every family at B in {1, 3, 32}: 4 launches on the same logits walk a 4-column label block."""
    from dynamic_llava_amd import hip_ops as ops

    worst = 0.0
    names = [n for n, _ in cs.families(V, dtype)]
    for B in (1, 3, 32):
        for name in names:
            x, labels = _batch(V, dtype, B, name)
            xd = x.cuda()
            dec = torch.tensor([b % 2 for b in range(B)], dtype=torch.int32).cuda()
            nll, top1, st = _launch(xd, labels, 4, decision=dec)
            greedy = ops.decode_advance(xd, torch.zeros(B, dtype=torch.int64, device="cuda")).cpu()
            for b in range(B):
                ref, t_ref, lse = sc.reference_row_labels(x[b], labels[b])
                assert top1[b].tolist() == [t_ref] * 4 and int(greedy[b]) == t_ref, (name, B, b)
                for j in range(4):
                    assert _close(nll[b, j], ref[j], lse, V), (name, B, b, j, float(nll[b, j]), float(ref[j]), cs.device_tol(V, float(lse), float(ref[j])))
                    if torch.isfinite(ref[j]):
                        worst = max(worst, abs(float(nll[b, j]) - float(ref[j])) / cs.device_tol(V, float(lse), float(ref[j])))
            assert torch.equal(st["next"], labels[:, 3]) and torch.equal(st["out"], labels)
            assert st["step"].tolist() == [4] * B and st["fin"].tolist() == [0] * B
            assert st["full"].tolist() == [104] * B and st["sparse"].tolist() == [50 + 4 * (b % 2) for b in range(B)]
        # without `decision` every step keeps its token; without top1 nothing else changes
        nll2, _, st2 = _launch(xd, labels, 4, decision=None, want_top1=False)
        assert torch.equal(nll2.view(torch.int32), nll.view(torch.int32)) and st2["sparse"].tolist() == [54] * B and st2["full"].tolist() == [104] * B
    print(f"V={V} {dtype}: worst |kernel - rule| / tol = {worst:.3f}")


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", [320, 32000, 32003, 65536])
def test_same_bits_whatever_the_launch_form(V, dtype):
    """Row b of a 32-row launch, its own 1-row launch, a launch on an odd row stride, one on a base pointer one element off a 16-byte boundary (both scalar-load
    routes) and a second run: the same bits."""
    B = 32
    bits = lambda t: t.view(torch.int32)
    for name in ("gauss6", "neginf"):
        x, labels = _batch(V, dtype, B, name)
        xd = x.cuda()
        nll, top1, _ = _launch(xd, labels, 4)
        again, top1_again, _ = _launch(xd, labels, 4)
        assert torch.equal(bits(nll), bits(again)) and torch.equal(top1, top1_again)
        for b in range(B):
            one, t_one, _ = _launch(xd[b : b + 1], labels[b : b + 1], 4)
            assert torch.equal(bits(one[0]), bits(nll[b])) and torch.equal(t_one[0], top1[b]), (name, b)
        wide = torch.zeros((B, V + 1), dtype=dtype, device="cuda")
        wide[:, :V] = xd
        strided = wide[:, :V]
        assert strided.stride(0) == V + 1
        s_nll, s_top1, _ = _launch(strided, labels, 4)
        assert torch.equal(bits(s_nll), bits(nll)) and torch.equal(s_top1, top1), name
        flat = torch.zeros(B * V + 1, dtype=dtype, device="cuda")
        off = flat[1:].view(B, V)
        off.copy_(xd)
        assert off.data_ptr() % 16 != 0
        o_nll, o_top1, _ = _launch(off, labels, 4)
        assert torch.equal(bits(o_nll), bits(nll)) and torch.equal(o_top1, top1), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_exhausted_rows(dtype):
    """A label of -100, a label >= V written straight into the device buffer, step >= label_cap and a row that was finished already all behave the same way:
    finished set, pad_id emitted, the nll / top1 slots keep their sentinel, the lengths advance as dl_decode_advance advances a finished row's; the live row in the
    same launch is scored.  Guard bands around nll, top1 and out_ids stay intact."""
    from dynamic_llava_amd import hip_ops as ops

    V, B, cap, G = 32003, 5, 4, 64
    x = torch.stack([dict(cs.families(V, dtype, seed=b))["gauss6"] for b in range(B)])
    xd = x.cuda()
    labels = torch.tensor([[-100, 5, 5, 5], [5, V + 5, 5, 5], [5, 5, 5, 5], [5, 5, 5, 5], [5, 7, 5, 5]], dtype=torch.int64).cuda()
    step0 = torch.tensor([0, 1, cap, 1, 1], dtype=torch.int32)
    fin0 = torch.tensor([0, 0, 0, 1, 0], dtype=torch.int32)

    def banded(fill, dt):
        buf = torch.full((G + B * cap + G,), fill, dtype=dt, device="cuda")
        return buf, buf[G : G + B * cap].view(B, cap)

    nll_buf, nll = banded(-1.0, torch.float32)
    top_buf, top1 = banded(-9, torch.int64)
    out_buf, out = banded(-7, torch.int64)
    st = _state(B, cap, "cuda")
    st["step"].copy_(step0)
    st["fin"].copy_(fin0)
    dec = torch.tensor([1, 0, 1, 0, 0], dtype=torch.int32).cuda()
    ops.decode_score(xd, st["next"], labels, nll, top1, out, st["step"], st["fin"], PAD, st["full"], st["sparse"], dec)
    # the same rows through dl_decode_advance, all of them finished: what the bookkeeping of a finished row is
    ref = _state(B, cap, "cuda")
    ref["step"].copy_(step0)
    ref["fin"].fill_(1)
    ops.decode_advance(xd, ref["next"], ref["out"], ref["step"], ref["fin"], -1, PAD, ref["full"], ref["sparse"], dec)
    torch.cuda.synchronize()
    dead = [0, 1, 2, 3]
    assert st["fin"].cpu().tolist() == [1, 1, 1, 1, 0]
    assert st["next"].cpu().tolist() == [PAD] * 4 + [7]
    for k in ("step", "full", "sparse"):
        assert torch.equal(st[k].cpu(), ref[k].cpu()), k
    assert torch.equal(out.cpu()[dead], ref["out"].cpu()[dead]) and out.cpu()[4].tolist() == [-7, 7, -7, -7]
    assert bool((nll.cpu()[dead] == -1.0).all()) and bool((top1.cpu()[dead] == -9).all())
    want, t_ref, lse = sc.reference_row_labels(x[4], [7])
    assert _close(nll.cpu()[4, 1], want[0], lse, V) and int(top1.cpu()[4, 1]) == t_ref
    assert nll.cpu()[4].tolist().count(-1.0) == 3 and top1.cpu()[4].tolist().count(-9) == 3
    for buf, fill in ((nll_buf, -1.0), (top_buf, -9), (out_buf, -7)):
        assert bool((buf[:G] == fill).all()) and bool((buf[-G:] == fill).all())


def test_argument_rejection():
    """Return codes, not faults: the checks come before any launch."""
    from dynamic_llava_amd import hip_ops

    lib = hip_ops.load_library()
    p = ctypes.c_void_p(16)  # never dereferenced
    args = lambda V, labels=p, nll=p: (p, hip_ops.DL_BF16, V, V, 1, labels, 4, nll, None, p, None, 0, None, None, 0, None, None, None, None)
    assert lib.dl_decode_score(*args(65537)) != 0 and b"65536" in lib.dl_last_error()
    assert lib.dl_decode_score(*args(32000, labels=None)) != 0
    assert lib.dl_decode_score(*args(32000, nll=None)) != 0
    with pytest.raises(hip_ops.HipOpsError):
        hip_ops.decode_score(torch.zeros((1, 320), device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), None, torch.zeros((1, 4), device="cuda"))
