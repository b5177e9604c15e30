"""GPU: the logits-processor kernel (dl_logits_process, through ops.logits_process) against the rule in dynamic_llava_amd/logits_rules.py.

Everything is compared as bits (`out.view(torch.int32)`), so -0.0 counts: the kernel's only arithmetic is one fp32 multiplication or one correctly
rounded fp32 division per edited entry, which the rule performs with the same operands; there is no tolerance to state."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import logits_rules as lr  # noqa: E402
from dynamic_llava_amd import sampling as sp  # noqa: E402

NEG = float("-inf")
SEED = 20261019


def _bits(t):
    return t.contiguous().view(torch.int32)


def _alphabet(V, g):
    """A handful of ids spread over the vocabulary (its first and last id included): histories over it repeat tokens and n-grams."""
    return [0, V - 1] + torch.randint(1, V - 1, (4,), generator=g).tolist()


def _logits(B, V, dtype, g, alpha):
    x = (torch.randn(B, V, generator=g) * 8).to(dtype)
    x[0, alpha[0]], x[0, alpha[1]], x[0, alpha[2]], x[0, alpha[3]] = NEG, -0.0, 0.0, 3.0e4  # hard values where the history points
    return x


def _history(B, cap, alpha, g):
    return torch.tensor(alpha)[torch.randint(0, len(alpha), (B, cap), generator=g)].to(torch.int64)


def _launch(x_dev, p, n, words, out_ids=None, step=None, out=None, no_table=False):
    from dynamic_llava_amd import hip_ops as ops

    B, V = x_dev.shape
    dev = x_dev.device
    prm = ops.logits_params_block(dev)
    prm.copy_(ops.logits_params_words(p, n, 0 if no_table else len(words)))
    tab = None if no_table else ops.bad_words_table(words, dev)
    out = torch.full((B, V), 123.0, dtype=torch.float32, device=dev) if out is None else out
    ops.logits_process(x_dev, out, prm, out_ids, step, tab)
    torch.cuda.synchronize()
    return out


def _expect(x, p, n, words, out_ids=None, step=None):
    B = x.shape[0]
    cap = 0 if out_ids is None else out_ids.shape[1]
    hist = [[] if step is None or out_ids is None else out_ids[b, : min(max(int(step[b]), 0), cap)].tolist() for b in range(B)]
    return lr.process(x, hist, p, n, words)


def _words(alpha, hist_row):
    w = [[alpha[4]], [alpha[0], alpha[5]], [alpha[1], alpha[0], alpha[2]], [alpha[2], alpha[2], alpha[2], alpha[3]]]
    if len(hist_row) >= 2:
        w += [[hist_row[-1], 7], [hist_row[-2], hist_row[-1], 9]]
    return w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [320, 1003, 32000, 50000])
def test_kernel_matches_the_rule(V, dtype):
    """B in {1, 3, 32} x out_cap in {8, 64}, all three processors on, a different step per row drawn from {0, 1, n-2, n-1, n, out_cap, out_cap + 5}."""
    g = torch.Generator().manual_seed(SEED + V)
    for B in (1, 3, 32):
        for cap, n, p in ((8, 3, 1.3), (64, 5, 0.7)):
            alpha = _alphabet(V, g)
            x = _logits(B, V, dtype, g, alpha)
            ids = _history(B, cap, alpha, g)
            choices = [0, 1, n - 2, n - 1, n, cap, cap + 5]
            step = torch.tensor([choices[(b + B) % len(choices)] for b in range(B)], dtype=torch.int32)
            words = _words(alpha, ids[B - 1, : int(step[B - 1])].tolist())
            got = _launch(x.cuda(), p, n, words, ids.cuda(), step.cuda()).cpu()
            want = _expect(x, p, n, words, ids, step)
            assert torch.equal(_bits(got), _bits(want)), (B, cap, int((_bits(got) != _bits(want)).sum()))
            assert not torch.equal(_bits(want), _bits(x.float())), "the case edits something"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_vocabulary_id_is_edited(dtype):
    """The history is a permutation of all ids followed by repeats: every output element is a penalty (or ban) write, so every boundary between two
    workgroups' ranges is hit whatever the tile size."""
    V, cap = 1003, 1100
    g = torch.Generator().manual_seed(SEED)
    x = (torch.randn(2, V, generator=g) * 8).to(dtype)
    x[x == 0] = 1.0
    perm = torch.stack([torch.randperm(V, generator=g) for _ in range(2)])
    ids = torch.cat([perm, perm[:, : cap - V]], dim=1).to(torch.int64)
    step = torch.tensor([cap, cap], dtype=torch.int32)
    for p, n, words in ((1.3, 0, []), (0.5, 2, [[int(ids[0, -1]), 5], [6]]), (2.0, 1, [])):
        got = _launch(x.cuda(), p, n, words, ids.cuda(), step.cuda()).cpu()
        want = _expect(x, p, n, words, ids, step)
        assert torch.equal(_bits(got), _bits(want)), (p, n)
        assert bool((want != x.float()).all()), "every element is edited"


def test_collisions():
    """Penalty and ban on the same token give -inf; a token three times in the history is penalised once; an id outside [0, V) leaves the row otherwise correct."""
    V = 1003
    g = torch.Generator().manual_seed(SEED + 1)
    x = (torch.randn(1, V, generator=g) * 8).bfloat16()
    ids = torch.tensor([[10, 11, 10, 500, 500, V, -3, 2**32 + 11, 600, 500, 11]], dtype=torch.int64)  # (2**32 + 11 is not 11: a 32-bit compare would ban 600)
    step = torch.tensor([ids.shape[1]], dtype=torch.int32)
    words = [[10], [500, 11, 77], [11, 500, 78]]
    got = _launch(x.cuda(), 1.3, 2, words, ids.cuda(), step.cuda()).cpu()
    want = _expect(x, 1.3, 2, words, ids, step)
    assert torch.equal(_bits(got), _bits(want))
    xf = x.float()[0]
    one = lambda v: v * torch.tensor(1.3) if v < 0 else v / torch.tensor(1.3)
    assert got[0, 10] == NEG  # in the history (penalised), follows 11 (the 2-gram ban) and is a one-token word
    assert got[0, 77] == NEG and got[0, 78] == xf[78]  # the three-token word whose prefix is the history's tail, and the one whose prefix is not
    assert got[0, 500] == one(xf[500]) and got[0, 11] == one(xf[11]) and got[0, 600] == one(xf[600])  # 500 occurs three times: penalised once
    assert sorted((got[0] != xf).nonzero().flatten().tolist()) == [10, 11, 77, 500, 600]


def test_addressing_routes_agree_with_the_rule():
    """An odd row stride with V = 1003 (scalar loads and stores) and an aligned row with V = 32000 (16-byte loads and stores)."""
    g = torch.Generator().manual_seed(SEED + 2)
    for V, pad, dtype in ((1003, 4, torch.bfloat16), (1003, 4, torch.float32), (32000, 0, torch.bfloat16), (32000, 0, torch.float32), (32000, 8, torch.float16)):
        B, cap, n = 3, 16, 2
        alpha = _alphabet(V, g)
        store = (torch.randn(B, V + pad, generator=g) * 8).to(dtype).cuda()
        xd = store[:, :V]
        assert xd.stride(0) == V + pad
        ids = _history(B, cap, alpha, g)
        step = torch.tensor([16, 7, 3], dtype=torch.int32)
        words = _words(alpha, ids[0].tolist())
        got = _launch(xd, 1.3, n, words, ids.cuda(), step.cuda()).cpu()
        assert torch.equal(_bits(got), _bits(_expect(xd.cpu(), 1.3, n, words, ids, step))), (V, pad, dtype)


@pytest.mark.parametrize("V", [1003, 4096])
def test_guard_bands_and_inputs_stay_untouched(V):
    from dynamic_llava_amd import hip_ops as ops

    B, cap, pad, G = 3, 16, 24, 256
    g = torch.Generator().manual_seed(SEED + 3)
    alpha = _alphabet(V, g)
    store = (torch.randn(B, V + pad, generator=g) * 8).bfloat16().cuda()
    store0 = store.clone()
    buf = torch.full((G + B * V + G,), -777.0, dtype=torch.float32).cuda()
    out = buf[G : G + B * V].view(B, V)
    ids = _history(B, cap, alpha, g).cuda()
    step = torch.tensor([cap + 5, cap, 1], dtype=torch.int32).cuda()
    ids0, step0 = ids.clone(), step.clone()
    words = _words(alpha, ids[1].tolist())
    got = _launch(store[:, :V], 0.7, 3, words, ids, step, out=out)
    assert torch.equal(_bits(got.cpu()), _bits(_expect(store0[:, :V].cpu(), 0.7, 3, words, ids0.cpu(), step0.cpu())))
    sentinel = _bits(torch.full((G,), -777.0))
    assert torch.equal(_bits(buf[:G].cpu()), sentinel) and torch.equal(_bits(buf[G + B * V :].cpu()), sentinel)
    assert torch.equal(store.view(torch.int16), store0.view(torch.int16)) and torch.equal(ids, ids0) and torch.equal(step, step0)
    assert ops.bad_words_table(words, "cuda").shape == (lr.MAX_BAD_WORDS, 1 + lr.MAX_BAD_WORD_LEN)


def test_null_step_and_null_table():
    V, B, cap = 1003, 2, 8
    g = torch.Generator().manual_seed(SEED + 4)
    alpha = _alphabet(V, g)
    x = _logits(B, V, torch.bfloat16, g, alpha)
    ids = _history(B, cap, alpha, g)
    step = torch.tensor([8, 5], dtype=torch.int32)
    words = [[alpha[4]], [int(ids[0, -1]), 7]]
    # no step: the history is empty -- only the one-token word acts
    got = _launch(x.cuda(), 1.3, 1, words, ids.cuda(), None).cpu()
    want = x.float().clone()
    want[:, alpha[4]] = NEG
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(want), _bits(_expect(x, 1.3, 1, words)))
    got = _launch(x.cuda(), 1.3, 1, words, None, None).cpu()
    assert torch.equal(_bits(got), _bits(want))
    # no table: penalty and n-gram alone
    got = _launch(x.cuda(), 1.3, 2, words, ids.cuda(), step.cuda(), no_table=True).cpu()
    assert torch.equal(_bits(got), _bits(_expect(x, 1.3, 2, [], ids, step)))


def test_one_captured_graph_serves_every_setting_and_replays_repeat():
    from dynamic_llava_amd import hip_ops as ops

    V, B, cap = 32000, 3, 32
    g = torch.Generator().manual_seed(SEED + 5)
    alpha = _alphabet(V, g)
    x = _logits(B, V, torch.bfloat16, g, alpha)
    ids = _history(B, cap, alpha, g)
    step = torch.tensor([32, 9, 2], dtype=torch.int32)
    xd, idd, sd = x.cuda(), ids.cuda(), step.cuda()
    prm, tab = ops.logits_params_block("cuda"), ops.bad_words_table((), "cuda")
    out = torch.zeros((B, V), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.logits_process(xd, out, prm, idd, sd, tab)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.logits_process(xd, out, prm, idd, sd, tab)
    settings = [(1.0, 0, []), (1.3, 0, []), (1.0, 3, []), (0.7, 2, _words(alpha, ids[0].tolist())), (2.0, 1, [[alpha[5]]]), (1.0, 0, [])]
    for p, n, words in settings:
        prm.copy_(ops.logits_params_words(p, n, len(words)))
        tab.copy_(ops.bad_words_table(words, "cpu"))
        graph.replay()
        torch.cuda.synchronize()
        first = out.cpu()
        assert torch.equal(_bits(first), _bits(_expect(x, p, n, words, ids, step))), (p, n)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out.cpu()), _bits(first)), "two launches on the same inputs are bit-equal"
    a = _launch(xd, 0.7, 2, settings[3][2], idd, sd).cpu()
    b = _launch(xd, 0.7, 2, settings[3][2], idd, sd).cpu()
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_chained_with_the_bookkeeping_kernels(dtype):
    """dl_decode_advance on the processed row picks argmax(rule), the lowest index on ties; dl_decode_sample with a fixed seed draws what
    sampling.reference_step draws on the rule's row."""
    from dynamic_llava_amd import hip_ops as ops

    V, B, cap = 32000, 3, 16
    g = torch.Generator().manual_seed(SEED + 6)
    alpha = _alphabet(V, g)
    x = (torch.randn(B, V, generator=g) * 3).to(dtype)
    ids = _history(B, cap, alpha, g)
    step = torch.tensor([16, 6, 0], dtype=torch.int32)
    top = x.float().argmax(dim=1).tolist()
    ids[0, 3] = top[0]  # row 0: its raw argmax is in the history ...
    x[0, top[0]] = 40.0
    x[0, 20000] = x[0, 123] = 25.0  # ... and penalised below a tie of two, which the lowest index wins
    words = [[top[1]], [top[2]]]  # rows 1 and 2: their raw argmax is a bad word
    p, n = 2.0, 0
    xd, idd = x.cuda(), ids.cuda()
    want = _expect(x, p, n, words, ids, step)
    assert float(want[0].max()) == 25.0 and int(want[0].argmax()) != top[0]
    proc = _launch(xd, p, n, words, idd, step.cuda())
    assert torch.equal(_bits(proc.cpu()), _bits(want))
    nxt = torch.zeros(B, dtype=torch.int64, device="cuda")
    st_a, ids_a = step.cuda(), idd.clone()
    ops.decode_advance(proc, nxt, ids_a, st_a, None, -1, 0)
    torch.cuda.synchronize()
    lowest = [int((want[b] == want[b].max()).nonzero()[0]) for b in range(B)]
    assert nxt.cpu().tolist() == lowest and lowest[0] == 123 and lowest[1] != top[1] and lowest[2] != top[2]
    assert st_a.cpu().tolist() == [17, 7, 1] and int(ids_a[1, 6]) == lowest[1] and int(ids_a[2, 0]) == lowest[2]
    T, k, tp = 0.8, 20, 0.9
    for seed in (7, 8, 9):
        prm = ops.sample_params_block("cuda")
        prm.copy_(ops.sample_params_words(T, k, tp, seed, 0))
        st_s = step.cuda()
        ops.decode_sample(proc, nxt, prm, idd.clone(), st_s, None, -1, 0)
        torch.cuda.synchronize()
        ref = [sp.reference_step(want[b], T, k, tp, (), seed, b, int(step[b]))[0] for b in range(B)]
        assert nxt.cpu().tolist() == ref, seed
