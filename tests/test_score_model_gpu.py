"""GPU, model level: model.score() -- teacher-forced NLL inside the captured decode graphs (dl_decode_score) -- against the reference's own numbers
(the fp32 goldens' step logits and forced tokens), against the forward() loop that was the only route before, over ragged batches, the weight / cache
formats, and next to greedy and sampled generate() calls on the same model.

Tolerances.  `tol` is score_cases.device_tol (kernel against the host rule on the same logits):
    tol = (2 * 2^-23 + V * 2^-40 + 2^-23) + 2 * ulp32(lse_ref) + ulp32(nll_ref).
Against a golden the logits themselves are only known to 1e-3 (the project's literal fp32 logit bound); log-sum-exp and the label's logit are each
1-Lipschitz in the sup norm, so the cross-entropy moves by at most 2 * 1e-3: bound = 2 * 1e-3 + tol."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import score_cases as cs  # noqa: E402
from oracle import fixtures as fx  # noqa: E402
from oracle.make_golden import CASES, SD_SEED, case_config  # noqa: E402

from dynamic_llava_amd import scoring as sc  # noqa: E402

# golden cases whose kept image-token set is tie-dependent (test_forward_loop_vs_reference_golden checks those with a tie-aware invariant instead of the
# golden's values): their downstream logits need not be the golden's, so they are not scored against it.  (Today every such case is a 16-bit one.)
TIES = sorted(n for n in CASES if "ties" in n)
# batched goldens: the reference's B > 1 decode zero-pads the rows that evicted a token and attends the pad slots (SURVEY finding 2; oracle/ref_cpu.py), so its
# numbers stop being per-row quantities at the first step where the rows' decisions differ (tiny_fp32_b3_same: step 5 of 9).  This project keeps true per-row
# lengths and defines batch parity per row against the B = 1 reference (test_batched_ragged_rows_equal_their_b1_runs; test_forward_loop_vs_reference_golden
# leaves the batched goldens out for the same reason).  The case's inputs are scored below against three B = 1 oracle runs instead, under the same bound.
BATCHED = sorted(n for n in CASES if len(CASES[n]["prompts"]) > 1)
SKIP = {**{n: "kept image-token set is tie-dependent" for n in TIES}, **{n: "the reference's B > 1 decode attends zero-padded KV slots" for n in BATCHED}}
GOLDEN = sorted(n for n in CASES if CASES[n]["dtype"] == "float32" and not CASES[n].get("nocache") and not CASES[n].get("rounds") and n not in SKIP
                and "forced" in np.load(os.path.join(os.path.dirname(__file__), "golden", n + ".npz")).files)


def _build(cfg_ns, sd, clip, dtype):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig

    return build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg_ns), sd, clip.state_dict() if clip is not None else None, dtype=dtype, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lens(pkv):
    return torch.as_tensor(pkv[1][0]).clone(), torch.as_tensor(pkv[1][-1]).clone()


def _forward_loop(model, ids, labels, pad=0, **inp):
    """The route that was the only one before: forward the prompt, then feed labels[:, j] (pad where a row has none) one token at a time.
    -> fp32 logits [T, B, V] (step j: after prompt + labels[:, :j]) and the two KV length vectors after T - 1 fed tokens."""
    out = model(ids, **inp)
    pkv = out.past_key_values
    last = torch.as_tensor(pkv[1][-1]).to(ids.device).long() - 1  # rows of different length are right-padded: the last VALID position
    logits = [out.logits[torch.arange(ids.shape[0], device=ids.device), last].float().clone()]
    feed = torch.where(labels >= 0, labels, torch.full_like(labels, pad)).to(ids.device)
    for j in range(labels.shape[1] - 1):
        out = model(feed[:, j : j + 1], past_key_values=pkv)
        pkv = out.past_key_values
        logits.append(out.logits[:, -1].float().clone())
    torch.cuda.synchronize()
    model.check_device_errors()
    return torch.stack(logits), _lens(pkv)


def _check_against_rule(res, logits, labels, what, own=None):
    """res["nll"] / ["top1"] within tol of the host rule on `logits` [T, B, V] (the forward loop's); exact zeros / -1 where there is no label; n_labels and ppl
    consistent.
    own: the logits the call itself reports (output_logits=True).  Where a row of them is not bit-equal to the loop's -- the prompt's last position of a batch of
    two or three rows: generate() runs that one vocabulary projection on dl_gemv, forward() on the library GEMM over all positions, two fp32 summation orders --
    the loop's logits are the kernel's inputs only to within d = max |own - loop|, which must stay inside the project's fp32 logit bound (1e-3); log-sum-exp and
    the label's logit are each 1-Lipschitz in the sup norm, so the bound there is tol + 2 d, and top1 is taken from the logits the kernel saw."""
    nll, top1 = res["nll"].cpu(), res["top1"].cpu()
    B, T = labels.shape
    V = logits.shape[-1]
    worst, widened = 0.0, []
    for b in range(B):
        for j in range(T):
            if int(labels[b, j]) < 0:
                assert float(nll[b, j]) == 0.0 and int(top1[b, j]) == -1, (what, b, j)
                continue
            ref, t_ref, det = sc.reference_step(logits[j, b].cpu(), int(labels[b, j]))
            tol = cs.device_tol(V, float(det["lse"]), float(ref))
            if own is not None and not torch.equal(_bits(own[j, b]), _bits(logits[j, b])):
                d = float((own[j, b] - logits[j, b]).abs().max())
                assert d <= 1e-3, (what, b, j, d)
                widened.append((j, b, d))
                tol += 2 * d
                t_ref = sc.reference_step(own[j, b].cpu(), int(labels[b, j]))[1]
            err = abs(float(nll[b, j]) - float(ref))
            worst = max(worst, err / tol)
            assert err <= tol and int(top1[b, j]) == t_ref, (what, b, j, float(nll[b, j]), float(ref), tol, int(top1[b, j]), t_ref)
    n = (labels >= 0).sum(dim=1)
    assert torch.equal(res["n_labels"].cpu(), n)
    ppl = torch.exp(nll.double().sum(dim=1) / n.double())
    assert torch.allclose(res["ppl"].cpu().double(), ppl, rtol=1e-5, atol=0.0), (what, res["ppl"], ppl)  # (fp32 sum / exp of at most a few dozen terms)
    print(f"{what}: worst |nll - rule| / tol = {worst:.3f}; (step, row, max |logit difference|) where the loop's logits are not the call's own: {widened or 'none'}")
    return widened


# ---------------------------------------------------------------- the reference's own numbers
@pytest.mark.parametrize("name", GOLDEN)
def test_score_against_the_reference_goldens(name, golden_dir):
    c = CASES[name]
    cfg = case_config(c)
    sd = fx.make_state_dict(cfg, seed=SD_SEED, predictor_gain=c["gain"])
    clip = fx.build_clip(cfg, seed=1)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    model = _build(cfg, sd, clip, torch.float32)
    ids = torch.from_numpy(g["input_ids"]).cuda()
    images = fx.make_images(cfg, ids.shape[0], seed=0).cuda()
    forced = torch.from_numpy(g["forced"]).long()  # [T, B]
    T, B = forced.shape
    assert g["step_logits"].shape[0] == T
    res = model.score(ids, forced.t().contiguous(), images=images)
    torch.cuda.synchronize()
    model.check_device_errors()
    nll = res["nll"].cpu()
    worst = 0.0
    for j in range(T):
        x = torch.from_numpy(g["step_logits"][j]).double()
        ce = -torch.log_softmax(x, dim=-1)[torch.arange(B), forced[j]]
        lse = torch.logsumexp(x - x.max(dim=-1, keepdim=True).values, dim=-1)
        for b in range(B):
            bound = 2 * 1e-3 + cs.device_tol(x.shape[-1], float(lse[b]), float(ce[b]))
            err = abs(float(nll[b, j]) - float(ce[b]))
            worst = max(worst, err)
            assert err <= bound, (name, j, b, float(nll[b, j]), float(ce[b]), bound)
    first, last = _lens(res["past_key_values"])
    np.testing.assert_array_equal(first.numpy(), g["len_first"][T - 1])
    np.testing.assert_array_equal(last.numpy(), g["len_last"][T - 1])
    assert int(first.max()) == int(g["kv_len_first"][T - 1]) and int(last.max()) == int(g["kv_len_last"][T - 1])
    assert res["n_labels"].tolist() == [T] * B
    print(f"[{name}] max |nll - golden cross-entropy| = {worst:.2e}")


@pytest.mark.parametrize("name", [n for n in BATCHED if CASES[n]["dtype"] == "float32" and not CASES[n].get("nocache")])
def test_score_of_a_batched_golden_case_against_the_b1_reference_of_every_row(name, golden_dir):
    """The batched golden's inputs (prompts, images, forced tokens); every row against its own B = 1 run of the oracle (pinned to the reference), bound
    2 * 1e-3 + tol as above; both KV lengths of every row equal that run's."""
    from oracle.ref_cpu import Oracle

    c = CASES[name]
    cfg = case_config(c)
    sd = fx.make_state_dict(cfg, seed=SD_SEED, predictor_gain=c["gain"])
    clip = fx.build_clip(cfg, seed=1)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    model = _build(cfg, sd, clip, torch.float32)
    ids = torch.from_numpy(g["input_ids"])
    images = fx.make_images(cfg, ids.shape[0], seed=0)
    forced = torch.from_numpy(g["forced"]).long()  # [T, B]
    T, B = forced.shape
    res = model.score(ids.cuda(), forced.t().contiguous(), images=images.cuda())
    torch.cuda.synchronize()
    model.check_device_errors()
    nll = res["nll"].cpu()
    first, last = _lens(res["past_key_values"])
    worst = 0.0
    for b in range(B):
        o = Oracle(cfg, sd, torch.float32, clip=clip)
        with torch.no_grad():
            l, p = o.forward(ids[b : b + 1], images=images[b : b + 1])
            for j in range(T):
                x = l[0, -1].double()
                ce = float(-torch.log_softmax(x, dim=-1)[forced[j, b]])
                lse = float(torch.logsumexp(x - x.max(), dim=-1))
                err = abs(float(nll[b, j]) - ce)
                worst = max(worst, err)
                assert err <= 2 * 1e-3 + cs.device_tol(x.shape[-1], lse, ce), (name, b, j, float(nll[b, j]), ce)
                if j + 1 < T:
                    l, p = o.forward(forced[j, b : b + 1][:, None], past_key_values=p)
        assert int(p[1][0][0]) == int(first[b]) and int(p[1][-1][0]) == int(last[b]), (name, b)
    print(f"[{name}] max |nll - B = 1 reference cross-entropy| = {worst:.2e}")


# ---------------------------------------------------------------- the 7B-width slice, bf16, B = 1
@pytest.fixture(scope="module")
def slice7b():
    """LLaVA-1.5-7B layer width (H = 4096, I = 11008), 3 layers, sparse_layer = 2, a 2048-word vocabulary: test_pack_model_gpu's configuration.  Batch 1
    runs the fused q|k|v + attention launch, dl_gemv_gu_tp and the packed streams (dl_gemv_pk)."""
    cfg = fx.llava7b_config(num_hidden_layers=3)
    cfg.vocab_size = 2048
    sd = fx.make_state_dict(cfg, seed=7, predictor_gain=50.0)
    model = _build(cfg, sd, None, torch.bfloat16)
    g = torch.Generator().manual_seed(21)
    feats = torch.randn(1, 576, 4096, generator=g).to(torch.bfloat16).cuda()
    ids = fx.make_prompt(cfg, 35, 20, seed=4)[None].cuda()
    return cfg, model, feats, ids


T_SLICE = 12


def _n_captured(model):
    return len(model._dstate.graphs), len(model._prefill_graphs), sum(e["graph"] is not None for e in model._prefill_graphs.values())


def test_score_against_the_forward_loop_on_the_slice(slice7b):
    cfg, model, feats, ids = slice7b
    labels = fx.make_forced_tokens(cfg, T_SLICE, 1, seed=6).t().contiguous()
    loop, loop_lens = _forward_loop(model, ids, labels, image_features=feats)
    step = model.score(ids, labels, image_features=feats, output_logits=True)
    torch.cuda.synchronize()
    model.check_device_errors()
    got = torch.stack(step["logits"])
    assert got.shape == loop.shape and got.dtype == torch.float32
    diff = [float((got[j] - loop[j]).abs().max()) for j in range(T_SLICE)]
    print("max |score logits - forward-loop logits| per step:", " ".join(f"{d:.3g}" for d in diff))
    assert torch.equal(_bits(got), _bits(loop)), diff
    _check_against_rule(step, loop, labels, "slice, step by step")
    first, last = _lens(step["past_key_values"])
    assert torch.equal(first, loop_lens[0]) and torch.equal(last, loop_lens[1])
    # the plain call: chunks of graph replays; then once more, nothing but replays
    plain = model.score(ids, labels, image_features=feats)
    assert "logits" not in plain and torch.equal(_bits(plain["nll"]), _bits(step["nll"])) and torch.equal(plain["top1"], step["top1"])
    again = model.score(ids, labels, image_features=feats)
    assert torch.equal(_bits(again["nll"]), _bits(step["nll"]))
    assert all(torch.equal(a, b) for a, b in zip(_lens(again["past_key_values"]), loop_lens))
    # other labels of the same length are device data: the same graphs serve them
    before = _n_captured(model)
    assert before[0] >= 1 and before[2] >= 1
    other = fx.make_forced_tokens(cfg, T_SLICE, 1, seed=7).t().contiguous()
    res = model.score(ids, other, image_features=feats)
    torch.cuda.synchronize()
    model.check_device_errors()
    assert _n_captured(model) == before
    assert not torch.equal(res["nll"], step["nll"])
    loop2, lens2 = _forward_loop(model, ids, other, image_features=feats)
    _check_against_rule(res, loop2, other, "slice, other labels")
    assert all(torch.equal(a, b) for a, b in zip(_lens(res["past_key_values"]), lens2))


@pytest.mark.parametrize("mode", ["no_pack", "mxfp8_kv", "mxfp8_weights"])
def test_score_in_every_decode_mode(slice7b, mode):
    """One short run per mode, against the forward loop in the same mode (MXFP8 weights last: that format rewrites the parameters for good)."""
    cfg, model, feats, ids = slice7b
    labels = fx.make_forced_tokens(cfg, 5, 1, seed=8).t().contiguous()
    try:
        if mode == "mxfp8_weights":
            model.set_decode_weight_format("mxfp8")
        elif mode == "mxfp8_kv":
            model.set_kv_cache_format("mxfp8")
        else:
            model.decode_weight_pack = False
            model._packed = False
            model.finalize()
        loop, lens = _forward_loop(model, ids, labels, image_features=feats)
        res = model.score(ids, labels, image_features=feats)
        torch.cuda.synchronize()
        model.check_device_errors()
        _check_against_rule(res, loop, labels, mode)
        assert all(torch.equal(a, b) for a, b in zip(_lens(res["past_key_values"]), lens))
    finally:
        if mode == "mxfp8_weights":
            model.set_decode_weight_format(None)
        elif mode == "mxfp8_kv":
            model.set_kv_cache_format(None)
        else:
            model.decode_weight_pack = True
            model._packed = False
            model.finalize()


# ---------------------------------------------------------------- the tiny model: ragged batches, mode leakage, validation
@pytest.fixture(scope="module")
def tiny():
    c = CASES["tiny_fp32_b1_gain50"]
    cfg = case_config(c)
    sd = fx.make_state_dict(cfg, seed=SD_SEED, predictor_gain=c["gain"])
    clip = fx.build_clip(cfg, seed=1)
    return cfg, _build(cfg, sd, clip, torch.float32)


def _tiny_inputs(cfg, B):
    ids = torch.stack([fx.make_prompt(cfg, 5, 7, seed=10 + b) for b in range(B)]).cuda()
    return ids, fx.make_images(cfg, B, seed=3).cuda()


@pytest.mark.parametrize("B", [3, 8])
def test_ragged_batch(tiny, B):
    """Label counts (T, T - 3, 1, ...) padded with -100.  Against the rule on the batched forward loop's logits, bound tol -- except at step 0 of the 3-row
    batch, whose logits the two routes compute in different fp32 summation orders (see _check_against_rule: measured there, nll 4.7244596 against the rule's
    4.7244611 on the loop's logits, tol 1.31e-6); every decode step must see the loop's bits."""
    cfg, model = tiny
    T = 7
    ids, images = _tiny_inputs(cfg, B)
    labels = fx.make_forced_tokens(cfg, T, B, seed=B).t().contiguous()
    counts = [T, T - 3, 1] + [1 + (3 * b) % T for b in range(3, B)]
    for b, n in enumerate(counts):
        labels[b, n:] = -100
    pad = model.config.pad_token_id or 0
    loop, _ = _forward_loop(model, ids, labels, pad=pad, images=images)
    res = model.score(ids, labels, images=images, output_logits=True)
    plain = model.score(ids, labels, images=images)
    torch.cuda.synchronize()
    model.check_device_errors()
    assert res["n_labels"].tolist() == counts
    assert torch.equal(_bits(plain["nll"]), _bits(res["nll"])) and torch.equal(plain["top1"], res["top1"])
    widened = _check_against_rule(res, loop, labels, f"ragged B={B}", own=torch.stack(res["logits"]))
    assert all(j == 0 for j, _, _ in widened), widened  # every decode step is the forward loop's own launch sequence: the same bits


def test_no_leakage_between_modes(tiny):
    cfg, model = tiny
    ids, images = _tiny_inputs(cfg, 1)
    labels = fx.make_forced_tokens(cfg, 6, 1, seed=2).t().contiguous()

    def greedy():
        out = model.generate(ids, images=images, max_new_tokens=6, eos_token_id=None)
        return out.clone(), model.last_prefill_logits.clone(), [t.clone() for t in _lens(model.last_cache)]

    def sampled():
        return model.generate(ids, images=images, max_new_tokens=6, eos_token_id=None, do_sample=True, seed=11, temperature=0.9, top_k=40, top_p=0.95).clone()

    s0 = sampled()  # before any scoring
    g1 = greedy()
    r1 = model.score(ids, labels, images=images)
    g2 = greedy()
    s1 = sampled()
    r2 = model.score(ids, labels, images=images)
    torch.cuda.synchronize()
    model.check_device_errors()
    assert torch.equal(g1[0], g2[0]) and torch.equal(_bits(g1[1]), _bits(g2[1])) and all(torch.equal(a, b) for a, b in zip(g1[2], g2[2]))
    assert torch.equal(_bits(r1["nll"]), _bits(r2["nll"])) and torch.equal(r1["top1"], r2["top1"]) and torch.equal(r1["ppl"], r2["ppl"])
    assert torch.equal(s0, s1)
    assert int(r1["top1"][0, 0]) == int(g1[0][0, 0])  # step 0 sees the prompt alone: its greedy token is generate()'s first


def test_validation_before_any_launch(tiny):
    cfg, model = tiny
    ids, images = _tiny_inputs(cfg, 2)
    V = cfg.vocab_size
    for bad in (torch.tensor([[3, -100, 4], [3, 4, 5]]), torch.tensor([[3, V, 4], [3, 4, 5]]), torch.tensor([[3, 4, 5]]), torch.tensor([[-100, 4, 5], [3, 4, 5]])):
        with pytest.raises(ValueError):
            model.score(ids, bad, images=images)
    with pytest.raises(NotImplementedError, match="score"):
        model(ids, images=images, labels=torch.zeros_like(ids))
