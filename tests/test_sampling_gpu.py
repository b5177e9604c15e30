"""GPU: the device sampler (dl_decode_sample) against the rule in dynamic_llava_amd/sampling.py, and generate(do_sample=True, seed=...)
against the greedy path whose code it shares.

Tolerances.  top-k, the bookkeeping and everything that is an integer are compared exactly.  The top-p set and the draw depend on exp():
the kernel calls the device library's expf, whose documented maximum error is 1 ulp (HIP programming guide, "HIP math API", single
precision table: expf -- 1 ULP), i.e. a relative error d <= 2^-23 = 1.2e-7; torch's CPU exp is within the same bound.  With
eps = 2 * d + V * 2^-40 (both exps, plus one unit of the fixed-point floor per token, relative to M >= 2^40) a token whose class mass
S(z_v) exceeds thr + eps * M must be kept, one below thr - eps * M must be dropped, anything between may go either way -- at most 64
tokens per row may sit in that band.  The drawn token v must satisfy prefix_excl(v) - eps * K <= t <= prefix_incl(v) + eps * K, where
the prefix sums are the REFERENCE's masses over the kept set the device reported (which the two-sided check has just validated: where
the band is not empty the reference's own set is one of two admissible ones, and every prefix behind a band token depends on which),
and at most 1 draw in 1000 may need the margin."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dynamic_llava_amd import sampling as sp  # noqa: E402

GRID = [(0.2, 0, None), (0.7, 50, 0.9), (1.0, 0, 0.95), (1.5, 200, 0.8), (5.0, 0, 0.95), (1.0, 0, 0.5)]
SEED = 20261016
D_EXP = 2.0 ** -23
STEPS = 16


def _eps(V):
    return 2 * D_EXP + V * 2.0 ** -sp.S_BITS


def _logits(B, V, sigma, dtype, extra=0):
    g = torch.Generator().manual_seed(SEED + extra)
    return (torch.randn(B, V, generator=g) * sigma).to(dtype)


def _launch(logits_dev, T, k, p, seed, steps=STEPS, row_base=0, eos=-1, min_new=0, finished=None, pad=0, step0=0, want_mask=True, decision=None):
    """`steps` launches on the same logits (the kernel advances `step` itself): tokens [B, steps], kept mask of the last launch, state."""
    from dynamic_llava_amd import hip_ops as ops

    B, V = logits_dev.shape
    dev = logits_dev.device
    prm = ops.sample_params_block(dev)
    prm.copy_(ops.sample_params_words(T, k, p, seed, row_base))
    st = dict(next=torch.zeros(B, dtype=torch.int64, device=dev), out=torch.full((B, step0 + steps), -7, dtype=torch.int64, device=dev),
              step=torch.full((B,), step0, dtype=torch.int32, device=dev),
              fin=torch.zeros(B, dtype=torch.int32, device=dev) if finished is None else finished.clone(),
              full=torch.full((B,), 100, dtype=torch.int32, device=dev), sparse=torch.full((B,), 50, dtype=torch.int32, device=dev))
    mask = torch.zeros((B, V), dtype=torch.uint8, device=dev) if want_mask else None
    for _ in range(steps):
        ops.decode_sample(logits_dev, st["next"], prm, st["out"], st["step"], st["fin"], eos, pad, st["full"], st["sparse"], decision, min_new_tokens=min_new, kept_mask=mask)
    torch.cuda.synchronize()
    return st["out"][:, step0:].cpu(), (mask.cpu().bool() if want_mask else None), {k_: v.cpu() for k_, v in st.items()}


def _check_row(row_logits, T, k, p, banned, seed, row, toks, kept_dev, stats, row_base=0, step0=0):
    """Two-sided kept-set check and draw check of one row (see the module docstring)."""
    V = row_logits.shape[0]
    eps = _eps(V)
    _, kept_ref, det = sp.reference_step(row_logits, T, k, p, banned, seed, row, step0, row_base)
    topk = det["topk_mask"]
    if p is None:
        assert torch.equal(kept_dev, kept_ref), "kept set without top-p is exact"
    else:
        S, thr, M = det["S"].double(), float(det["thr"]), float(det["M"])
        must_keep = topk & (S > thr + eps * M)
        must_drop = ~topk | (S < thr - eps * M)
        assert bool(kept_dev[must_keep].all()) and not bool(kept_dev[must_drop].any())
        band = int((~must_keep & ~must_drop).sum())
        stats["band_max"] = max(stats["band_max"], band)
        assert band <= 64, band
    m = torch.where(kept_dev, det["m"], torch.zeros_like(det["m"]))
    prefix = torch.cumsum(m, 0)
    K = int(prefix[-1])
    assert K > 0
    for i, tok in enumerate(toks.tolist()):
        t = (sp.draw_r64(seed, row, step0 + i, row_base) * K) >> 64
        incl = int(prefix[tok])
        excl = incl - int(m[tok])
        stats["draws"] += 1
        if excl <= t < incl:
            continue
        assert excl - eps * K <= t <= incl + eps * K, (tok, t, excl, incl, K)
        stats["margin"] += 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V", [32000, 320, 50000, 65536])
def test_kernel_matches_the_rule(V, dtype):
    """Kept set and 16 draws per row for B in {1, 3, 32}, sigma in {1, 3, 6} and the parameter grid; the band and margin conditions
    are asserted over everything this case ran.  V = 50000 and 65536 (B in {1, 3}) run the kernel's second 16-bit shape: 64 entries per
    thread, weights recomputed at every use."""
    stats = dict(band_max=0, draws=0, margin=0)
    for B in ((1, 3, 32) if V <= 32768 else (1, 3)):
        for sigma in (1.0, 3.0, 6.0):
            x = _logits(B, V, sigma, dtype, extra=B)
            xd = x.cuda()
            for gi, (T, k, p) in enumerate(GRID):
                seed = SEED + 1000 * gi + B
                toks, kept, _ = _launch(xd, T, k, p, seed)
                for b in range(B):
                    _check_row(x[b], T, k, p, (), seed, b, toks[b], kept[b], stats)
    print(f"V={V} {dtype}: band_max={stats['band_max']} draws={stats['draws']} margin_only={stats['margin']}")
    assert stats["margin"] * 1000 <= stats["draws"], stats


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_top_k_kept_set_is_bit_exact(dtype):
    """The kernel's kept mask with top-p off is the top-k set, ties at the threshold included: equal to the reference bit for bit."""
    for V in (32000, 320, 50000, 65536):
        for sigma in (1.0, 6.0):
            x = _logits(3, V, sigma, dtype, extra=7)
            x[1, : min(V, 400)] = x[1, 0]  # a large tie class (around the threshold for some k, above or below it for others)
            x[2, 10:20] = float("-inf")  # -inf in the input: out of the kept set, like a banned id
            xd = x.cuda()
            for T, k in ((0.7, 50), (1.5, 200), (0.2, 1), (5.0, 7), (1.0, V), (1.0, V + 5), (1.0, 0)):
                _, kept, _ = _launch(xd, T, k, None, 3, steps=1)
                for b in range(3):
                    _, ref, _ = sp.warp_row(x[b], T, k, None)
                    assert torch.equal(kept[b], ref), (V, sigma, T, k, b, int(kept[b].sum()), int(ref.sum()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_special_rows(dtype):
    """A banned EOS set, rows already finished, a row of all-equal logits, a row with one huge (finite) maximum, an odd row stride."""
    V, B = 32000, 6
    x = _logits(B, V, 3.0, dtype, extra=11)
    x[2] = 1.25                      # all equal: every token kept, uniform draw
    x[3, 777] = 3.0e4                # one huge maximum: everything else has no mass
    fin = torch.tensor([0, 1, 0, 0, 0, 1], dtype=torch.int32).cuda()
    eos = [int(x[0].float().argmax()), int(x[4].float().argmax()), 5]
    stats = dict(band_max=0, draws=0, margin=0)
    xd = x.cuda()
    for T, k, p in ((1.0, 0, 0.95), (0.7, 50, 0.9), (5.0, 0, None)):
        toks, kept, st = _launch(xd, T, k, p, 42, steps=4, eos=eos, min_new=4, finished=fin, pad=9)
        assert toks[1].tolist() == [9] * 4 and toks[5].tolist() == [9] * 4  # finished rows emit pad_id
        assert not bool(kept[:, eos].any()), "banned ids are never kept"
        for b in (0, 2, 3, 4):
            _check_row(x[b], T, k, p, eos, 42, b, toks[b], kept[b], stats)
            assert not set(toks[b].tolist()) & set(eos)
        assert toks[3].tolist() == [777] * 4
        if p is None and k == 0:
            assert int(kept[2].sum()) == V - len(set(eos))
        assert st["step"].tolist() == [4] * B and st["full"].tolist() == [104] * B and st["sparse"].tolist() == [54] * B
    # the ban ends at min_new_tokens: from step 2 on the (dominant) EOS can be drawn and finishes the row
    x2 = x.clone()
    x2[0, eos[0]] = 3.0e4
    toks, _, st = _launch(x2.cuda(), 1.0, 0, None, 42, steps=4, eos=eos, min_new=2, pad=9)
    assert toks[0, 2] == eos[0] and toks[0, 3] == 9 and eos[0] not in toks[0, :2].tolist() and st["fin"][0] == 1
    # rows that are not 16-byte addressable (odd stride) and a vocabulary that is not a multiple of the vector width
    Vo = 1003
    wide = torch.zeros(3, Vo + 3, dtype=dtype)
    wide[:, :Vo] = _logits(3, Vo, 3.0, dtype, extra=12)
    view = wide.cuda()[:, :Vo]
    toks, kept, _ = _launch(view, 0.7, 50, 0.9, 5)
    for b in range(3):
        _check_row(wide[b, :Vo], 0.7, 50, 0.9, (), 5, b, toks[b], kept[b], stats)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_top_k_1_bookkeeping_equals_decode_advance(dtype):
    """top_k = 1 keeps the argmax class; where the maximum is unique that is dl_decode_advance's token, and then every output --
    next_ids, out_ids, step, finished, both KV lengths -- is bit-equal, including the min_new_tokens ban, three EOS ids, pad_id for finished rows
    and a per-row decision.  (A row whose maximum is TIED draws inside the tie class by the rule, where the argmax takes the lowest index: such rows
    are checked against the reference instead -- the token must be the reference's, and a member of the class.)"""
    from dynamic_llava_amd import hip_ops as ops

    n_unique = 0
    for V in (32000, 320):
        for B in (1, 3, 32):
            for sigma in (1.0, 3.0, 6.0):
                x = _logits(B, V, sigma, dtype, extra=B + 100)
                xd = x.cuda()
                top = x.float().argmax(dim=1)
                eos = [int(top[0]), int(top[B // 2]), 3]
                fin0 = torch.zeros(B, dtype=torch.int32)
                fin0[B - 1] = 1 if B > 1 else 0
                dec = (torch.arange(B) % 2).to(torch.int32).cuda()
                for min_new in (0, 2):
                    toks, _, st = _launch(xd, 0.7, 1, None, 5, steps=4, eos=eos, min_new=min_new, finished=fin0.cuda(), pad=2, want_mask=False, decision=dec)
                    a = dict(next=torch.zeros(B, dtype=torch.int64).cuda(), out=torch.full((B, 4), -7, dtype=torch.int64).cuda(), step=torch.zeros(B, dtype=torch.int32).cuda(),
                             fin=fin0.cuda(), full=torch.full((B,), 100, dtype=torch.int32).cuda(), sparse=torch.full((B,), 50, dtype=torch.int32).cuda())
                    for _ in range(4):
                        ops.decode_advance(xd, a["next"], a["out"], a["step"], a["fin"], eos, 2, a["full"], a["sparse"], dec, min_new_tokens=min_new)
                    xf = x.float().clone()
                    unique = torch.ones(B, dtype=torch.bool)
                    for banned in ((eos if min_new else []), []):  # the maximum with and without the ban
                        y = xf.clone()
                        if banned:
                            y[:, banned] = float("-inf")
                        unique &= (y == y.max(dim=1, keepdim=True).values).sum(dim=1) == 1
                    n_unique += int(unique.sum())
                    for key in ("step", "full", "sparse"):
                        assert torch.equal(st[key], a[key].cpu()), key
                    assert torch.equal(st["out"][unique], a["out"].cpu()[unique]) and torch.equal(st["next"][unique], a["next"].cpu()[unique])
                    assert torch.equal(st["fin"][unique], a["fin"].cpu()[unique])
                    for b in torch.where(~unique)[0].tolist():
                        if fin0[b]:
                            assert st["out"][b].tolist() == [2] * 4
                            continue
                        done = False
                        for i in range(4):
                            if done:
                                assert int(st["out"][b, i]) == 2
                                continue
                            banned = eos if i < min_new else ()
                            tok, kept, _ = sp.reference_step(x[b], 0.7, 1, None, banned, 5, b, i)
                            assert int(st["out"][b, i]) == tok and bool(kept[tok])
                            done = tok in eos
    assert n_unique > 100


def test_determinism_and_stream_separation():
    """The same call 20 times: identical tokens.  Changing only the seed, only the first step or only the row base changes the stream: at T = 5 over
    > 20000 kept tokens of near-uniform weight two independent streams agree in a position with probability < 1e-4, so 16 steps x 32 rows differ
    in (far) more than half the positions."""
    x = _logits(32, 32000, 1.0, torch.bfloat16, extra=21).cuda()
    base, kept, _ = _launch(x, 5.0, 0, 0.95, 77)
    assert int(kept.sum(dim=1).min()) > 20000
    for _ in range(19):
        again, _, _ = _launch(x, 5.0, 0, 0.95, 77, want_mask=False)
        assert torch.equal(again, base)
    for kw in (dict(seed=78), dict(seed=77 + (1 << 32)), dict(row_base=1), dict(step0=1)):
        args = dict(seed=77, row_base=0, step0=0)
        args.update(kw)
        other, _, _ = _launch(x, 5.0, 0, 0.95, args["seed"], row_base=args["row_base"], step0=args["step0"], want_mask=False)
        assert int((other != base).sum()) > 16 * 32 // 2, kw
    # row_base shifts the rows' streams: row b with base 1 is row b + 1 with base 0 (same logits in both rows)
    same = _logits(1, 32000, 1.0, torch.bfloat16, extra=22).expand(4, -1).contiguous().cuda()
    t0, _, _ = _launch(same, 5.0, 0, 0.95, 9, want_mask=False)
    t1, _, _ = _launch(same, 5.0, 0, 0.95, 9, row_base=1, want_mask=False)
    assert torch.equal(t1[:3], t0[1:]) and not torch.equal(t1, t0)
    # and step0 = 1 is the same stream one step later
    s1, _, _ = _launch(same, 5.0, 0, 0.95, 9, step0=1, want_mask=False)
    assert torch.equal(s1[:, :-1], t0[:, 1:])


def test_uniformity_through_the_kernel():
    """One row with 8 kept tokens of known mass, 20000 steps in one launch sequence: every token's count within 5 standard deviations of
    20000 * p (binomial).  The reference's own draws from the same counters are held to the same bound first."""
    V, N = 320, 20000
    probs = torch.tensor([0.30, 0.20, 0.15, 0.12, 0.10, 0.06, 0.04, 0.03])
    ids = [5, 17, 40, 41, 99, 200, 201, 319]
    x = torch.full((1, V), -50.0)
    x[0, ids] = probs.log()
    toks, kept, _ = _launch(x.cuda(), 1.0, 8, None, 2026, steps=N)
    assert torch.where(kept[0])[0].tolist() == ids
    _, _, det = sp.reference_step(x[0], 1.0, 8, None, (), 2026, 0, 0)
    prefix, K = det["prefix"], det["K"]
    p_ref = (det["m"][ids].double() / K)
    ts = torch.tensor([(sp.draw_r64(2026, 0, i) * K) >> 64 for i in range(N)], dtype=torch.int64)
    ref_toks = torch.searchsorted(prefix, ts, right=True)
    for name, got in (("reference", ref_toks), ("kernel", toks[0])):
        for i, v in enumerate(ids):
            n, pv = int((got == v).sum()), float(p_ref[i])
            assert abs(n - N * pv) <= 5 * math.sqrt(N * pv * (1 - pv)), (name, v, n, N * pv)
        assert int(sum(int((got == v).sum()) for v in ids)) == N
    # the two exps may differ in the last bit: a draw changes hands only when t falls within ~1e-7 * K of a boundary (expected 0.02 of 20000 draws)
    assert int((toks[0] != ref_toks).sum()) <= 2


# ---------------------------------------------------------------------------------------------------------------------------------------
# model level: the tiny config and builders of oracle/fixtures.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def _model(dtype, seed=None):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from oracle import fixtures as fx
    from oracle.make_golden import SD_SEED

    cfg = fx.tiny_config()  # text predictor on: rows evict
    sd = fx.make_state_dict(cfg, seed=SD_SEED if seed is None else seed, predictor_gain=50.0)
    clip = fx.build_clip(cfg, seed=1, dtype=dtype)
    model = build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg), sd, clip.state_dict(), dtype=dtype, device="cuda")
    return cfg, model


def _inputs(cfg, B, dtype):
    from oracle import fixtures as fx

    if B == 1:
        return dict(inputs=fx.make_prompt(cfg, 5, 9, seed=2)[None].cuda(), images=fx.make_images(cfg, 1, seed=3).to(dtype).cuda())
    prompts = [fx.make_prompt(cfg, 5, 7, seed=0), fx.make_prompt(cfg, 2, 15, seed=1)]  # ragged
    n = max(p.shape[0] for p in prompts)
    ids, am = torch.zeros(B, n, dtype=torch.long), torch.zeros(B, n, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, : p.shape[0]] = p
        am[b, : p.shape[0]] = 1
    return dict(inputs=ids.cuda(), attention_mask=am.cuda(), images=fx.make_images(cfg, B, seed=3).to(dtype).cuda())


def _lens(model):
    c = model.last_cache
    return c.lens.cpu().tolist(), list(c.full_len_host)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_degenerate_settings_equal_greedy(dtype, B):
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=10, eos_token_id=None)
    greedy = model.generate(**kw)
    lens_g = _lens(model)
    a = model.generate(**kw, do_sample=True, seed=5, temperature=0.7, top_k=1)
    assert torch.equal(a, greedy) and _lens(model) == lens_g
    b = model.generate(**kw, do_sample=True, seed=6, temperature=1.3, top_p=1e-6)
    assert torch.equal(b, greedy) and _lens(model) == lens_g
    assert torch.equal(model.generate(**kw), greedy), "a greedy call after sampled ones is what it was before them"


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_same_seed_same_tokens_whatever_the_schedule(dtype, B):
    cfg, model = _model(dtype)
    kw = dict(_inputs(cfg, B, dtype), max_new_tokens=24, eos_token_id=None, do_sample=True, temperature=5.0, top_p=0.95, seed=11)
    greedy = model.generate(**{k: v for k, v in kw.items() if k not in ("do_sample", "temperature", "top_p", "seed")})
    base = model.generate(**kw)
    lens = _lens(model)
    assert base.shape == (B, 24) and not torch.equal(base, greedy)
    assert torch.equal(model.generate(**kw), base) and _lens(model) == lens
    assert not torch.equal(model.generate(**dict(kw, seed=12)), base)
    for se in (1, 4, 64):
        assert torch.equal(model.generate(**kw, sync_every=se), base) and _lens(model) == lens, se
    model.use_hip_graph = False
    assert torch.equal(model.generate(**kw), base) and _lens(model) == lens
    model.use_hip_graph = True
    if B == 2:  # sample_row_base: row b of a shard that starts at global row 1 draws what global row b + 1 draws -- different from base 0
        assert not torch.equal(model.generate(**kw, sample_row_base=1), base)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_replay_every_draw_from_the_scores(dtype, B):
    """output_scores (+ output_logits: the raw step logits): the reference accepts every emitted token under the two-sided rule, and scores[i] is
    -inf exactly outside the kept set."""
    cfg, model = _model(dtype)
    T, k, p, seed, base_row = 1.5, 200, 0.8, 31, 3
    res = model.generate(**_inputs(cfg, B, dtype), max_new_tokens=12, eos_token_id=None, do_sample=True, temperature=T, top_k=k, top_p=p, seed=seed, sample_row_base=base_row,
                         return_dict_in_generate=True, output_scores=True, output_logits=True)
    seq = res["sequences"].cpu()
    assert len(res["scores"]) == len(res["logits"]) == seq.shape[1] == 12
    stats = dict(band_max=0, draws=0, margin=0)
    for i in range(seq.shape[1]):
        raw = res["logits"][i].cpu().to(dtype)  # the step buffer holds the model dtype; the fp32 copy is exact
        sc = res["scores"][i].cpu()
        for b in range(B):
            kept_scores = sc[b] > float("-inf")
            _check_row(raw[b], T, k, p, (), seed, b, seq[b, i : i + 1], kept_scores, stats, row_base=base_row, step0=i)
            z, kept_ref, _ = sp.warp_row(raw[b], T, k, p)
            # (`scores` are computed on the host with the contract's own functions, so this pins only their FORM -- z inside the kept set, -inf outside; what
            # checks the device in this test is the draw check above, against that host-side kept set)
            assert torch.equal(kept_scores, kept_ref) and torch.equal(sc[b][kept_ref], z[kept_ref])
    assert stats["margin"] == 0 or stats["draws"] >= 1000 * stats["margin"]
    # the same request without the step-by-step outputs draws the same tokens
    plain = model.generate(**_inputs(cfg, B, dtype), max_new_tokens=12, eos_token_id=None, do_sample=True, temperature=T, top_k=k, top_p=p, seed=seed, sample_row_base=base_row)
    assert torch.equal(plain.cpu(), seq)


def test_one_graph_serves_every_setting():
    cfg, model = _model(torch.bfloat16)
    kw = dict(_inputs(cfg, 1, torch.bfloat16), max_new_tokens=12, eos_token_id=None)
    for _ in range(3):  # first sighting runs eagerly, the second captures, the third replays
        model.generate(**kw, do_sample=True, seed=1, temperature=0.7)
    st = model._dstate
    n_dec, n_pre = len(st.graphs), len(model._prefill_graphs)
    assert n_dec >= 1 and n_pre >= 1
    outs = []
    for T, k, p, seed in ((0.2, 0, None, 2), (0.7, 50, 0.9, 3), (5.0, 0, 0.95, 4), (1.5, 200, 0.8, 5)):
        outs.append(model.generate(**kw, do_sample=True, seed=seed, temperature=T, top_k=k, top_p=p))
        assert len(st.graphs) == n_dec and len(model._prefill_graphs) == n_pre and model._dstate is st, (T, k, p)
    assert len({tuple(o.cpu().tolist()[0]) for o in outs}) > 1
    # the first greedy call afterwards adds at most the greedy entries it would add anyway: one prefill entry, and one decode graph per split factor
    # the sampled calls walked through (same request shape, same schedule)
    model.generate(**kw)
    assert len(model._prefill_graphs) <= n_pre + 1 and len(st.graphs) <= 2 * n_dec
    assert {key[-1].sampled for key in st.graphs} == {True, False}, "sampled / greedy is in the decode key's last element, the request's step mode"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generate_eos_stops_and_pads_and_min_new_tokens_delays(dtype):
    cfg, model = _model(dtype)
    inp = _inputs(cfg, 2, dtype)
    T = 1.0
    res = model.generate(**inp, max_new_tokens=1, eos_token_id=None, return_dict_in_generate=True, output_logits=True)
    first = res["logits"][0].cpu().to(dtype)
    eos = torch.topk(first[0].float(), 3).indices.tolist()  # EOS set = row 0's three most probable ids
    seed = next(s for s in range(200) if sp.reference_step(first[0], T, 0, None, (), s, 0, 0)[0] in eos and sp.reference_step(first[1], T, 0, None, (), s, 1, 0)[0] not in eos)
    kw = dict(inp, max_new_tokens=40, eos_token_id=eos, pad_token_id=7, do_sample=True, temperature=T, seed=seed)
    out = model.generate(**kw).cpu()
    executed = int(model._dstate.step.max())  # tokens the device loop produced in that call (the prefill's included), before any trimming
    assert int(out[0, 0]) in eos and (out.shape[1] == 1 or out[0, 1:].tolist() == [7] * (out.shape[1] - 1))
    free = model.generate(**dict(kw, eos_token_id=None)).cpu()
    # HF stops when every row has emitted EOS: the call ends with row 1's first EOS (trimmed there), or at max_new_tokens
    n = out.shape[1]
    assert n <= 40 and not set(out[1, : n - 1].tolist()) & set(eos) and (n == 40 or int(out[1, n - 1]) in eos)
    # ... and the device loop itself stopped where the greedy path's chunk rule stops: chunks of 4, 4, then sync_every (8) steps after the prefill's token; the
    # flags of the first two chunks are read as soon as the chunk is enqueued, later ones one chunk late.  (The trimming above would hide surplus steps;
    # the device's own step counter does not.)
    chunk_end = min(e for e in (5, 9, 17, 25, 33, 40) if e >= n)
    allowed = min(40, chunk_end if chunk_end <= 9 else chunk_end + 8)
    assert n <= executed <= allowed, (n, executed, allowed)
    assert free.shape[1] == 40 and int(free[0, 0]) == int(out[0, 0])  # without an EOS set nothing stops; the first draw is the same draw
    assert int(model._dstate.step.max()) == 40
    late = model.generate(**kw, min_new_tokens=3).cpu()
    assert not set(late[0, :3].tolist()) & set(eos) and late.shape[1] >= 3
    res2 = model.generate(**dict(kw, max_new_tokens=1), min_new_tokens=1, return_dict_in_generate=True, output_scores=True)
    assert bool((res2["scores"][0][:, eos] == float("-inf")).all())


def test_untouched_routes():
    """generator= (today's loop, torch's RNG) gives what it gave, before and after a device-sampled call; so does a greedy call."""
    cfg, model = _model(torch.float32)
    kw = dict(_inputs(cfg, 2, torch.float32), max_new_tokens=8, eos_token_id=None)
    greedy = model.generate(**kw)
    loop = lambda: model.generate(**kw, do_sample=True, temperature=5.0, top_p=0.95, generator=torch.Generator(device="cuda").manual_seed(7))
    c1 = loop()
    dev = model.generate(**kw, do_sample=True, temperature=5.0, top_p=0.95, seed=7)
    assert torch.equal(loop(), c1) and torch.equal(model.generate(**kw), greedy)
    assert dev.shape == c1.shape and not torch.equal(dev, greedy)
    # a generator wins over a seed, and four EOS ids keep the plain loop
    assert torch.equal(model.generate(**kw, do_sample=True, temperature=5.0, top_p=0.95, seed=7, generator=torch.Generator(device="cuda").manual_seed(7)), c1)
    with pytest.raises(ValueError):
        model.generate(**kw, do_sample=True, seed=1, top_p=0.0)
    # more than three EOS ids, named in the call or coming from the model config, keep the loop they had -- and that loop still SAMPLES (torch's RNG)
    four = [cfg.vocab_size - 1 - i for i in range(4)]
    kw4 = {k: v for k, v in kw.items() if k != "eos_token_id"}
    hot = dict(do_sample=True, temperature=5.0, top_p=0.95, seed=7)
    torch.manual_seed(123)
    by_kwarg = model.generate(**kw4, eos_token_id=four, **hot)
    saved = model.config.eos_token_id
    model.config.eos_token_id = four
    try:
        torch.manual_seed(123)
        by_config = model.generate(**kw4, **hot)
        greedy4 = model.generate(**kw4)
    finally:
        model.config.eos_token_id = saved
    assert torch.equal(by_config, by_kwarg), "the config's EOS list routes like the same list named in the call"
    n4 = min(by_config.shape[1], greedy4.shape[1])
    assert not torch.equal(by_config[:, :n4], greedy4[:, :n4]), "a sampling request must not come back greedy"
