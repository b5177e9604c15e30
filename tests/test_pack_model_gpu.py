"""GPU, model level: the batch-1 decode step on 12-bit packed weights (decode_weight_pack, dl_gemv_pk) against the same model with the pack off -- every
number must be bit-equal: generated ids, prefill logits, KV lengths, the per-step logits of a forward() loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fixtures as fx  # noqa: E402

from dynamic_llava_amd import hip_ops as ops  # noqa: E402


def _build(cfg_ns, sd, clip, dtype):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig

    return build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg_ns), sd, clip.state_dict() if clip is not None else None, dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def slice7b():
    """LLaVA-1.5-7B layer width (H = 4096, I = 11008), 3 layers, sparse_layer = 2, a 2048-word vocabulary: the configuration of
    test_model_gpu.test_full_width_slice_vs_oracle.  Every packed launch shape of the flagship step occurs."""
    cfg = fx.llava7b_config(num_hidden_layers=3)
    cfg.vocab_size = 2048
    sd = fx.make_state_dict(cfg, seed=7, predictor_gain=50.0)
    model = _build(cfg, sd, None, torch.bfloat16)
    assert model.decode_weight_pack and not model.decode_weight_pack_plain  # the defaults: gate|up and the vocabulary projection only
    assert all(l.pk["gu"] is not None and l.pk["o"] is None and l.pk["down"] is None for l in model.model.layers) and model._pk_lm_head is not None
    model.decode_weight_pack_plain = True  # the tests below run every packed launch: o_proj and down_proj too
    model._packed = False
    model.finalize()
    g = torch.Generator().manual_seed(21)
    feats = torch.randn(1, 576, 4096, generator=g).to(torch.bfloat16).cuda()
    ids = fx.make_prompt(cfg, 35, 20, seed=4)[None].cuda()
    return cfg, model, feats, ids


def _set_pack(model, on):
    model.decode_weight_pack = on
    model._packed = False
    model.finalize()  # makes / drops the packed copies


def _generate(model, ids, feats, n):
    out = model.generate(ids, image_features=feats, max_new_tokens=n, do_sample=False, eos_token_id=None)
    torch.cuda.synchronize()
    model.check_device_errors()
    lens = (torch.as_tensor(model.last_cache[1][0]).clone(), torch.as_tensor(model.last_cache[1][-1]).clone())  # final KV lengths of the first / last layer
    return out.clone(), model.last_prefill_logits.clone(), lens


def _forward_loop(model, ids, feats, forced):
    out = model(ids, image_features=feats)
    logits = [out.logits[:, -1].clone()]
    pkv = out.past_key_values
    for j in range(forced.shape[0]):
        out = model(forced[j][:, None].cuda(), past_key_values=pkv)
        pkv = out.past_key_values
        logits.append(out.logits[:, -1].clone())
    torch.cuda.synchronize()
    model.check_device_errors()
    return torch.stack(logits)


def test_packed_copies_are_made_and_used(slice7b):
    cfg, model, feats, ids = slice7b
    assert model.knobs()["decode_weight_pack"] is True
    for l in model.model.layers:
        assert all(l.pk[k] is not None for k in ("o", "gu", "down")), {k: v is not None for k, v in l.pk.items()}
    assert model._pk_lm_head is not None
    b = model.weight_pack_bytes()
    print(f"packed copies: {b['matrices']} matrices, {b['packed'] / b['bf16']:.4f} of their bf16 bytes")
    assert b["matrices"] == 3 * 3 + 1 and b["packed"] < 0.9 * b["bf16"]  # (pack() keeps no copy at or above 0.9)
    calls = []
    orig = ops.gemv_pk

    def spy(p, *a, **k):
        calls.append((p.N, p.K, k.get("mode", 0)))
        return orig(p, *a, **k)

    ops.gemv_pk = spy
    try:
        model._dstate = None  # a fresh capture: the spy sees the step's launches once
        _generate(model, ids, feats, 3)
    finally:
        ops.gemv_pk = orig
    kinds = set(calls)
    A, PAIR = ops.GEMV_ADDNORM, ops.GEMV_OUT_SILU_PAIR
    assert {(4096, 4096, 0), (22016, 4096, A | PAIR), (4096, 11008, 0), (2048, 4096, A)} <= kinds, kinds


def test_generate_and_forward_loop_are_bit_equal_with_the_pack_off(slice7b):
    cfg, model, feats, ids = slice7b
    forced = fx.make_forced_tokens(cfg, 5, 1, seed=6)
    try:
        ids_on, pre_on, lens_on = _generate(model, ids, feats, 12)
        loop_on = _forward_loop(model, ids, feats, forced)
        _set_pack(model, False)
        assert all(l.pk is None for l in model.model.layers) and model._pk_lm_head is None
        ids_off, pre_off, lens_off = _generate(model, ids, feats, 12)
        loop_off = _forward_loop(model, ids, feats, forced)
    finally:
        _set_pack(model, True)
    assert torch.equal(ids_on, ids_off)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)
    assert ids_on.shape[1] == 12 and torch.equal(bits(pre_on), bits(pre_off))
    assert torch.equal(lens_on[0], lens_off[0]) and torch.equal(lens_on[1], lens_off[1])
    assert loop_on.dtype == torch.float32 and torch.equal(loop_on.view(torch.int32), loop_off.view(torch.int32))
    assert torch.isfinite(loop_on).all()


def test_rewritten_weights_are_repacked(slice7b):
    """The packed copies are detached from the parameters: an in-place edit of a decoder weight or of the lm_head must reach the packed step (the fingerprint
    check of generate() re-finalizes), exactly as it reaches the model-dtype step."""
    cfg, model, feats, ids = slice7b
    w = model.lm_head.weight
    saved = w.data.clone()
    try:
        before, _, _ = _generate(model, ids, feats, 4)
        old_pk = model._pk_lm_head
        with torch.no_grad():
            w.mul_(-1.0)  # every logit changes sign: greedy picks other tokens
        after, _, _ = _generate(model, ids, feats, 4)
        assert model._pk_lm_head is not old_pk
        _set_pack(model, False)
        after_off, _, _ = _generate(model, ids, feats, 4)
        assert torch.equal(after, after_off) and not torch.equal(after, before)
    finally:
        with torch.no_grad():
            w.copy_(saved)
        _set_pack(model, True)
