"""GPU, model level: the batch-1 decode step with every layer's q|k|v streamed as 12-bit packed bf16 inside the fused q|k|v + attention launch
(decode_weight_pack_qkv: dl_gemv_qkv_attn_pk; layer sparse_layer's gate|up inside dl_gemv_gu_tp_pk) against the same model with the knob off -- every
number must be bit-equal: generated ids, prefill logits, KV lengths, the per-step logits of a forward() loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fixtures as fx  # noqa: E402

from dynamic_llava_amd import hip_ops as ops  # noqa: E402


@pytest.fixture(scope="module")
def slice7b():
    """LLaVA-1.5-7B layer width (H = 4096, I = 11008), 3 layers, sparse_layer = 2, a 2048-word vocabulary, built with the defaults."""
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig

    cfg = fx.llava7b_config(num_hidden_layers=3)
    cfg.vocab_size = 2048
    sd = fx.make_state_dict(cfg, seed=7, predictor_gain=50.0)
    model = build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg), sd, None, dtype=torch.bfloat16, device="cuda")
    g = torch.Generator().manual_seed(21)
    feats = torch.randn(1, 576, 4096, generator=g).to(torch.bfloat16).cuda()
    ids = fx.make_prompt(cfg, 35, 20, seed=4)[None].cuda()
    return cfg, model, feats, ids


def _set_qkv(model, on):
    model.decode_weight_pack_qkv = on
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


def _spied(model, ids, feats, names):
    calls = {n: [] for n in names}
    orig = {n: getattr(ops, n) for n in names}

    def make(n):
        def spy(p, *a, **k):
            calls[n].append(getattr(p, "N", None) or p.shape[0])
            return orig[n](p, *a, **k)

        return spy

    for n in names:
        setattr(ops, n, make(n))
    try:
        model._dstate = None  # a fresh capture: the spies see the step's launches once
        _generate(model, ids, feats, 3)
    finally:
        for n in names:
            setattr(ops, n, orig[n])
    return calls


def test_the_packed_fused_launches_are_the_default_route(slice7b):
    cfg, model, feats, ids = slice7b
    L = cfg.num_hidden_layers
    assert model.decode_weight_pack_qkv and model.knobs()["decode_weight_pack_qkv"] is True
    assert all(l.pk_qkv is not None and (l.pk_qkv.N, l.pk_qkv.K) == (3 * 4096, 4096) for l in model.model.layers)
    assert all(set(l.pk) == {"o", "gu", "down"} for l in model.model.layers)  # the copy is kept beside layer.pk, not in it
    names = ("gemv_qkv_attn_pk", "gemv_gu_tp_pk", "gemv_qkv_attn", "gemv_gu_tp")
    calls = _spied(model, ids, feats, names)
    try:
        _set_qkv(model, False)
        off = _spied(model, ids, feats, names)
    finally:
        _set_qkv(model, True)
    # every capture of the step (generate() captures one graph per chunk length) holds the predictor's launch once and the packed launch once per fused
    # layer -- the layers the knob-off step runs on dl_gemv_qkv_attn
    captures = len(calls["gemv_gu_tp_pk"])
    assert captures >= 1 and calls["gemv_gu_tp_pk"] == [2 * 11008] * captures and calls["gemv_gu_tp"] == [], calls
    n_fused, rest = divmod(len(calls["gemv_qkv_attn_pk"]), captures)
    assert rest == 0 and 1 <= n_fused <= L, calls
    assert calls["gemv_qkv_attn_pk"] == [3 * 4096] * (n_fused * captures) and calls["gemv_qkv_attn"] == [], calls
    assert off["gemv_qkv_attn_pk"] == [] and len(off["gemv_qkv_attn"]) == n_fused * captures, off
    assert off["gemv_gu_tp_pk"] == [2 * 11008] * captures, off  # (gate|up's copy belongs to decode_weight_pack, not to this knob)


def test_knob_off_makes_no_copy_and_leaves_the_other_keys_alone(slice7b):
    cfg, model, feats, ids = slice7b
    on = model.weight_pack_bytes()
    try:
        _set_qkv(model, False)
        assert all(getattr(l, "pk_qkv", None) is None for l in model.model.layers)
        off = model.weight_pack_bytes()
    finally:
        _set_qkv(model, True)
    assert {k: on[k] for k in ("matrices", "packed", "bf16")} == {k: off[k] for k in ("matrices", "packed", "bf16")}
    assert on["matrices"] == cfg.num_hidden_layers + 1  # gate|up of every layer and the vocabulary projection, as before
    assert on["qkv"]["matrices"] == cfg.num_hidden_layers and 0 < on["qkv"]["packed"] < 0.9 * on["qkv"]["bf16"] and off["qkv"] == {"matrices": 0, "packed": 0, "bf16": 0}


def test_generate_and_forward_loop_are_bit_equal_with_the_knob_off(slice7b):
    cfg, model, feats, ids = slice7b
    forced = fx.make_forced_tokens(cfg, 5, 1, seed=6)
    try:
        ids_on, pre_on, lens_on = _generate(model, ids, feats, 12)
        loop_on = _forward_loop(model, ids, feats, forced)
        _set_qkv(model, False)
        ids_off, pre_off, lens_off = _generate(model, ids, feats, 12)
        loop_off = _forward_loop(model, ids, feats, forced)
    finally:
        _set_qkv(model, True)
    assert torch.equal(ids_on, ids_off)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)
    assert ids_on.shape[1] == 12 and torch.equal(bits(pre_on), bits(pre_off))
    assert torch.equal(lens_on[0], lens_off[0]) and torch.equal(lens_on[1], lens_off[1])
    assert loop_on.dtype == torch.float32 and torch.equal(loop_on.view(torch.int32), loop_off.view(torch.int32))
    assert torch.isfinite(loop_on).all()


def test_rewritten_q_proj_is_repacked(slice7b):
    """The packed copy is detached from the parameters: an in-place edit of one layer's q_proj.weight must reach the packed step (the fingerprint check of
    generate() re-finalizes and replaces the copy object), exactly as it reaches the model-dtype step."""
    cfg, model, feats, ids = slice7b
    layer = model.model.layers[1]
    w = layer.self_attn.q_proj.weight
    saved = w.data.clone()
    try:
        before, _, _ = _generate(model, ids, feats, 4)
        old_pk = layer.pk_qkv
        with torch.no_grad():
            w.mul_(-3.0)
        after, _, _ = _generate(model, ids, feats, 4)
        assert layer.pk_qkv is not None and layer.pk_qkv is not old_pk
        _set_qkv(model, False)
        after_off, _, _ = _generate(model, ids, feats, 4)
        assert torch.equal(after, after_off)
    finally:
        with torch.no_grad():
            w.copy_(saved)
        _set_qkv(model, True)
    restored, _, _ = _generate(model, ids, feats, 4)
    assert torch.equal(restored, before)
