"""GPU, model level: the batch-1 decode step with every layer's long-row down_proj streamed as 12-bit packed bf16 (decode_weight_pack_down: dl_gemv_pk's
long-row kernel, the copy kept as layer.pk_down beside layer.pk) against the same model with the knob off -- every number must be bit-equal: generated
ids, prefill logits, KV lengths, the per-step logits of a forward() loop."""
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


def _set_down(model, on):
    model.decode_weight_pack_down = on
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


def _spied(model, ids, feats):
    """-> ((N, K, mode) of every ops.gemv_pk call, data_ptr of every weight ops.gemv received) of a fresh capture of the step."""
    pk_calls, gemv_ptrs = [], []
    orig_pk, orig_gemv = ops.gemv_pk, ops.gemv

    def spy_pk(p, *a, **k):
        pk_calls.append((p.N, p.K, k.get("mode", 0)))
        return orig_pk(p, *a, **k)

    def spy_gemv(w, *a, **k):
        gemv_ptrs.append(w.data_ptr())
        return orig_gemv(w, *a, **k)

    ops.gemv_pk, ops.gemv = spy_pk, spy_gemv
    try:
        model._dstate = None  # a fresh capture: the spies see the step's launches once
        _generate(model, ids, feats, 3)
    finally:
        ops.gemv_pk, ops.gemv = orig_pk, orig_gemv
    return pk_calls, gemv_ptrs


def test_the_packed_down_proj_is_the_default_route(slice7b):
    cfg, model, feats, ids = slice7b
    L = cfg.num_hidden_layers
    assert model.decode_weight_pack_down and model.knobs()["decode_weight_pack_down"] is True and not model.decode_weight_pack_plain
    for l in model.model.layers:
        assert l.pk_down is not None and (l.pk_down.N, l.pk_down.K) == (4096, 11008)
        assert set(l.pk) == {"o", "gu", "down"} and l.pk["down"] is None  # the copy is kept beside layer.pk, not in it
    b = model.weight_pack_bytes()
    assert b["down"]["matrices"] == L and 0 < b["down"]["packed"] < 0.9 * b["down"]["bf16"] and b["matrices"] == L + 1
    down_ptrs = {l.mlp.down_proj.weight.data_ptr() for l in model.model.layers}
    o_ptrs = {l.self_attn.o_proj.weight.data_ptr() for l in model.model.layers}
    pk_calls, gemv_ptrs = _spied(model, ids, feats)
    assert (4096, 11008, 0) in set(pk_calls), set(pk_calls)
    assert pk_calls.count((4096, 11008, 0)) % L == 0  # every layer of every capture
    assert not (set(gemv_ptrs) & down_ptrs)  # no down_proj weight reaches dl_gemv ...
    assert set(gemv_ptrs) & o_ptrs  # ... while o_proj's still does (the spy does see the step's bf16 launches)


def test_knob_off_makes_no_copy_and_leaves_the_other_keys_alone(slice7b):
    cfg, model, feats, ids = slice7b
    on = model.weight_pack_bytes()
    try:
        _set_down(model, False)
        assert all(getattr(l, "pk_down", None) is None for l in model.model.layers)
        assert model.knobs()["decode_weight_pack_down"] is False
        off = model.weight_pack_bytes()
        pk_calls, gemv_ptrs = _spied(model, ids, feats)
    finally:
        _set_down(model, True)
    assert {k: on[k] for k in ("matrices", "packed", "bf16", "qkv")} == {k: off[k] for k in ("matrices", "packed", "bf16", "qkv")}
    assert off["down"] == {"matrices": 0, "packed": 0, "bf16": 0}
    assert (4096, 11008, 0) not in set(pk_calls)
    assert {l.mlp.down_proj.weight.data_ptr() for l in model.model.layers} <= set(gemv_ptrs)


def test_plain_pack_is_not_packed_twice(slice7b):
    cfg, model, feats, ids = slice7b
    try:
        model.decode_weight_pack_plain = True
        _set_down(model, True)
        assert all(l.pk["down"] is not None and l.pk_down is l.pk["down"] for l in model.model.layers)
        b = model.weight_pack_bytes()
        assert b["matrices"] == 3 * cfg.num_hidden_layers + 1 and b["down"]["matrices"] == 0  # counted once, where it was counted before
    finally:
        model.decode_weight_pack_plain = False
        _set_down(model, True)
    assert all(l.pk["down"] is None and l.pk_down is not None for l in model.model.layers)


def test_generate_and_forward_loop_are_bit_equal_with_the_knob_off(slice7b):
    cfg, model, feats, ids = slice7b
    forced = fx.make_forced_tokens(cfg, 5, 1, seed=6)
    try:
        ids_on, pre_on, lens_on = _generate(model, ids, feats, 12)
        loop_on = _forward_loop(model, ids, feats, forced)
        _set_down(model, False)
        ids_off, pre_off, lens_off = _generate(model, ids, feats, 12)
        loop_off = _forward_loop(model, ids, feats, forced)
    finally:
        _set_down(model, True)
    assert torch.equal(ids_on, ids_off)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)
    assert ids_on.shape[1] == 12 and torch.equal(bits(pre_on), bits(pre_off))
    assert torch.equal(lens_on[0], lens_off[0]) and torch.equal(lens_on[1], lens_off[1])
    assert loop_on.dtype == torch.float32 and torch.equal(loop_on.view(torch.int32), loop_off.view(torch.int32))
    assert torch.isfinite(loop_on).all()
