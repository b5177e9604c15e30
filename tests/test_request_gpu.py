"""GPU: the two host routes of generate() -- both run request.host_loop over forward() -- against the routes that do not, on the tiny config of
oracle/fixtures.py: equal tokens and equal KV lengths."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from oracle import fixtures as fx
    from oracle.make_golden import SD_SEED

    cfg = fx.tiny_config()  # text predictor on: rows evict
    sd = fx.make_state_dict(cfg, seed=SD_SEED, predictor_gain=50.0)
    clip = fx.build_clip(cfg, seed=1, dtype=torch.bfloat16)
    model = build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg), sd, clip.state_dict(), dtype=torch.bfloat16, device="cuda")
    req = dict(inputs=fx.make_prompt(cfg, 3, 4, seed=2)[None].cuda(), images=fx.make_images(cfg, 1, seed=3).to(torch.bfloat16).cuda())
    yield cfg, model, req
    del model  # (a model that served requests is an object cycle: collected here, not inside somebody's stream capture)
    gc.collect()
    torch.cuda.synchronize()


def _kv_lens(cache):
    return [[int(n) for n in layer] for layer in cache[1]]


def test_four_eos_ids_take_the_host_loop_and_match_the_device_loop(tiny):
    cfg, model, req = tiny
    plain = model.generate(**req, max_new_tokens=12, eos_token_id=None)
    plain_lens = _kv_lens(model.last_cache)
    assert plain.shape == (1, 12)
    never = [t for t in range(3, cfg.vocab_size) if t not in plain[0].tolist()][:4]  # more ids than the device compares; none of them occurs
    calls = []
    host, model._generate_sample = model._generate_sample, lambda *a, **k: calls.append(k.get("greedy")) or host(*a, **k)
    try:
        got = model.generate(**req, max_new_tokens=12, eos_token_id=never)
    finally:
        del model._generate_sample
    assert calls == [True]
    assert got.tolist() == plain.tolist() and _kv_lens(model.last_cache) == plain_lens


def test_continuation_on_a_cache_matches_forward_driven_by_argmax(tiny):
    cfg, model, req = tiny
    turn2 = torch.randint(3, cfg.vocab_size, (1, 5), generator=torch.Generator().manual_seed(12)).cuda()
    first = [model.generate(**req, max_new_tokens=4, eos_token_id=None, return_dict_in_generate=True) for _ in range(2)]  # two caches of one dialogue
    assert first[0]["sequences"].tolist() == first[1]["sequences"].tolist() and _kv_lens(first[0]["past_key_values"]) == _kv_lens(first[1]["past_key_values"])
    got = model.generate(turn2, past_key_values=first[0]["past_key_values"], max_new_tokens=6, eos_token_id=None)
    got_lens = _kv_lens(model.last_cache)
    cache, ref = first[1]["past_key_values"], []
    out = model(turn2, past_key_values=cache)
    for step in range(6):
        nxt = out.logits[:, -1].argmax(dim=-1)
        ref.append(int(nxt[0]))
        if step < 5:
            out = model(nxt[:, None], past_key_values=out.past_key_values)
    assert got.tolist() == [ref] and got_lens == _kv_lens(out.past_key_values)
