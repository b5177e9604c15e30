"""CPU: the sampling rule (dynamic_llava_amd/sampling.py) against its sources -- Philox known answers, HF's logits warpers as
_generate_sample applies them -- plus the host-side pieces of the device sampler: argument rejection, parameter validation, routing."""
import ctypes

import pytest
import torch

from dynamic_llava_amd import sampling as sp

GRID = [(0.2, 0, None), (0.7, 50, 0.9), (1.0, 0, 0.95), (1.5, 200, 0.8), (5.0, 0, 0.95), (1.0, 0, 0.5)]
V = 32000


def test_philox4x32_10_known_answers():
    """The three known-answer vectors of the Random123 distribution (kat_vectors: philox4x32 10)."""
    assert sp.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    f = 0xFFFFFFFF
    assert sp.philox4x32_10((f, f, f, f), (f, f)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert sp.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    # the draw's packing: r64 = out[1] << 32 | out[0], counter = (step, row_base + row, 0, 0), key = the seed's two halves
    seed = (0x299F31D0 << 32) | 0xA4093822
    o = sp.philox4x32_10((7, 5, 0, 0), (0xA4093822, 0x299F31D0))
    assert sp.draw_r64(seed, 2, 7, row_base=3) == (o[1] << 32) | o[0]


def _hf_kept(x, T, top_k, top_p, banned=()):
    """_generate_sample's warpers (temperature, min-new-tokens ban, top-k, top-p), restated: the set of tokens left finite."""
    z = x.float()[None] / T
    if banned:
        z[:, list(banned)] = float("-inf")
    if top_k > 0:
        kth = torch.topk(z, min(top_k, z.shape[-1]), dim=-1).values[:, -1:]
        z = z.masked_fill(z < kth, float("-inf"))
    if top_p is not None and float(top_p) < 1.0:
        sz, si = torch.sort(z, dim=-1, descending=False)
        cum = sz.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= (1.0 - float(top_p))
        remove[:, -1] = False
        z = z.masked_fill(remove.scatter(1, si, remove), float("-inf"))
    return z[0] > float("-inf")


def _tie_free_fp32(sigma, seed):
    """V fp32 logits whose z = logit / T has no two equal values for any T of the grid."""
    g = torch.Generator().manual_seed(seed)
    x = torch.unique(torch.randn(3 * V, generator=g) * sigma)
    ok = torch.ones_like(x, dtype=torch.bool)
    for T in sorted({t for t, _, _ in GRID}):
        z = x / torch.tensor(T, dtype=torch.float32)  # x is sorted, so is z
        same = z[1:] == z[:-1]
        ok[1:] &= ~same
        ok[:-1] &= ~same
    x = x[ok]
    assert x.numel() >= V
    return x[torch.randperm(x.numel(), generator=g)[:V]]


@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_rule_equals_the_hf_warpers_on_tie_free_fp32_logits(sigma):
    x = _tie_free_fp32(sigma, 20261016)
    for T, k, p in GRID:
        for banned in ((), (int(x.argmax()), 17)):
            _, kept, det = sp.reference_step(x, T, k, p, banned, seed=1, row=0, step=0)
            hf = _hf_kept(x, T, k, p, banned)
            assert torch.equal(kept, hf), (T, k, p, int(kept.sum()), int(hf.sum()))
            assert det["K"] > 0 and bool(kept[int(torch.where(hf)[0][x[hf].argmax()])])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sigma", [1.0, 3.0, 6.0])
def test_rule_is_a_superset_by_whole_tie_classes_on_16_bit_logits(dtype, sigma):
    g = torch.Generator().manual_seed(20261016)
    x = (torch.randn(V, generator=g) * sigma).to(dtype)
    for T, k, p in GRID:
        z, kept, _ = sp.warp_row(x, T, k, p)
        hf = _hf_kept(x, T, k, p)
        assert bool((kept | ~hf).all()), (T, k, p)  # superset
        extra = kept & ~hf
        if bool(extra.any()):
            assert bool(torch.isin(z[extra], z[hf]).all()), (T, k, p)  # every extra token ties with a token HF kept


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_top_k_1_and_a_tiny_top_p_keep_exactly_the_argmax_class(dtype):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(V, generator=g) * 3).to(dtype)
    x[123] = x[4567] = x.max()  # a tied maximum
    cls = x == x.max()
    for T, k, p in ((0.7, 1, None), (1.3, 0, 1e-6), (5.0, 1, 1e-6)):
        tok, kept, det = sp.reference_step(x, T, k, p, (), seed=9, row=1, step=2)
        assert torch.equal(kept, cls) and bool(cls[tok])
        assert det["K"] == int(cls.sum()) << sp.S_BITS


def test_draw_walks_the_kept_masses_in_index_order():
    x = torch.full((64,), -1e4)
    x[[3, 10, 40]] = torch.tensor([0.0, 0.0, 0.0])
    seen = set()
    for step in range(64):
        tok, kept, det = sp.reference_step(x, 1.0, 0, None, (), seed=5, row=0, step=step)
        assert det["K"] == 3 << sp.S_BITS and int(kept.sum()) == 64  # zero-mass tokens stay in the set without top-p, and are never drawn
        third = det["t"] // (1 << sp.S_BITS)
        assert tok == [3, 10, 40][third]
        seen.add(tok)
    assert seen == {3, 10, 40}
    _, kept, _ = sp.reference_step(x, 1.0, 0, 0.99, (), seed=5, row=0, step=0)
    assert int(kept.sum()) == 3  # top-p drops what has no mass


def test_parameter_validation():
    assert sp.normalize_params(None, None, None) == (1.0, 0, None)
    assert sp.normalize_params(0, 0, 1.0) == (1.0, 0, None)  # 0 / None mean "off", as in _generate_sample
    assert sp.normalize_params(0.2, 50, 0.9) == (0.2, 50, 0.9)
    for bad in (dict(temperature=-0.5), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=-0.1), dict(top_k=-1)):
        with pytest.raises(ValueError):
            sp.normalize_params(**bad)


def test_routing_is_a_pure_function_of_the_kwargs():
    base = dict(do_sample=True, seed=7, temperature=0.7)
    assert sp.device_route(base, 32000) and sp.device_route(dict(base, eos_token_id=[1, 2, 3]), 65536)
    assert not sp.device_route(dict(do_sample=True, temperature=0.7), 32000)  # no seed: torch's RNG, today's loop
    assert not sp.device_route(dict(base, generator=torch.Generator()), 32000)
    assert not sp.device_route(dict(base, eos_token_id=[1, 2, 3, 4]), 32000)
    assert not sp.device_route(dict(base, past_key_values=object()), 32000)
    assert not sp.device_route(base, 65537)
    assert not sp.device_route(dict(seed=7), 32000)  # greedy
    # the EOS set is resolved as generate() resolves it: the config's default when the call names none, and an explicit None means no EOS
    assert not sp.device_route(base, 32000, default_eos=[1, 2, 3, 4])
    assert sp.device_route(base, 32000, default_eos=[1, 2, 3]) and sp.device_route(base, 32000, default_eos=2)
    assert sp.device_route(dict(base, eos_token_id=None), 32000, default_eos=[1, 2, 3, 4])
    assert sp.device_route(dict(base, eos_token_id=2), 32000, default_eos=[1, 2, 3, 4])


def test_generate_validates_before_any_launch_and_reports_the_knob():
    """On a box without a GPU nothing can be launched: a ValueError (not a HipOpsError) shows the parameters were checked first."""
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM
    from oracle import fixtures as fx

    m = DynamicLlavaLlamaForCausalLM(DynamicLlavaConfig.from_namespace(fx.tiny_config()), with_vision_tower=False)
    m._check_ready = lambda: None
    assert m.knobs()["device_sampling"] is True
    ids = torch.tensor([[1, 5, -200, 9]])
    for bad in (dict(temperature=-1.0), dict(top_p=0.0), dict(top_k=-3), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            m.generate(ids, do_sample=True, seed=1, max_new_tokens=2, **bad)


def test_library_rejects_bad_arguments():
    from dynamic_llava_amd import hip_ops

    lib = hip_ops.load_library()
    p = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    args = lambda V, prm: (p, hip_ops.DL_BF16, V, V, 1, p, None, 0, None, None, -1, -1, -1, 0, None, None, None, 0, prm, None, None)
    assert lib.dl_decode_sample(*args(65537, p)) != 0 and b"65536" in lib.dl_last_error()
    assert lib.dl_decode_sample(*args(32000, None)) != 0 and b"parameter block" in lib.dl_last_error()
    assert lib.dl_decode_sample(*args(0, p)) != 0
    words = hip_ops.sample_params_words(0.7, 50, 0.9, seed=(5 << 32) | 9, row_base=3)
    assert words.dtype == torch.int32 and words.tolist()[1] == 50 and words.tolist()[3:6] == [9, 5, 3]
    assert words[:1].view(torch.float32).item() == pytest.approx(0.7) and hip_ops.sample_params_words(1.0).view(torch.float32)[2].item() == 1.0
    assert hip_ops.sample_params_words(0.0).view(torch.float32)[0].item() == 1.0  # one validator: generate()'s conventions (0 = off)
    for bad in (dict(temperature=-1.0), dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_k=-1)):
        with pytest.raises(ValueError):
            hip_ops.sample_params_words(**bad)
