"""CPU: the MXFP8 host reference (dynamic_llava_amd/mxfp8.py) on hand-made blocks and random tensors, and the C ABI of the MXFP8 entries."""
import os
import re

import pytest
import torch

from dynamic_llava_amd.mxfp8 import dequantize_mx8, e_min, quantize_mx8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(vals, dtype=torch.float32):
    """one row, one 32-element block: vals first, zeros after"""
    w = torch.zeros(1, 32, dtype=torch.float32)
    w[0, : len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return w.to(dtype)


def _one(vals, dtype=torch.float32):
    q, s = quantize_mx8(_block(vals, dtype), dtype)
    return q[0].tolist(), int(s[0, 0]) - 127


def test_all_zero_block():
    q, e = _one([])
    assert e == 0 and q == [0] * 32
    q, s = quantize_mx8(torch.zeros(3, 64, dtype=torch.bfloat16))
    assert int(q.abs().sum()) == 0 and s.tolist() == [[127, 127]] * 3


def test_power_of_two_amax():
    # amax = 2^k -> e = k - 8 and the amax element is 2^8 = 256: e4m3 code 0x78 (exponent field 15, mantissa 0)
    for k in (-3, 0, 5):
        q, e = _one([2.0**k, -(2.0**k), 2.0 ** (k - 1)])
        assert e == k - 8
        assert q[:3] == [0x78, 0xF8, 0x70]


def test_rne_midpoints_ties_to_even():
    # e = 0 (amax in [256, 512)).  Between 256 (0x78) and 288 (0x79) the midpoint 272 goes to 256 (even mantissa); between 288 and 320 (0x7A) 304 goes to 320.
    q, e = _one([256.0, 272.0, 304.0, 280.0, 273.0, -272.0])
    assert e == 0
    assert q == [0x78, 0x78, 0x7A, 0x79, 0x79, 0xF8] + [0] * 26
    # in the normal range near 1: 1 (0x38), 1.0625 = midpoint of 1 and 1.125 -> 1; 1.1875 = midpoint of 1.125 and 1.25 -> 1.25 (0x3A)
    q, e = _one([256.0, 1.0625, 1.1875])
    assert e == 0 and q[1:3] == [0x38, 0x3A]


def test_saturates_to_448():
    # amax = 500 in [256, 512): e = 0; 500 / 1 would round to 512, which e4m3fn does not have: saturate to 448 (0x7E); 464 (the 448 / 480 midpoint) likewise
    q, e = _one([500.0, -470.0, 464.0, 448.0, 440.0])
    assert e == 0
    assert q[:5] == [0x7E, 0xFE, 0x7E, 0x7E, 0x7E]  # 440 -> 448 (RNE between 416 and 448)


def test_e4m3_subnormals():
    # e = 0: values below 2^-6 are subnormal multiples of 2^-9 (codes 1..7); 2^-10 is the tie between 0 and 2^-9 -> 0; 3 * 2^-10 -> 2^-8 (code 2, even)
    q, e = _one([256.0, 2.0**-9, 3 * 2.0**-9, 7 * 2.0**-9, 2.0**-10, 3 * 2.0**-10, -(2.0**-9), 2.0**-6, 15 * 2.0**-10])
    assert e == 0
    assert q[:9] == [0x78, 1, 3, 7, 0, 2, 0x81, 0x08, 0x08]  # 15 * 2^-10 = 7.5 * 2^-9 -> 8 * 2^-9 = 2^-6 (code 0x08)


def test_fp16_e_min_clamp():
    assert e_min(torch.float16) == -15 and e_min(torch.bfloat16) == -124 and e_min(torch.float32) == -124
    # amax = 2^-10: bf16 / fp32 give e = -18; fp16 clamps to -15, so the element becomes 2^5 = 32 (code 0x60) instead of 256
    q, e = _one([2.0**-10, 2.0**-20], torch.bfloat16)
    assert e == -18 and q[:2] == [0x78, 0x28]  # 2^-20 / 2^-18 = 2^-2: exponent field 5
    q, e = _one([2.0**-10, 2.0**-20], torch.float16)
    assert e == -15 and q[:2] == [0x60, 0x10]  # 2^-20 / 2^-15 = 2^-5: exponent field 2


def test_fp16_e_min_clamp_values():
    w = torch.tensor([[2.0**-10, 2.0**-16, 2.0**-24] + [0.0] * 29], dtype=torch.float16)
    q, s = quantize_mx8(w)
    assert int(s[0, 0]) - 127 == -15
    # 2^-10 / 2^-15 = 32 (0x60), 2^-16 / 2^-15 = 0.5 (0x30), 2^-24 / 2^-15 = 2^-9 (smallest subnormal, code 1)
    assert q[0, :3].tolist() == [0x60, 0x30, 0x01]
    wp = dequantize_mx8(q, s, torch.float16)
    assert torch.equal(wp.float(), w.float())


def _ref_codes_with_torch_cast(w, q, s):
    """torch's float8_e4m3fn cast applied where |w / 2^e| <= 448 (the cast is only trusted there)"""
    N, K = w.shape
    e = s.to(torch.int32) - 127
    x = w.float().reshape(N, K // 32, 32) / torch.pow(2.0, e.double()).float()[..., None]
    ok = (x.abs() <= 448) & (w.float().reshape(N, K // 32, 32).abs().amax(-1, keepdim=True) > 0)
    t = x.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    return t, ok


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_random_agrees_with_torch_cast(dtype):
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(96, 512, generator=g) * torch.logspace(-4, 1, 96)[:, None]).to(dtype)
    w[5, 40:50] = 0
    q, s = quantize_mx8(w, dtype)
    t, ok = _ref_codes_with_torch_cast(w, q, s)
    qq = q.reshape(t.shape)
    assert int(ok.sum()) > 0.9 * ok.numel()
    assert torch.equal(qq[ok], t[ok])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_dequantized_is_exact_in_dtype_and_idempotent(dtype):
    g = torch.Generator().manual_seed(11)
    rows = [torch.randn(32, 256, generator=g) * 10.0 ** float(k) for k in (-7, -5, -3, -1, 1, 3)]
    w = torch.cat(rows)
    if dtype == torch.float16:
        w = w.clamp(-6e4, 6e4)
    w = w.to(dtype)
    q, s = quantize_mx8(w, dtype)
    w32 = dequantize_mx8(q, s, torch.float32)
    wp = dequantize_mx8(q, s, dtype)
    assert torch.equal(w32.to(dtype).to(torch.float32), w32)  # exact in the dtype: the cast changes no bit
    assert torch.equal(wp.to(torch.float32), w32)
    q2, s2 = quantize_mx8(wp, dtype)
    assert torch.equal(q, q2) and torch.equal(s, s2)
    # and W' is close to W: half an e4m3 step of the largest binade is amax / 16; the saturation at 448 (amax / 2^e up to 512) costs up to amax / 8
    amax = w.float().reshape(-1, 32).abs().amax(-1, keepdim=True)
    err = (w32 - w.float()).reshape(-1, 32).abs()
    small = amax > 2.0**-100 if dtype != torch.float16 else amax > 2.0**-6
    assert bool((err <= amax * 2.0**-3)[small.expand_as(err)].all())


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nan_inf_raise(bad):
    w = torch.randn(4, 64)
    w[2, 17] = bad
    with pytest.raises(ValueError):
        quantize_mx8(w)


def test_bad_shape_raises():
    with pytest.raises(ValueError):
        quantize_mx8(torch.randn(4, 48))
    with pytest.raises(ValueError):
        quantize_mx8(torch.randn(4, 64), torch.int8)


def test_header_binding_and_exports():
    """include/dynllava.h declares the MXFP8 entries, hip_ops' prototype table matches them, the library exports them, the ABI version is unchanged."""
    from ctypes import c_float, c_int, c_int64, c_void_p

    from dynamic_llava_amd import hip_ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dynllava.h")).read(), flags=re.S)
    want = {
        "dl_mx8_e_min": (c_int, [c_int]),
        "dl_quantize_mx8": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
        "dl_gemv_mx8": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int, c_int,
                                c_int, c_void_p]),
    }
    for name, (res, args) in want.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
        assert hip_ops.SIGNATURES[name] == (res, args), name
    lib = hip_ops.load_library()
    assert lib.dl_version() == 4
    for name in want:
        assert hasattr(lib, name)
    assert lib.dl_mx8_e_min(hip_ops.dtype_code(torch.float16)) == e_min(torch.float16)
    assert lib.dl_mx8_e_min(hip_ops.dtype_code(torch.bfloat16)) == e_min(torch.bfloat16)
    assert lib.dl_mx8_e_min(hip_ops.dtype_code(torch.float32)) == e_min(torch.float32)
    # argument checks run before any launch (no device needed): K % 32, NULL scale, B over the maximum, unknown dtype
    p = c_void_p(16)
    assert lib.dl_gemv_mx8(0, p, p, 64, 48, p, 48, None, None, None, None, 0.0, p, 64, 1, 2, 0, None) == -1
    assert b"multiple of 32" in lib.dl_last_error()
    assert lib.dl_gemv_mx8(0, p, None, 64, 64, p, 64, None, None, None, None, 0.0, p, 64, 1, 2, 0, None) == -1
    assert lib.dl_gemv_mx8(0, p, p, 64, 4096, p, 4096, None, None, None, None, 0.0, p, 64, 9, 2, 0, None) == -1
    assert lib.dl_gemv_mx8(0, p, p, 64, 64, p, 64, None, None, None, None, 0.0, p, 64, 1, 7, 0, None) == -1
    assert lib.dl_gemv_mx8(2, p, p, 64, 64, p, 64, None, None, None, None, 0.0, p, 64, 1, 2, 0, None) == -1  # SILUMUL prologue: not part of this contract
    assert lib.dl_quantize_mx8(p, 4, 48, 2, 2, p, p, None, None) == -1


def test_format_api_surface():
    """set_decode_weight_format / load_pretrained_model's decode_weight_format validate their argument; load_8bit / load_4bit keep raising."""
    import inspect

    from dynamic_llava_amd import builder
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM as M

    assert "decode_weight_format" in inspect.signature(builder.load_pretrained_model).parameters
    with pytest.raises(ValueError):
        builder.load_pretrained_model("/nonexistent", decode_weight_format="int4")
    with pytest.raises(NotImplementedError):
        builder.load_pretrained_model("/nonexistent", load_8bit=True)
    with pytest.raises(NotImplementedError):
        builder.load_pretrained_model("/nonexistent", load_4bit=True)
    assert hasattr(M, "set_decode_weight_format") and hasattr(M, "decode_weight_bytes")
