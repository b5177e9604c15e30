"""CPU: the C ABI and binding of dl_gemm_mx8, the argument rule of set_decode_weight_format(max_batch=), the knob, and the pure-torch statement (mxfp8.py) of what the
host computes for the kernel -- split-K factor, slice bounds, workspace size -- against the C helpers."""
import inspect
import os
import re

import pytest
import torch

from dynamic_llava_amd import mxfp8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_exports():
    """include/dynllava.h declares the three entries, hip_ops' prototype table matches them, the library exports them, the ABI version is unchanged; argument
    checks run before any launch."""
    from ctypes import c_int, c_int64, c_void_p

    from dynamic_llava_amd import hip_ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dynllava.h")).read(), flags=re.S)
    want = {
        "dl_gemm_mx8_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int]),
        "dl_gemm_mx8_slices": (c_int, [c_int, c_int, c_int, c_int]),
        "dl_gemm_mx8": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    }
    for name, (res, args) in want.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
        assert hip_ops.SIGNATURES[name] == (res, args), name
    assert re.search(r"#define\s+DL_MX8_PLAIN\s+0\b", hdr) and re.search(r"#define\s+DL_MX8_PARTS\s+1\b", hdr)
    assert (hip_ops.MX8_PLAIN, hip_ops.MX8_PARTS) == (0, 1)
    for f in ("gemm_mx8", "gemm_mx8_parts", "gemm_mx8_ok"):
        assert callable(getattr(hip_ops, f)), f
    lib = hip_ops.load_library()
    assert lib.dl_version() == 4
    for name in want:
        assert hasattr(lib, name)
    p = c_void_p(256)
    bf, f32 = hip_ops.dtype_code(torch.bfloat16), hip_ops.dtype_code(torch.float32)
    big = 1 << 30
    ok_shape = (4, 64, 512)
    for args, what in [
        ((p, 512, p, p, p, 64, p, big, 4, 64, 480, 0, 0, bf, None), b"256"),  # K % 256
        ((p, 512, p, p, p, 64, p, big, 0, 64, 512, 0, 0, bf, None), b"bad shape"),
        ((p, 512, p, p, p, 64, p, big, 33, 64, 512, 0, 0, bf, None), b"bad shape"),
        ((p, 512, p, p, p, 64, p, big, *ok_shape, 0, 0, f32, None), b"bf16 / f16 only"),
        ((p, 512, p, None, p, 64, p, big, *ok_shape, 0, 0, bf, None), b"NULL"),
        ((p, 512, p, p, p, 64, p, 2 * 4 * 64 * 4 - 1, *ok_shape, 0, 0, bf, None), b"workspace"),  # automatic split-K of this shape: 2 slices
        ((p, 512, p, p, None, 0, None, 0, *ok_shape, 1, 1, bf, None), b"workspace"),  # PARTS without a workspace
        ((p, 512, p, p, p, 64, p, big, *ok_shape, 0, 7, bf, None), b"epilogue"),
        ((p, 512, p, p, p, 66, p, big, 4, 66, 512, 0, 0, bf, None), b"N %% 4".replace(b"%%", b"%")),
    ]:
        assert lib.dl_gemm_mx8(*args) == -1, what
        assert what in lib.dl_last_error(), (what, lib.dl_last_error())


SHAPES = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (15360, 5120), (5120, 5120), (27648, 5120), (5120, 13824), (132, 256), (200, 512), (132, 768), (768, 256)]


def test_host_slices_workspace_and_bounds():
    """mxfp8.gemm_mx8_slices / _workspace_bytes / _slice_bounds on their own terms: every slice is a non-empty multiple of 256, the slices tile [0, K) in order, the
    X slice of the longest one fits the LDS left beside the staging, the automatic rule is 4 slices for the wide projections and 8 otherwise."""
    for N, K in SHAPES:
        for M in (1, 4, 16, 17, 32):
            for want in (0, 1, 2, 3, 8, 64):
                s = mxfp8.gemm_mx8_slices(M, N, K, want)
                assert 1 <= s <= K // 256
                if want and want <= K // 256:
                    assert s >= want
                b = mxfp8.gemm_mx8_slice_bounds(K, s)
                assert len(b) == s and b[0][0] == 0 and b[-1][1] == K
                assert all(k1 > k0 and (k1 - k0) % 256 == 0 and k0 % 256 == 0 for k0, k1 in b)
                assert all(b[i][1] == b[i + 1][0] for i in range(s - 1))
                rows = 16 if M <= 16 else 32
                lds = 8 * (16 * (256 + 16) + 16 * 8) + rows * (max(k1 - k0 for k0, k1 in b) + 8) * 2
                assert lds <= 150 * 1024, (M, N, K, want, lds)
                assert mxfp8.gemm_mx8_workspace_bytes(M, N, K, want) == s * M * N * 4
    assert mxfp8.gemm_mx8_slices(8, 22016, 4096) == 4 and mxfp8.gemm_mx8_slices(8, 12288, 4096) == 8 and mxfp8.gemm_mx8_slices(8, 4096, 4096) == 8
    assert mxfp8.gemm_mx8_slices(32, 768, 256) == 1  # K / 256 caps the factor
    for bad in ((0, 64, 512), (33, 64, 512), (4, 64, 480), (4, 66, 512), (4, 0, 512)):
        assert mxfp8.gemm_mx8_slices(*bad) == 0 and mxfp8.gemm_mx8_workspace_bytes(*bad) == 0


def test_host_slices_match_the_c_helpers():
    from dynamic_llava_amd import hip_ops

    lib = hip_ops.load_library()
    for N, K in SHAPES + [(64, 480), (66, 512)]:
        for M in (0, 1, 4, 16, 17, 32, 33):
            for want in (0, 1, 2, 3, 5, 8, 64, 65):
                assert lib.dl_gemm_mx8_slices(M, N, K, want) == mxfp8.gemm_mx8_slices(M, N, K, want), (M, N, K, want)
                assert lib.dl_gemm_mx8_workspace_bytes(M, N, K, want) == mxfp8.gemm_mx8_workspace_bytes(M, N, K, want), (M, N, K, want)


def test_max_batch_argument_rule():
    """set_decode_weight_format(fmt, max_batch) / load_pretrained_model(decode_weight_format, decode_weight_max_batch): max_batch is None or an int in
    [gemv_max_decode_batch, 32], and needs the format."""
    from dynamic_llava_amd import builder
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM as M

    chk = mxfp8.check_decode_weight_format
    for fmt, mb in ((None, None), ("mxfp8", None), ("mxfp8", 3), ("mxfp8", 4), ("mxfp8", 32)):
        chk(fmt, mb, 3)
    for fmt, mb in ((None, 8), ("mxfp8", 2), ("mxfp8", 33), ("mxfp8", 0), ("mxfp8", -1), ("mxfp8", 8.0), ("mxfp8", "8"), ("mxfp8", True), ("fp4", None), ("fp4", 8)):
        with pytest.raises(ValueError):
            chk(fmt, mb, 3)
    sig = inspect.signature(M.set_decode_weight_format).parameters
    assert "max_batch" in sig and sig["max_batch"].default is None
    sig = inspect.signature(builder.load_pretrained_model).parameters
    assert "decode_weight_max_batch" in sig and sig["decode_weight_max_batch"].default is None
    for kw in (dict(decode_weight_format="mxfp8", decode_weight_max_batch=33), dict(decode_weight_max_batch=8), dict(decode_weight_format="mxfp8", decode_weight_max_batch=0)):
        with pytest.raises(ValueError):
            builder.load_pretrained_model("/nonexistent", **kw)

    class Stub:  # the method validates before it touches the device
        gemv_max_decode_batch = 3
        decode_weight_format = None
        mx8_max_decode_batch = None

    for fmt, mb in ((None, 8), ("mxfp8", 33), ("mxfp8", 2), ("int4", None)):
        st = Stub()
        with pytest.raises(ValueError):
            M.set_decode_weight_format(st, fmt, max_batch=mb)
        assert st.decode_weight_format is None and st.mx8_max_decode_batch is None, "a rejected call changes nothing"


def test_knobs_carry_mx8_max_decode_batch():
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM as M

    cfg = DynamicLlavaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, vocab_size=64)
    m = M(cfg, with_vision_tower=False)
    k = m.knobs()
    assert "mx8_max_decode_batch" in k and k["mx8_max_decode_batch"] is None and k["decode_weight_format"] is None
    m.mx8_max_decode_batch = 16
    assert m.knobs()["mx8_max_decode_batch"] == 16
