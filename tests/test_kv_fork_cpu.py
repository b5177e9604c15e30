"""CPU: generate(num_return_sequences=n) before any launch -- dl_kv_fork's place in the C ABI and its argument checks (which run in front of every device call), and
the request table: how the keyword parses, what it refuses, where it routes, and that a host route sees every prompt n times."""
import dataclasses
import os
import re
from ctypes import c_int, c_int64, c_void_p

import pytest
import torch

from dynamic_llava_amd import hip_ops, request
from dynamic_llava_amd.config import DynamicLlavaConfig
from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM
from oracle import fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DL_ERR_ARG = -1  # include/dynllava.h


def test_header_binding_and_library_agree_on_dl_kv_fork():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dynllava.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+dl_kv_fork\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, "include/dynllava.h does not declare dl_kv_fork"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = hip_ops.SIGNATURES["dl_kv_fork"]
    assert res is c_int and len(args) == len(params) == 24
    for p, a in zip(params, args):  # pointers, 64-bit strides and ints, in the header's order
        assert a is (c_void_p if "*" in p else c_int64 if p.startswith("int64_t") else c_int), (p, a)
    lib = hip_ops.load_library()
    assert hasattr(lib, "dl_kv_fork") and lib.dl_version() == hip_ops.ABI_VERSION == 4  # an added export: the ABI version stays


GOOD = dict(src=0x1000, dst=0x2000, ss=(4096, 2048, 1024, 512), ds=(8192, 4096, 1024, 512), n_layers=3, sparse_layer=1, B_src=1, n_rep=2, n_kv_heads=2, row_bytes=16, src_T_cap=8,
            dst_T_cap=8, src_lens=0x3000, src_lens_stride=1, dst_lens=None, dst_lens_stride=0, max_len=8)
BAD = [("src", None), ("dst", None), ("src_lens", None), ("n_rep", 0), ("n_rep", -2), ("B_src", 0), ("row_bytes", 0), ("sparse_layer", -1), ("sparse_layer", 4),
       ("ss", (4096, 2048, -1024, 512)), ("ss", (-1, 2048, 1024, 512)), ("ds", (8192, -4096, 1024, 512)), ("ds", (8192, 4096, 1024, -512)), ("src_T_cap", -1), ("dst_T_cap", -3)]


@pytest.mark.parametrize("name,value", BAD, ids=[f"{n}={v}" for n, v in BAD])
def test_bad_arguments_are_refused_before_any_device_call(name, value):
    """Every refusal returns DL_ERR_ARG and leaves a message; the pointers are never dereferenced and nothing is launched (the addresses are not memory)."""
    a = dict(GOOD, **{name: value})
    rc = hip_ops.load_library().dl_kv_fork(a["src"], a["dst"], *a["ss"], *a["ds"], a["n_layers"], a["sparse_layer"], a["B_src"], a["n_rep"], a["n_kv_heads"], a["row_bytes"],
                                           a["src_T_cap"], a["dst_T_cap"], a["src_lens"], a["src_lens_stride"], a["dst_lens"], a["dst_lens_stride"], a["max_len"], None)
    assert rc == DL_ERR_ARG and b"dl_kv_fork" in hip_ops.lib().dl_last_error()


def test_sparse_layer_may_be_either_end():
    """sparse_layer = 0 and = n_layers are valid (all layers in one group): their refusal would be an off-by-one.  Checked through the NEXT check failing instead."""
    for sl in (0, 3):
        a = dict(GOOD, sparse_layer=sl, src_T_cap=-1)
        rc = hip_ops.load_library().dl_kv_fork(a["src"], a["dst"], *a["ss"], *a["ds"], 3, sl, 1, 2, 2, 16, -1, 8, a["src_lens"], 1, None, 0, 8, None)
        assert rc == DL_ERR_ARG and b"capacity" in hip_ops.lib().dl_last_error()


# ---- the request table ------------------------------------------------------------------------------------------------------------------------------
def _mcfg():
    return DynamicLlavaConfig.from_namespace(fx.tiny_config())


def test_none_and_one_are_the_request_without_the_keyword():
    mcfg = _mcfg()
    for kw in (dict(max_new_tokens=4), dict(max_new_tokens=4, do_sample=True, seed=3, temperature=0.7), dict(max_new_tokens=4, do_sample=True), dict(max_new_tokens=4, repetition_penalty=1.2),
               dict(max_new_tokens=4, _score_labels=torch.zeros(1, 4, dtype=torch.long)), dict(max_new_tokens=4, past_key_values=object())):
        base = request.parse(kw, mcfg)
        assert base.n_return == 1
        for n in (None, 1):
            got = request.parse(dict(kw, num_return_sequences=n), mcfg)
            assert all(getattr(got, f.name) is getattr(base, f.name) or getattr(got, f.name) == getattr(base, f.name) for f in dataclasses.fields(request.Request)), (kw, n)
    assert request.parse(dict(max_new_tokens=4, do_sample=True, seed=1, num_return_sequences=3), mcfg).n_return == 3


REFUSED = [
    (dict(num_return_sequences=0, do_sample=True, seed=1), ValueError),
    (dict(num_return_sequences=-2, do_sample=True, seed=1), ValueError),
    (dict(num_return_sequences=True, do_sample=True, seed=1), ValueError),  # a bool is not a count
    (dict(num_return_sequences=2.0, do_sample=True, seed=1), ValueError),
    (dict(num_return_sequences=2), ValueError),  # greedy search returns one sequence (HF's rule)
    (dict(num_return_sequences=2, do_sample=False, seed=1), ValueError),
    (dict(num_return_sequences=2, do_sample=True, seed=1, _score_labels=torch.zeros(1, 4, dtype=torch.long)), ValueError),
    (dict(num_return_sequences=2, do_sample=True, seed=1, past_key_values=object()), NotImplementedError),
    (dict(num_return_sequences=2, do_sample=True, past_key_values=object()), NotImplementedError),
]


@pytest.mark.parametrize("kw,exc", REFUSED, ids=[",".join(f"{k}={v}" if k == "num_return_sequences" else k for k, v in r[0].items()) for r in REFUSED])
def test_refusals(kw, exc):
    with pytest.raises(exc):
        request.parse(dict(kw, max_new_tokens=4), _mcfg())
    with pytest.raises(exc):  # ... and generate() raises it before it touches a device
        m = DynamicLlavaLlamaForCausalLM(_mcfg(), with_vision_tower=False)
        m._check_ready = lambda *a, **k: None
        m.generate(torch.tensor([[1, 5, -200, 9]]), **dict(kw, max_new_tokens=4))


class _Device(Exception):
    pass


class _Cache:
    def __init__(self, rows):
        self.full_len_host = [7] * rows

    def __getitem__(self, i):
        return [torch.full((len(self.full_len_host),), 3)]


def test_seeded_request_takes_the_device_route_and_a_generator_the_host_loop_with_n_times_the_rows(monkeypatch):
    cfg, mcfg = fx.tiny_config(), _mcfg()
    assert request.parse(dict(max_new_tokens=2, do_sample=True, seed=1, num_return_sequences=3), mcfg).route == "device"
    m = DynamicLlavaLlamaForCausalLM(mcfg, with_vision_tower=False)
    m._check_ready = lambda *a, **k: None
    seen = {}

    def device(B, t_need):
        seen["pooled_rows"] = B
        raise _Device()

    m._pooled_cache = device
    ids = torch.tensor([[1, 5, -200, 9], [2, 6, -200, 8]])
    am = torch.tensor([[1, 1, 1, 1], [1, 1, 1, 0]])
    feats = torch.arange(2.0)[:, None, None].expand(2, 4, cfg.hidden_size).contiguous()
    with pytest.raises(_Device):
        m.generate(ids, image_features=feats, max_new_tokens=2, do_sample=True, seed=1, num_return_sequences=3)
    assert seen["pooled_rows"] == 6, "the decode cache of a forked request has B * n rows"
    with pytest.raises(_Device):
        m.generate(ids, image_features=feats, max_new_tokens=2, do_sample=True, seed=1)
    assert seen["pooled_rows"] == 2

    # generator=: the host loop, on every prompt three times in a row (HF's order), mask and features with them
    def forward(input_ids, attention_mask=None, images=None, image_features=None, past_key_values=None):
        if past_key_values is None:
            seen.update(ids=input_ids.clone(), am=attention_mask.clone(), feats=image_features.clone())
        return type("Out", (), dict(logits=torch.zeros(input_ids.shape[0], 4, mcfg.vocab_size), past_key_values=_Cache(input_ids.shape[0])))()

    def host_loop(logits, advance, req, max_new, greedy):
        seen.update(loop_rows=logits.shape[0], greedy=greedy, n=req.n_return)
        return [torch.zeros(logits.shape[0], dtype=torch.long)] * max_new, [], []

    m.forward = forward
    monkeypatch.setattr(request, "host_loop", host_loop)
    out = m.generate(ids, image_features=feats, attention_mask=am, max_new_tokens=2, do_sample=True, seed=1, generator=torch.Generator(), num_return_sequences=3)
    assert seen["loop_rows"] == 6 and seen["greedy"] is False and seen["n"] == 3 and out.shape == (6, 2)
    assert torch.equal(seen["ids"], ids.repeat_interleave(3, dim=0)) and torch.equal(seen["am"], am.repeat_interleave(3, dim=0))
    assert seen["feats"][:, 0, 0].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
    # ... and so does an unseeded request
    m.generate(ids, image_features=feats, attention_mask=am, max_new_tokens=2, do_sample=True, num_return_sequences=2)
    assert seen["loop_rows"] == 4


def test_knob_and_docstring():
    m = DynamicLlavaLlamaForCausalLM(_mcfg(), with_vision_tower=False)
    assert m.knobs()["device_fork"] is True
    assert "num_return_sequences" in DynamicLlavaLlamaForCausalLM.generate.__doc__
