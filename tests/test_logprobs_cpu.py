"""CPU: the log-probability rule (dynamic_llava_amd/logprobs.py, the contract of dl_decode_logprobs) -- against torch.log_softmax in float64, its bit identity
with the scoring rule, the order of the top-n list, the post-EOS masking helper, generate()'s validation and the C entry's declaration and argument checks.

Bound against float64: score_cases.device_tol with the float64 values of lse and of the result (2 * 2^-23 + V * 2^-40 + 2^-23 on the summed masses, two ulps of
lse, one ulp of the result); no new number."""
import ctypes
import math
import os
import re

import pytest
import torch

import score_cases as cs
from dynamic_llava_amd import logprobs as lpr
from dynamic_llava_amd import scoring as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")


def _bits(t):
    return torch.as_tensor(t, dtype=torch.float32).reshape(-1).view(torch.int32)


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", [320, 32003])
def test_rule_against_float64_log_softmax(V, dtype):
    worst = 0.0
    for name, row in cs.families(V, dtype):
        truth = torch.log_softmax(row.double(), dim=0)
        lse64 = cs.truth64(row, 0)[1]
        for tok in cs.labels_for(row):
            lp, top_lp, top_ids = lpr.reference_row(row, tok, 8)
            ref = float(truth[tok])
            if math.isinf(ref):
                assert float(lp) == ref, (name, tok)
            else:
                tol = cs.device_tol(V, lse64, ref)
                err = abs(float(lp) - ref)
                worst = max(worst, err / tol)
                print(f"{name} V={V} {dtype} token {tok}: |rule - float64| = {err:.3e}, tol = {tol:.3e}")
                assert err <= tol, (name, tok, float(lp), ref, err, tol)
        for k in range(8):
            ref = float(truth[int(top_ids[k])])
            assert float(top_lp[k]) == ref if math.isinf(ref) else abs(float(top_lp[k]) - ref) <= cs.device_tol(V, lse64, ref), (name, k)
    print(f"V={V} {dtype}: worst |rule - float64| / tol = {worst:.3f}")


@pytest.mark.parametrize("dtype", cs.DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("V", [320, 32003])
def test_bit_exact_negative_of_the_scoring_rule(V, dtype):
    for name, row in cs.families(V, dtype):
        for tok in cs.labels_for(row):
            lp = lpr.reference_row(row, tok, 0)[0]
            nll = sc.reference_step(row, tok)[0]
            assert torch.equal(_bits(lp), _bits(-nll)), (name, tok, float(lp), float(nll))
    rows = torch.stack([r for _, r in cs.families(320, torch.float32)])
    toks = torch.tensor([cs.labels_for(r)[4] for r in rows])
    lp, top_lp, top_ids = lpr.reference_rows(rows, toks, 3)
    assert torch.equal(_bits(lp), _bits(-sc.reference_rows(rows, toks)[0])) and top_lp.shape == top_ids.shape == (rows.shape[0], 3)
    assert top_ids[:, 0].tolist() == sc.reference_rows(rows, toks)[1].tolist()  # entry 0 is the greedy token


def _order_by_definition(row, n):
    x = row.float().tolist()
    return sorted(range(len(x)), key=lambda v: (-x[v], v))[:n]


def test_top_n_order():
    g = torch.Generator().manual_seed(5)
    ties = torch.randint(-3, 4, (64,), generator=g).float()  # seven values over 64 entries: every one of them repeats
    run = torch.zeros(40)
    run[[31, 7, 8, 9, 22]] = 6.5  # a run of equal maxima
    ninf = torch.randn(24, generator=g)
    ninf[[0, 3, 4, 11, 23]] = NEG
    few = torch.tensor([NEG, 1.0, NEG, NEG, 1.0, 0.5])  # n reaches into the -inf entries
    for name, row in (("ties", ties), ("run", run), ("neginf", ninf), ("few", few)):
        V = row.shape[0]
        for n in (0, 1, 5, min(8, V), V):
            lp, top_lp, top_ids = lpr.reference_row(row, 1, n) if n <= 8 else (None, None, lpr.top_order(row, n))
            assert top_ids.tolist() == _order_by_definition(row, n), (name, n)
            if n <= 8:
                assert top_lp.shape == (n,) and top_ids.dtype == torch.int64 and top_lp.dtype == torch.float32
                for k in range(n):  # an entry of the list and the same token asked for directly: the same bits
                    assert torch.equal(_bits(top_lp[k]), _bits(lpr.reference_row(row, int(top_ids[k]))[0])), (name, n, k)
    assert lpr.top_order(run, 5).tolist() == [7, 8, 9, 22, 31]
    assert lpr.reference_row(few, 0, 6)[1].tolist()[3:] == [NEG, NEG, NEG] and lpr.reference_row(few, 0, 6)[2].tolist() == [1, 4, 5, 0, 2, 3]
    assert float(lpr.reference_row(few, 0)[0]) == NEG  # a token at -inf
    assert float(lpr.reference_row(few, 6)[0]) == 0.0 and float(lpr.reference_row(few, -1)[0]) == 0.0  # a token outside [0, V)
    empty = lpr.reference_rows(torch.stack([few, few]), torch.tensor([1, 4]), 0)
    assert empty[1].shape == (2, 0) and empty[2].shape == (2, 0) and empty[2].dtype == torch.int64


def _masked(seq, eos, n=2):
    seq = torch.tensor(seq)
    B, T = seq.shape
    lp = torch.arange(1, B * T + 1, dtype=torch.float32).view(B, T).neg()
    top_lp = lp[..., None].repeat(1, 1, n) - 0.5
    top_ids = torch.arange(B * T * n).view(B, T, n) + 100
    keep = (lp.clone(), top_lp.clone(), top_ids.clone())
    out = lpr.mask_after_eos(seq, eos, lp, top_lp, top_ids)
    assert out[0] is lp and out[1] is top_lp and out[2] is top_ids  # in place
    return keep, out


def _assert_masked(keep, out, dead):
    """dead [B][T]: 1 where the column lies after the row's first EOS."""
    dead = torch.tensor(dead, dtype=torch.bool)
    assert torch.equal(out[0], torch.where(dead, torch.zeros_like(keep[0]), keep[0]))
    assert torch.equal(out[1], torch.where(dead[..., None], torch.zeros_like(keep[1]), keep[1]))
    assert torch.equal(out[2], torch.where(dead[..., None], torch.full_like(keep[2], -1), keep[2]))


def test_mask_after_eos():
    EOS, PAD = 2, 0
    # EOS in the first column; never; in the last column
    _assert_masked(*_masked([[EOS, PAD, PAD, PAD], [5, 6, 7, 8], [5, 6, 7, EOS]], [EOS]), [[0, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]])
    # pad equal to the EOS id: the columns are found by position
    _assert_masked(*_masked([[5, EOS, EOS, EOS], [EOS, EOS, EOS, EOS], [5, 6, 7, 8]], [EOS]), [[0, 0, 1, 1], [0, 1, 1, 1], [0, 0, 0, 0]])
    # three EOS ids; a pad (0) in front of any EOS is a token like any other
    _assert_masked(*_masked([[5, 9, PAD, PAD], [PAD, 6, 11, PAD], [5, 6, 7, 13], [13, 9, 11, 5]], [9, 11, 13]), [[0, 0, 1, 1], [0, 0, 0, 1], [0, 0, 0, 0], [0, 1, 1, 1]])
    # no EOS set: nothing is masked
    _assert_masked(*_masked([[EOS, PAD, PAD]], []), [[0, 0, 0]])
    # without the top-n tensors
    lp = torch.full((1, 3), -1.5)
    assert lpr.mask_after_eos(torch.tensor([[EOS, 4, 4]]), [EOS], lp)[0].tolist() == [[-1.5, 0.0, 0.0]]


def test_host_result_is_the_rule_masked():
    g = torch.Generator().manual_seed(9)
    steps = [torch.randn(2, 50, generator=g) for _ in range(3)]
    seq = torch.tensor([[4, 7, 0], [1, 2, 3]])
    res = lpr.host_result(steps, seq, [7], 2)
    assert sorted(res) == ["logprobs", "top_logprob_ids", "top_logprobs"] and res["top_logprobs"].shape == (2, 3, 2) and res["top_logprob_ids"].dtype == torch.int64
    for t in range(3):
        lp, top_lp, top_ids = lpr.reference_rows(steps[t], seq[:, t], 2)
        for b in range(2):
            if b == 0 and t == 2:
                assert float(res["logprobs"][b, t]) == 0.0 and res["top_logprobs"][b, t].tolist() == [0.0, 0.0] and res["top_logprob_ids"][b, t].tolist() == [-1, -1]
            else:
                assert torch.equal(_bits(res["logprobs"][b, t]), _bits(lp[b])) and torch.equal(_bits(res["top_logprobs"][b, t]), _bits(top_lp[b]))
                assert torch.equal(res["top_logprob_ids"][b, t], top_ids[b])
    assert sorted(lpr.host_result(steps, seq, [], 0)) == ["logprobs"]


def test_generate_validates_before_any_launch_and_reports_the_knob():
    """On a box without a GPU nothing can be launched: a ValueError (not a HipOpsError) shows the keywords were checked first."""
    from dynamic_llava_amd import sampling
    from dynamic_llava_amd.config import DynamicLlavaConfig
    from dynamic_llava_amd.decode import StepMode
    from dynamic_llava_amd.model import DynamicLlavaLlamaForCausalLM
    from oracle import fixtures as fx

    cfg = fx.tiny_config()
    m = DynamicLlavaLlamaForCausalLM(DynamicLlavaConfig.from_namespace(cfg), with_vision_tower=False)
    m._check_ready = lambda: None
    assert m.knobs()["device_logprobs"] is True
    assert lpr.MAX_TOP_LOGPROBS == 8 and StepMode().logprobs == -1 and StepMode(logprobs=3) != StepMode(logprobs=0) != StepMode()
    ids = torch.tensor([[1, 5, -200, 9]])
    labels = torch.zeros((1, 2), dtype=torch.long)
    D = dict(return_dict_in_generate=True)
    bad = [dict(output_logprobs=True),  # without return_dict_in_generate
           dict(D, output_logprobs=True, top_logprobs=-1), dict(D, output_logprobs=True, top_logprobs=9), dict(D, output_logprobs=True, top_logprobs=2.0),
           dict(D, output_logprobs=True, top_logprobs="2"), dict(D, output_logprobs=True, top_logprobs=True), dict(D, output_logprobs=True, top_logprobs=None),
           dict(D, top_logprobs=2), dict(D, output_logprobs=False, top_logprobs=1),  # alternatives without the log-probabilities
           dict(D, output_logprobs=True, _score_labels=labels), dict(D, top_logprobs=3, _score_labels=labels),
           dict(D, output_logprobs=1)]
    for kw in bad:
        for route in (dict(), dict(do_sample=True, seed=1), dict(do_sample=True), dict(eos_token_id=[2, 3, 4, 5])):
            with pytest.raises(ValueError):
                m.generate(ids, max_new_tokens=2, **kw, **route)
    with pytest.raises(ValueError):  # the continuation route validates too, before it looks at its cache
        m.generate(ids, max_new_tokens=2, past_key_values=object(), **D, output_logprobs=True, top_logprobs=9)
    small, wide = lpr.validate, DynamicLlavaConfig.from_namespace(cfg)
    assert small(dict(D, output_logprobs=True, top_logprobs=8), 320) == 8 and small(dict(D, output_logprobs=True), 320) == 0 and small(dict(D), 320) == -1
    assert small(dict(top_logprobs=0), 320) == -1
    with pytest.raises(ValueError):  # more alternatives than tokens
        small(dict(D, output_logprobs=True, top_logprobs=5), 4)
    with pytest.raises(ValueError):  # 64-bit fixed-point masses
        small(dict(D, output_logprobs=True), sampling.MAX_VOCAB + 1)
    wide.vocab_size = sampling.MAX_VOCAB + 1
    m.config = wide
    with pytest.raises(ValueError):
        m.generate(ids, max_new_tokens=2, **D, output_logprobs=True)
    wide.vocab_size = 4
    with pytest.raises(ValueError):
        m.generate(ids, max_new_tokens=2, **D, output_logprobs=True, top_logprobs=5)


def test_c_abi_entry():
    """include/dynllava.h declares dl_decode_logprobs, hip_ops' prototype table matches its argument count, the library exports it and refuses bad arguments
    before any launch (no device needed: the pointers are never dereferenced)."""
    from ctypes import c_int, c_int64, c_void_p

    from dynamic_llava_amd import hip_ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dynllava.h")).read(), flags=re.S)
    want = (c_int, [c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p])
    m = re.search(r"\bdl_decode_logprobs\s*\(([^)]*)\)", hdr)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(want[1])
    assert hip_ops.SIGNATURES["dl_decode_logprobs"] == want
    assert int(re.search(r"#define\s+DL_MAX_TOP_LOGPROBS\s+(\d+)", hdr).group(1)) == lpr.MAX_TOP_LOGPROBS
    assert callable(hip_ops.decode_logprobs)
    lib = hip_ops.load_library()
    assert lib.dl_version() == 4 and hip_ops.ABI_VERSION == 4 and hasattr(lib, "dl_decode_logprobs")
    p = ctypes.c_void_p(16)

    def call(V=320, B=1, logits=p, ids=p, step=p, cap=4, lp=p, n=0, stride=8, top_lp=p, top_ids=p, dtype=hip_ops.DL_BF16):
        return lib.dl_decode_logprobs(logits, dtype, V, V, B, ids, step, cap, lp, n, stride, top_lp, top_ids, None)

    for kw in (dict(logits=None), dict(ids=None), dict(step=None), dict(lp=None), dict(V=0), dict(B=0), dict(cap=0), dict(dtype=7), dict(n=-1), dict(n=9),
               dict(V=4, n=5), dict(n=5, stride=4), dict(n=1, top_lp=None), dict(n=1, top_ids=None)):
        assert call(**kw) == -1, kw
    assert call(V=65537) == -1 and b"65536" in lib.dl_last_error()
    assert call(n=9) == -1 and b"0..8" in lib.dl_last_error()
