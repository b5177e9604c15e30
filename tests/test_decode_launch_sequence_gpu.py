"""GPU, model level: the decode step's launch sequence, pinned.  For every route of the step the names of the C entries that ONE decode step (the second of a
short generate(), eager launches) and the first-token launch call, in order, must equal the literal lists below; one more test pins which launches the two
grid caps (gu_grid_cap, qkv_attn_grid_cap) reach.

The lists in EXPECTED were recorded with this file's own recorder on the commit BEFORE the step was rewritten around _layer_streams / ops.gemv_any (the one
that still had _decode_layer_mx8 and a branch per storage), never on the code under test: they say what the step launched then, and the rewrite must launch
the same.  To re-record after a deliberate change of the sequence, print `_record(...)` on the commit before that change.

Model: the smallest shape every route still takes -- H = 1024 (K % 1024 == 0: q|k|v, gate|up and the lm_head pack; K <= 5120: the fused predictor launch),
8 heads of 128, I = 2048, 3 layers (sparse_layer = 2), a 1024-word vocabulary; bf16 unless a case says otherwise; 576 image features + a 57-token prompt."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fixtures as fx  # noqa: E402

from dynamic_llava_amd import hip_ops as ops  # noqa: E402

N_NEW = 4  # the first token + three decode steps


def _build(dtype):
    from dynamic_llava_amd.builder import build_from_state_dict
    from dynamic_llava_amd.config import DynamicLlavaConfig

    cfg = fx.make_config(hidden_size=1024, intermediate_size=2048, num_hidden_layers=3, num_attention_heads=8, vocab_size=1024)
    sd = fx.make_state_dict(cfg, seed=7, predictor_gain=50.0)
    model = build_from_state_dict(DynamicLlavaConfig.from_namespace(cfg), sd, None, dtype=dtype, device="cuda")
    g = torch.Generator().manual_seed(21)
    feats = torch.randn(4, 576, 1024, generator=g).to(dtype).cuda()
    ids = fx.make_prompt(cfg, 35, 20, seed=4)[None].repeat(4, 1).cuda()
    return cfg, model, feats, ids


@pytest.fixture(scope="module")
def net():
    return _build(torch.bfloat16)


@pytest.fixture(scope="module")
def net_mx8():
    """A model of its own: the format overwrites the weights."""
    cfg, model, feats, ids = _build(torch.bfloat16)
    model.set_decode_weight_format("mxfp8")
    return cfg, model, feats, ids


def _record(model, run):
    """run() with eager launches -> (the C entries _first_token called, the C entries the SECOND _decode_step_kernels call made): every wrapper of hip_ops
    reports its entry's name to ops._check."""
    first, step, sink, n_steps = [], [], [None], [0]
    check, cls = ops._check, type(model)

    def spy_check(rc, what):
        if sink[0] is not None:
            sink[0].append(what)
        return check(rc, what)

    def first_token(*a, **k):
        sink[0] = first
        try:
            return cls._first_token(model, *a, **k)
        finally:
            sink[0] = None

    def step_kernels(*a, **k):
        n_steps[0] += 1
        sink[0] = step if n_steps[0] == 2 else None
        try:
            return cls._decode_step_kernels(model, *a, **k)
        finally:
            sink[0] = None

    graph = model.use_hip_graph
    ops._check, model._first_token, model._decode_step_kernels, model.use_hip_graph = spy_check, first_token, step_kernels, False
    try:
        run()
        torch.cuda.synchronize()
        model.check_device_errors()
    finally:
        ops._check, model.use_hip_graph = check, graph
        del model._first_token, model._decode_step_kernels
    assert n_steps[0] == N_NEW - 1
    return first, step


@contextlib.contextmanager
def _knobs(model, refinalize=False, **kw):
    """Model attributes set for the block and restored after it (refinalize: the packed copies are made / dropped by finalize())."""
    old = {k: getattr(model, k) for k in kw}

    def put(vals):
        for k, v in vals.items():
            setattr(model, k, v)
        if refinalize:
            model._packed = False
            model.finalize()

    put(kw)
    try:
        yield
    finally:
        put(old)


def _generate(net, B=1, **kw):
    cfg, model, feats, ids = net
    return _record(model, lambda: model.generate(ids[:B], image_features=feats[:B], max_new_tokens=N_NEW, eos_token_id=None, **kw))


# case -> (the first-token launch, the second decode step)
EXPECTED = {
    "defaults": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk",
        "dl_gemv", "dl_gemv_gu_tp_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_advance"],
    ),
    "pack_off": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_qkv_attn", "dl_gemv", "dl_gemv", "dl_gemv", "dl_gemv_qkv_attn", "dl_gemv", "dl_gemv", "dl_gemv", "dl_gemv_qkv_attn", "dl_gemv",
        "dl_gemv_gu_tp", "dl_gemv", "dl_gemv", "dl_decode_advance"],
    ),
    "pack_qkv_off": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_qkv_attn", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn", "dl_gemv",
        "dl_gemv_gu_tp_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_advance"],
    ),
    "pack_plain_on": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_qkv_attn_pk", "dl_gemv_pk", "dl_gemv_pk", "dl_gemv_pk", "dl_gemv_qkv_attn_pk", "dl_gemv_pk", "dl_gemv_pk", "dl_gemv_pk",
        "dl_gemv_qkv_attn_pk", "dl_gemv_pk", "dl_gemv_gu_tp_pk", "dl_gemv_pk", "dl_gemv_pk", "dl_decode_advance"],
    ),
    "fuse_qkv_attn_off": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_pk", "dl_attn_decode_rope", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_pk", "dl_attn_decode_rope", "dl_gemv", "dl_gemv_pk", "dl_gemv",
        "dl_gemv_pk", "dl_attn_decode_rope", "dl_gemv", "dl_gemv_gu_tp_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_advance"],
    ),
    "fuse_gu_tp_off": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk",
        "dl_text_predictor_decide", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_advance"],
    ),
    "tp_side_stream_on": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk",
        "dl_text_predictor_decide", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_advance"],
    ),
    "several_splits": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_pk", "dl_attn_decode_rope", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_pk", "dl_attn_decode_rope", "dl_gemv", "dl_gemv_pk", "dl_gemv",
        "dl_gemv_pk", "dl_attn_decode_rope", "dl_gemv", "dl_gemv_gu_tp_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_advance"],
    ),
    "mxfp8_kv": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_pk", "dl_attn_decode_rope_kv8", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_pk", "dl_attn_decode_rope_kv8", "dl_gemv", "dl_gemv_pk",
        "dl_gemv", "dl_gemv_pk", "dl_attn_decode_rope_kv8", "dl_gemv", "dl_gemv_gu_tp_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_advance"],
    ),
    "sampled": (
        ["dl_gemv", "dl_decode_sample"],
        ["dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk",
        "dl_gemv", "dl_gemv_gu_tp_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_sample"],
    ),
    "score": (
        ["dl_gemv", "dl_decode_score"],
        ["dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk", "dl_gemv", "dl_gemv_pk", "dl_gemv", "dl_gemv_qkv_attn_pk",
        "dl_gemv", "dl_gemv_gu_tp_pk", "dl_gemv", "dl_gemv_pk", "dl_decode_score"],
    ),
    "batch_2": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv", "dl_attn_decode_rope", "dl_gemv", "dl_gemv", "dl_gemv", "dl_gemv", "dl_attn_decode_rope", "dl_gemv", "dl_gemv", "dl_gemv", "dl_gemv",
        "dl_text_predictor_decide", "dl_attn_decode_rope", "dl_gemv", "dl_gemv", "dl_gemv", "dl_gemv", "dl_decode_advance"],
    ),
    "batch_4": (
        ["dl_decode_advance"],
        ["dl_rmsnorm", "dl_gemm_smallm", "dl_attn_decode_rope", "dl_gemm_smallm", "dl_add_rmsnorm_parts_packed", "dl_linear_packed", "dl_linear_packed",
        "dl_add_rmsnorm_parts", "dl_gemm_smallm", "dl_attn_decode_rope", "dl_gemm_smallm", "dl_add_rmsnorm_parts_packed", "dl_linear_packed",
        "dl_linear_packed", "dl_add_rmsnorm_parts", "dl_text_predictor_decide", "dl_gemm_smallm", "dl_attn_decode_rope", "dl_gemm_smallm",
        "dl_add_rmsnorm_parts_packed", "dl_linear_packed", "dl_linear_packed", "dl_add_rmsnorm_parts", "dl_gemm_smallm", "dl_decode_advance"],
    ),
    "fp16": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_qkv_attn", "dl_gemv", "dl_gemv", "dl_gemv", "dl_gemv_qkv_attn", "dl_gemv", "dl_gemv", "dl_gemv", "dl_gemv_qkv_attn", "dl_gemv",
        "dl_gemv_gu_tp", "dl_gemv", "dl_gemv", "dl_decode_advance"],
    ),
    "mxfp8_weights": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_mx8", "dl_attn_decode_rope", "dl_gemv_mx8", "dl_gemv_mx8", "dl_gemv_mx8", "dl_gemv_mx8", "dl_attn_decode_rope", "dl_gemv_mx8",
        "dl_gemv_mx8", "dl_gemv_mx8", "dl_gemv_mx8", "dl_text_predictor_decide", "dl_attn_decode_rope", "dl_gemv_mx8", "dl_gemv_mx8", "dl_gemv_mx8",
        "dl_gemv", "dl_decode_advance"],
    ),
    "mxfp8_weights_tp_side_stream_on": (
        ["dl_gemv", "dl_decode_advance"],
        ["dl_gemv_mx8", "dl_attn_decode_rope", "dl_gemv_mx8", "dl_gemv_mx8", "dl_gemv_mx8", "dl_gemv_mx8", "dl_attn_decode_rope", "dl_gemv_mx8",
        "dl_gemv_mx8", "dl_gemv_mx8", "dl_gemv_mx8", "dl_text_predictor_decide", "dl_attn_decode_rope", "dl_gemv_mx8", "dl_gemv_mx8", "dl_gemv_mx8",
        "dl_gemv", "dl_decode_advance"],
    ),
}


def _check_case(name, got):
    want = EXPECTED[name]
    assert got[0] == want[0], (name, "first token", got[0])
    assert got[1] == want[1], (name, "decode step", got[1])


def test_defaults(net):
    _check_case("defaults", _generate(net))


def test_weight_pack_off(net):
    with _knobs(net[1], refinalize=True, decode_weight_pack=False):
        _check_case("pack_off", _generate(net))


def test_weight_pack_qkv_off(net):
    with _knobs(net[1], refinalize=True, decode_weight_pack_qkv=False):
        _check_case("pack_qkv_off", _generate(net))


def test_weight_pack_plain_on(net):
    with _knobs(net[1], refinalize=True, decode_weight_pack_plain=True):
        _check_case("pack_plain_on", _generate(net))


def test_fuse_qkv_attn_off(net):
    with _knobs(net[1], fuse_qkv_attn=False):
        _check_case("fuse_qkv_attn_off", _generate(net))


def test_fuse_gu_tp_off(net):
    with _knobs(net[1], fuse_gu_tp=False):
        _check_case("fuse_gu_tp_off", _generate(net))


def test_tp_side_stream_on(net):
    with _knobs(net[1], tp_side_stream=True):
        _check_case("tp_side_stream_on", _generate(net))


def test_attention_stands_alone_with_several_splits(net):
    with _knobs(net[1], single_split_keys_override=64):
        got = _generate(net)
        cache = net[1]._cache_pool
        assert cache.n_splits(0, net[0].num_attention_heads) > 1  # (the override took: the rows are past what one workgroup per head takes)
    _check_case("several_splits", got)


def test_mxfp8_kv_cache(net):
    model = net[1]
    try:
        model.set_kv_cache_format("mxfp8")
        got = _generate(net)
    finally:
        model.set_kv_cache_format(None)
    _check_case("mxfp8_kv", got)


def test_sampled(net):
    _check_case("sampled", _generate(net, do_sample=True, seed=11, temperature=0.8, top_k=20))


def test_score(net):
    cfg, model, feats, ids = net
    labels = fx.make_forced_tokens(cfg, N_NEW, 1, seed=6).t().contiguous()
    _check_case("score", _record(model, lambda: model.score(ids[:1], labels, image_features=feats[:1])))


def test_batch_2(net):
    _check_case("batch_2", _generate(net, B=2))


def test_batch_4_gemm_step(net):
    _check_case("batch_4", _generate(net, B=4))


def test_fp16_packs_nothing():
    _check_case("fp16", _generate(_build(torch.float16)))


def test_mxfp8_weights(net_mx8):
    _check_case("mxfp8_weights", _generate(net_mx8))


def test_mxfp8_weights_tp_side_stream_on(net_mx8):
    with _knobs(net_mx8[1], tp_side_stream=True):
        _check_case("mxfp8_weights_tp_side_stream_on", _generate(net_mx8))


# ---------------------------------------------------------------- the grid caps
_WRAPPERS = ("gemv", "gemv_pk", "gemv_mx8", "gemv_qkv_attn", "gemv_qkv_attn_pk", "gemv_gu_tp", "gemv_gu_tp_pk")


def _grid_caps(net):
    """One eager generate() with gu_grid_cap = 512 and qkv_attn_grid_cap = 768 -> [(wrapper, is the unfused gate|up launch, grid_cap it was given)]."""
    cfg, model, feats, ids = net
    calls, orig = [], {n: getattr(ops, n) for n in _WRAPPERS}

    def make(n):
        def spy(*a, **k):
            calls.append((n, bool(k.get("mode", 0) & ops.GEMV_OUT_SILU_PAIR), k.get("grid_cap", 0)))
            return orig[n](*a, **k)

        return spy

    for n in _WRAPPERS:
        setattr(ops, n, make(n))
    try:
        with _knobs(model, gu_grid_cap=512, qkv_attn_grid_cap=768, use_hip_graph=False):
            model.generate(ids[:1], image_features=feats[:1], max_new_tokens=N_NEW, eos_token_id=None)
            torch.cuda.synchronize()
            model.check_device_errors()
    finally:
        for n in _WRAPPERS:
            setattr(ops, n, orig[n])
    return calls


def _assert_caps(calls):
    for n, gate_up, cap in calls:
        want = 512 if (gate_up and n in ("gemv", "gemv_pk")) else 768 if n in ("gemv_qkv_attn", "gemv_qkv_attn_pk") else 0
        assert cap == want, (n, gate_up, cap, calls)


def test_grid_caps_reach_the_gate_up_and_the_fused_qkv_launch_only(net, net_mx8):
    packed = _grid_caps(net)
    _assert_caps(packed)
    assert ("gemv_pk", True, 512) in packed and ("gemv_qkv_attn_pk", False, 768) in packed
    with _knobs(net[1], refinalize=True, decode_weight_pack=False):
        plain = _grid_caps(net)
    _assert_caps(plain)
    assert ("gemv", True, 512) in plain and ("gemv_qkv_attn", False, 768) in plain and not any(n.endswith("_pk") for n, _, _ in plain)
    codes = _grid_caps(net_mx8)
    _assert_caps(codes)
    assert ("gemv_mx8", True, 0) in codes and not any(c for _, _, c in codes)  # MXFP8 codes: neither cap reaches any launch
