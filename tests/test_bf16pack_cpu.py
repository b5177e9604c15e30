"""CPU: the 12-bit lossless bf16 packing rule (dynamic_llava_amd/bf16pack.py) -- unpack(pack(w)) is w bit for bit, and the packed size is a condition."""
import pytest
import torch

from dynamic_llava_amd import bf16pack as bp


def _bits(w):
    return w.view(torch.int16)


def _roundtrip(w, force=False):
    p = bp.pack(w, force=force)
    assert p is not None
    assert p.data.numel() == w.shape[0] * w.shape[1] * 3 // 2 and p.hdr.shape == (w.shape[0], 2) and p.pool.numel() == max(p.n_pool, 1) * 1024
    assert 0 <= p.hb <= 120
    assert torch.equal(_bits(bp.unpack(p)), _bits(w))
    return p


def _normal(N, K, seed=0, std=0.02):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * std).to(torch.bfloat16)


def test_every_bf16_bit_pattern_round_trips():
    """All 65536 words (NaN payloads, Inf, +-0, subnormals) as 16 rows of an otherwise ordinary matrix, and the same 16 rows alone."""
    allw = torch.arange(65536, dtype=torch.int32)
    allw = torch.where(allw >= 32768, allw - 65536, allw).to(torch.int16).view(16, 4096)
    w = _normal(256, 4096, seed=1)
    _bits(w)[100:116] = allw
    p = _roundtrip(w)
    assert torch.equal(_bits(bp.unpack(p))[100:116], allw)
    _roundtrip(allw.view(torch.bfloat16).clone(), force=True)


@pytest.mark.parametrize("K", [4096, 11008])
def test_normal_weights_round_trip_and_size(K):
    w = _normal(256, K, seed=K)
    p = _roundtrip(w)
    ratio = bp.packed_nbytes(p) / bp.raw_nbytes(p)
    print(f"N(0, 0.02) [256, {K}]: hb {p.hb}, {p.n_pool} pool spans, packed / raw = {ratio:.4f}")
    assert ratio <= 0.80


def test_rows_of_zeros_and_rows_of_escapes():
    w = _normal(64, 4096, seed=3)
    w[5] = 0.0
    w[6] = -0.0
    w[7] = 3.0e4  # far above the window
    w[8] = 1.0e-30
    w[63] = float("inf")
    p = _roundtrip(w)
    hdr = p.hdr.to(torch.int64)
    assert all(int(hdr[r, 0]) & 0xFF == 0xFF for r in (5, 6, 7, 8, 63))  # every span of these rows is in the pool
    _roundtrip(torch.zeros(8, 4096, dtype=torch.bfloat16), force=True)


@pytest.mark.parametrize("K", [4096, 5120, 11008, 13824, 64, 8256, 16384])
def test_escapes_at_the_row_ends_and_in_the_ragged_tail(K):
    w = _normal(40, K, seed=K + 1)
    w[0, 0] = 0.0  # first chunk of the first row
    w[0, K - 1] = 1.0e4  # last chunk
    w[3, 7] = 1.0e-20
    w[39, K - 8] = -0.0  # last chunk of the last row
    w[39, 0] = 65504.0
    w[17, K - 1] = float("nan")
    if K % 512:
        w[20, K - (K % 512) + 1] = 0.0  # in the ragged last span
    w[21, K // 2] = 0.0
    p = _roundtrip(w, force=True)
    nspan = (K + 511) // 512
    hdr = p.hdr.to(torch.int64) & 0xFFFFFFFF
    assert int(hdr[0, 0]) & 1 and int(hdr[0, 0]) >> (nspan - 1) & 1 and int(hdr[39, 0]) >> (nspan - 1) & 1
    # the pool spans of a row follow each other, rows in order
    cnt = torch.tensor([bin(int(m)).count("1") for m in hdr[:, 0]])
    assert torch.equal(p.hdr[:, 1].to(torch.int64), cnt.cumsum(0) - cnt) and int(cnt.sum()) == p.n_pool


def test_a_matrix_with_an_escape_in_every_span_is_not_packed():
    w = _normal(32, 4096, seed=9)
    w[:, ::512] = 0.0
    assert bp.pack(w) is None
    assert bp.pack(_normal(8, 4096 + 8)) is None  # K is not a multiple of 64
    assert bp.pack(_normal(8, 4096).float()) is None  # not bf16
    _roundtrip(w, force=True)


def test_window_choice_follows_the_weights():
    for std in (0.02, 1.0, 1e-4):
        w = _normal(64, 4096, seed=11, std=std)
        p = _roundtrip(w)
        e = (_bits(w).to(torch.int32) >> 8) & 0x7F
        cover = [int(((e >= hb) & (e <= hb + 7)).sum()) for hb in range(121)]
        assert cover[p.hb] == max(cover)


def test_heavy_tailed_weights_ratio_is_reported():
    g = torch.Generator().manual_seed(5)
    t = torch.distributions.StudentT(4.0)
    torch.manual_seed(5)
    w = (t.sample((256, 4096)) * 0.015).to(torch.bfloat16)
    p = bp.pack(w, force=True)
    assert torch.equal(_bits(bp.unpack(p)), _bits(w))
    print(f"Student-t(4) * 0.015 [256, 4096]: packed / raw = {bp.packed_nbytes(p) / bp.raw_nbytes(p):.4f} (reported, not asserted)")
    del g
