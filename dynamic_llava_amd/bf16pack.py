"""Lossless 12-bit packing of bf16 weight matrices for the batch-1 decode stream (csrc/gemv_pk.hip).  This file is the DEFINITION of the format:
the kernels are tested against unpack(pack(w)) == w, bit for bit, and against dl_gemv on the same weights.

A bf16 word is s | e[7:0] | m[6:0].  Its low byte L = e[0] | m is stored verbatim; of its high byte H = s | e[7:1] only 4 bits are kept:

    n = s << 3 | ((H & 0x7f) - hb)          when 0 <= (H & 0x7f) - hb <= 7   ("in window": 16 consecutive exponents from the even exponent 2 hb)

with ONE hb (0..120) per matrix, the one that covers the most weights.  Decoding is byte-parallel on four spread nibbles u:
H4 = ((u & 0x07070707) + hb * 0x01010101) | ((u & 0x08080808) << 4).  Everything else -- +-0, subnormals, Inf / NaN, very small and very large
values, unless the window happens to hold them -- is an ESCAPE.

Units.  A *chunk* is 8 consecutive elements of a row (the 16 bytes one lane multiplies at a time), a *span* the 64 chunks v = lane + 64 c that one
wave reads together (512 elements).  A span that holds an escape is ALSO stored raw (1024 bytes of bf16, the ragged last span of a row zero-padded)
in the matrix's pool; the row's header {span mask, index of its first pool span} says which and where, and the pool spans of a row follow each
other in span order.  The packed bytes of such a span are still present (escaped elements carry nibble 0) and are ignored.

Row layout (12 bytes per chunk, K * 3 / 2 bytes per row, no padding).  A row is one *segment* of chunks [0, K/8) when K <= 8192 and two
segments [0, hv), [hv, K/8) with hv = ceil(ceil(K/16) / 64) * 64 when 8192 < K <= 16384 -- the two halves the long-row kernel gives to the two
waves of a pair.  A segment of nc chunks starts at byte 12 * (its first chunk) of the row and holds
  * P = nc // 128 *pairs* of full spans, 1536 bytes each: 64 x 16 bytes of low bytes -- lane l's 16 bytes are the 8 low bytes of chunk l + 128 p
    followed by the 8 of chunk l + 128 p + 64 -- then 64 x 8 bytes of nibbles, 4 bytes per chunk in the same order;
  * the nt = nc - 128 P chunks left, in chunk order: nt x 8 low bytes, then nt x 4 nibble bytes.
The 4 nibble bytes of a chunk are pre-spread: byte j = n[j] | n[j + 4] << 4, so that w & 0x0f0f0f0f and (w >> 4) & 0x0f0f0f0f are the nibbles of
elements 0..3 and 4..7, one per byte.

K must be a multiple of 64 and <= 16384 (<= 32 spans: the mask is 32 bits).  Pure torch; works on CPU and GPU tensors."""
from __future__ import annotations

from dataclasses import dataclass

import torch

SPAN = 512  # elements one wave reads as one 16-byte chunk per lane
SPAN_BYTES = 2 * SPAN
MAX_K = 16384
KEEP_RATIO = 0.9  # a matrix whose packed size is >= this fraction of its bf16 size is not packed


@dataclass
class PackedBf16:
    data: torch.Tensor  # uint8 [N * K * 3 / 2]
    hdr: torch.Tensor  # int32 [N, 2]: span mask (bit s: span s is read from the pool), index of the row's first pool span
    pool: torch.Tensor  # uint8 [max(n_pool, 1) * 1024]
    n_pool: int
    hb: int
    N: int
    K: int

    @property
    def row_bytes(self) -> int:
        return self.K * 3 // 2


def can_pack(K: int) -> bool:
    return K > 0 and K % 64 == 0 and K <= MAX_K


def segments(K: int):
    """[(first chunk, chunk count)] of a row."""
    nvec = K // 8
    if K <= 8192:
        return [(0, nvec)]
    hv = ((nvec + 1) // 2 + 63) // 64 * 64
    return [(0, hv), (hv, nvec - hv)]


_index_cache: dict = {}


def _indices(K: int, device):
    """Byte offsets inside a packed row: lo_idx [K] (element k's low byte), nb_idx [K / 2] (chunk v's nibble byte j at v * 4 + j)."""
    key = (K, str(device))
    if key not in _index_cache:
        lo, nb = [], []
        for v0, nc in segments(K):
            cl = torch.arange(nc, dtype=torch.int64)
            P = nc // 128
            nt = nc - 128 * P
            c, lane = cl // 64, cl % 64
            p, j2 = c // 2, c % 2
            t = cl - 128 * P
            in_pair = cl < 128 * P
            lo_c = torch.where(in_pair, p * 1536 + lane * 16 + j2 * 8, P * 1536 + t * 8) + 12 * v0
            nb_c = torch.where(in_pair, p * 1536 + 1024 + lane * 8 + j2 * 4, P * 1536 + nt * 8 + t * 4) + 12 * v0
            lo.append((lo_c[:, None] + torch.arange(8)[None, :]).reshape(-1))
            nb.append((nb_c[:, None] + torch.arange(4)[None, :]).reshape(-1))
        lo_idx, nb_idx = torch.cat(lo), torch.cat(nb)
        both = torch.cat([lo_idx, nb_idx])
        assert both.numel() == K * 3 // 2 and torch.equal(both.sort().values, torch.arange(K * 3 // 2)), "the row layout must be a permutation"
        _index_cache[key] = (lo_idx.to(device), nb_idx.to(device))
    return _index_cache[key]


def _words(w):
    return w.view(torch.int16).to(torch.int32) & 0xFFFF


def choose_hb(w) -> int:
    """The window start that covers the most weights (the lowest one among equals)."""
    hist = torch.zeros(128, dtype=torch.int64, device=w.device)
    for r0 in range(0, w.shape[0], 4096):
        hist += torch.bincount(((_words(w[r0:r0 + 4096]) >> 8) & 0x7F).reshape(-1), minlength=128)
    cover = hist.cumsum(0)
    cover = torch.cat([cover[7:8], cover[8:] - cover[:-8]])  # windows hb = 0..120
    return int(cover.argmax().item())


def pack(w, force: bool = False):
    """w: bf16 [N, K] -> PackedBf16, or None when the matrix cannot be packed (shape) or would not be smaller than KEEP_RATIO of its bf16 size
    (force=True packs it all the same)."""
    assert w.dim() == 2
    N, K = w.shape
    if w.dtype != torch.bfloat16 or N == 0 or not can_pack(K):
        return None
    w = w.detach().contiguous()
    dev = w.device
    hb = choose_hb(w)
    nspan = (K + SPAN - 1) // SPAN
    lo_idx, nb_idx = _indices(K, dev)
    row_bytes = K * 3 // 2
    data = torch.empty((N, row_bytes), dtype=torch.uint8, device=dev)
    mask = torch.empty(N, dtype=torch.int64, device=dev)
    pools = []
    shifts = torch.arange(nspan, dtype=torch.int64, device=dev)
    for r0 in range(0, N, 4096):
        x = _words(w[r0:r0 + 4096])
        n = x.shape[0]
        d = ((x >> 8) & 0x7F) - hb
        inwin = (d >= 0) & (d <= 7)
        nib = torch.where(inwin, ((x >> 15) << 3) | d, torch.zeros_like(d)).view(n, K // 8, 8)
        blk = torch.empty((n, row_bytes), dtype=torch.uint8, device=dev)
        blk[:, lo_idx] = (x & 0xFF).to(torch.uint8)
        blk[:, nb_idx] = (nib[..., :4] | (nib[..., 4:] << 4)).to(torch.uint8).view(n, K // 2)
        data[r0:r0 + n] = blk
        esc = ~inwin
        raw = w[r0:r0 + n].view(torch.int16)
        if K % SPAN:
            esc = torch.nn.functional.pad(esc, (0, nspan * SPAN - K))
            raw = torch.nn.functional.pad(raw, (0, nspan * SPAN - K))
        flagged = esc.view(n, nspan, SPAN).any(-1)
        mask[r0:r0 + n] = (flagged.to(torch.int64) << shifts).sum(-1)
        pools.append(raw.reshape(n, nspan, SPAN)[flagged])  # row-major: by row, then by span
    pool16 = torch.cat(pools)
    n_pool = int(pool16.shape[0])
    per_row = torch.zeros(N, dtype=torch.int64, device=dev)
    for s in range(nspan):
        per_row += (mask >> s) & 1
    off = per_row.cumsum(0) - per_row
    assert n_pool == int(per_row.sum().item()) and n_pool < 2**31
    hdr = torch.stack([torch.where(mask >= 2**31, mask - 2**32, mask), off], dim=1).to(torch.int32).contiguous()
    pool = torch.zeros(max(n_pool, 1) * SPAN_BYTES, dtype=torch.uint8, device=dev)
    if n_pool:
        pool[: n_pool * SPAN_BYTES] = pool16.contiguous().view(torch.uint8).reshape(-1)
    p = PackedBf16(data.reshape(-1), hdr, pool, n_pool, hb, N, K)
    if not force and packed_nbytes(p) >= KEEP_RATIO * raw_nbytes(p):
        return None
    return p


def raw_nbytes(p: PackedBf16) -> int:
    return 2 * p.N * p.K


def packed_nbytes(p: PackedBf16) -> int:
    """Bytes the packed copy occupies: rows + headers + pool."""
    return p.data.numel() + p.hdr.numel() * 4 + p.pool.numel()


def unpack(p: PackedBf16):
    """-> bf16 [N, K], the exact words that were packed."""
    N, K, dev = p.N, p.K, p.data.device
    nspan = (K + SPAN - 1) // SPAN
    lo_idx, nb_idx = _indices(K, dev)
    data = p.data.view(N, p.row_bytes)
    out = torch.empty((N, K), dtype=torch.int16, device=dev)
    pool16 = p.pool.view(torch.int16).view(-1, SPAN)
    shifts = torch.arange(nspan, dtype=torch.int64, device=dev)
    for r0 in range(0, N, 4096):
        blk = data[r0:r0 + 4096]
        n = blk.shape[0]
        lo = blk[:, lo_idx].to(torch.int32)
        nb = blk[:, nb_idx].to(torch.int32).view(n, K // 8, 4)
        nib = torch.cat([nb & 0xF, nb >> 4], dim=-1).view(n, K)
        hi = ((nib & 7) + p.hb) | ((nib & 8) << 4)
        x = (hi << 8) | lo
        x = torch.where(x >= 32768, x - 65536, x).to(torch.int16)
        h = p.hdr[r0:r0 + n].to(torch.int64)
        flagged = (((h[:, 0:1] & 0xFFFFFFFF) >> shifts) & 1).bool()  # [n, nspan]
        if bool(flagged.any()):
            idx = h[:, 1:2] + flagged.to(torch.int64).cumsum(-1) - 1  # pool span of (row, span) where flagged
            if K % SPAN:
                x = torch.nn.functional.pad(x, (0, nspan * SPAN - K))
            x = x.reshape(n, nspan, SPAN).clone()
            x[flagged] = pool16[idx[flagged]]
            x = x.reshape(n, nspan * SPAN)[:, :K]
        out[r0:r0 + n] = x
    return out.view(torch.bfloat16)
