"""The sampling rule of the device sampler (dl_decode_sample, csrc/sample.hip), written once in plain torch / Python integers.

Same role as mxfp8.py has for the weight format: this file is the contract the kernel is tested against; it runs on the CPU (and on
any torch device) and is also what generate(output_scores=True) uses to report a sampled step's processed logits.

One step of one row, `reference_step(logits_row, temperature, top_k, top_p, banned_ids, seed, row, step)`:

1. z = float32(logit) / float32(T), a correctly rounded division (TemperatureLogitsWarper), T > 0.  Banned ids (the EOS set while
   step < min_new_tokens) become -inf.
2. top-k (top_k >= 1): keep z >= (k-th largest z); ties at the threshold are all kept (TopKLogitsWarper's `z < kth` rule, exact).
3. weights: w = exp(z - zmax) in fp32, then a fixed-point mass m = floor(w * 2^S) as a 64-bit integer, S = 40 (V * 2^40 < 2^63 for
   every V <= 65536).  From here on every sum is an integer sum: exact, independent of the order of summation, the same in every run.
4. top-p (top_p < 1): with M = sum(m) over the survivors of top-k and thr = floor(float64(1 - float32(top_p)) * float64(M)), token v is
   kept iff S(z_v) > thr, where S(x) is the mass of all surviving tokens with z <= x (the whole tie class of x included).  The maximum
   is always kept.  On logits without ties this is exactly HF's TopPLogitsWarper.  With ties (16-bit logits have thousands) HF's
   result depends on the order torch.sort leaves tied tokens in; the rule here keeps a tie class whole: a superset of HF's set by
   less than one tie class, independent of any sort order.
5. draw: Philox4x32-10, key = (seed low 32 bits, seed high 32 bits), counter = (step, row_base + row, 0, 0); r64 = out[1] << 32 | out[0];
   with K = sum(m) over the kept set, t = (r64 * K) >> 64; the token is the kept token with the smallest vocabulary index whose inclusive
   prefix sum of m, taken in index order, exceeds t.

A token is in the kept set when it survives steps 1, 2 and 4 (a banned token never does).  top_p travels to the device as an fp32
number, so the rule rounds it to fp32 first; (1 - top_p) and its product with M are single IEEE double operations, which the kernel
repeats literally.  A logit that is -inf in the input is treated like a banned one: out of the kept set.
NaN logits are not supported (as in the greedy argmax)."""
from __future__ import annotations

import math

import torch

S_BITS = 40  # fixed-point fraction bits of a token's mass
MAX_VOCAB = 65536  # V * 2^S_BITS must stay below 2^63
MAX_EOS_IDS = 3  # the device compares three ids

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 generator):
    counter = four 32-bit words, key = two; returns four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & _U32 for c in counter)
    k0, k1 = (int(k) & _U32 for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _U32, p1 & _U32, ((p0 >> 32) ^ c3 ^ k1) & _U32, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return (c0, c1, c2, c3)


def draw_r64(seed, row, step, row_base=0):
    """The 64 random bits of (seed, row_base + row, step)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = philox4x32_10((int(step), int(row_base) + int(row), 0, 0), (seed & _U32, seed >> 32))
    return (out[1] << 32) | out[0]


def normalize_params(temperature=None, top_k=None, top_p=None):
    """generate()'s kwargs -> (temperature > 0, top_k >= 0, top_p or None).  0 / None mean "off" as in _generate_sample (temperature 1.0,
    no top-k, no top-p); a negative or non-finite temperature, top_p <= 0 and top_k < 0 raise ValueError."""
    t = 1.0 if temperature is None else float(temperature)
    if not math.isfinite(t) or t < 0.0:
        raise ValueError(f"temperature must be a finite number >= 0 (got {temperature!r})")
    if t == 0.0:
        t = 1.0
    k = 0 if top_k is None else int(top_k)
    if k < 0:
        raise ValueError(f"top_k must be >= 0 (got {top_k!r})")
    p = None
    if top_p is not None:
        p = float(top_p)
        if not p > 0.0:  # (also NaN)
            raise ValueError(f"top_p must be > 0 (got {top_p!r})")
        if p >= 1.0:
            p = None
    return t, k, p


def eos_ids(kwargs, default):
    """The only resolver of eos_token_id (request.py re-exports it): the ids as given (order, repeats), () for none.  `default` (the config's) stands in when the call names none; None means none."""
    eos = kwargs.get("eos_token_id", default)
    eos = eos if isinstance(eos, (list, tuple)) else (() if eos is None else (eos,))
    return tuple(int(e) for e in eos)


def device_route(kwargs, vocab_size, default_eos=None):
    """True when generate(**kwargs) samples on the device: do_sample=True with an integer `seed`, torch's RNG not asked for (`generator=`),
    a fresh cache, an EOS set the device can compare and a vocabulary the kernel takes.  Everything else keeps the route it had.
    default_eos: the model config's eos_token_id, which generate() falls back to when the call names none (eos_token_id=None means no EOS)."""
    if not kwargs.get("do_sample", False) or kwargs.get("seed") is None or kwargs.get("generator") is not None:
        return False
    if kwargs.get("past_key_values") is not None or int(vocab_size) > MAX_VOCAB:
        return False
    return len(eos_ids(kwargs, default_eos)) <= MAX_EOS_IDS


def masses(z, alive):
    """m = floor(exp(z - zmax) * 2^S) over the `alive` tokens (int64; 0 elsewhere)."""
    zmax = z[alive].max() if bool(alive.any()) else z.new_tensor(float("-inf"))
    if not bool(torch.isfinite(zmax)):
        return torch.zeros_like(z, dtype=torch.int64), zmax
    w = torch.exp(z - zmax)  # fp32
    m = torch.floor(w.double() * float(2 ** S_BITS)).to(torch.int64)
    return torch.where(alive, m, torch.zeros_like(m)), zmax


def class_mass_below(z, m, alive):
    """S(z_v) for every token: the mass of the alive tokens with z <= z_v (0 for tokens that are not alive)."""
    zs = torch.where(alive, z, z.new_tensor(float("-inf")))
    sz, si = torch.sort(zs)
    cm = torch.cumsum(m[si], dim=0)
    last = torch.searchsorted(sz, sz, right=True) - 1  # last member of every tie class
    s = torch.empty_like(cm)
    s[si] = cm[last]
    return torch.where(alive, s, torch.zeros_like(s))


def top_p_threshold(top_p, M):
    return int(math.floor((1.0 - float(torch.tensor(float(top_p), dtype=torch.float32))) * float(int(M))))


def warp_row(logits_row, temperature, top_k, top_p, banned_ids=()):
    """Steps 1-4 for one row: (z fp32 [V], kept bool [V], details)."""
    assert logits_row.dim() == 1 and temperature > 0
    V = logits_row.shape[0]
    z = logits_row.float() / torch.tensor(float(temperature), dtype=torch.float32, device=logits_row.device)
    banned = [int(i) for i in banned_ids if 0 <= int(i) < V]
    if banned:
        z[banned] = float("-inf")
    alive = z > float("-inf")
    kth = None
    if top_k and int(top_k) >= 1:
        kth = torch.topk(z, min(int(top_k), V)).values[-1]
        alive = alive & (z >= kth)
    m, zmax = masses(z, alive)
    M = int(m.sum())
    det = dict(z=z, m=m, zmax=zmax, M=M, kth=kth, topk_mask=alive.clone(), thr=None, S=None)
    if top_p is not None and float(top_p) < 1.0:
        thr = top_p_threshold(top_p, M)
        S = class_mass_below(z, m, alive)
        alive = alive & (S > thr)
        det.update(thr=thr, S=S)
    return z, alive, det


def reference_step(logits_row, temperature, top_k, top_p, banned_ids, seed, row, step, row_base=0):
    """One sampled step of one row -> (token, kept_mask, details).  details: z, m (int64 masses of the top-k survivors), M, thr, S (top-p
    only), topk_mask, K, r64, t, prefix (inclusive prefix sums of the kept masses in index order)."""
    z, kept, det = warp_row(logits_row, temperature, top_k, top_p, banned_ids)
    mk = torch.where(kept, det["m"], torch.zeros_like(det["m"]))
    prefix = torch.cumsum(mk, dim=0)
    K = int(prefix[-1])
    r64 = draw_r64(seed, row, step, row_base)
    t = (r64 * K) >> 64
    token = int(torch.searchsorted(prefix, torch.tensor(t, dtype=torch.int64, device=prefix.device), right=True)) if K > 0 else 0
    det.update(K=K, r64=r64, t=t, prefix=prefix)
    return token, kept, det


def processed_logits(logits, temperature, top_k, top_p, banned_ids=()):
    """HF `scores` of a sampled step for a batch [B, V]: z with -inf outside the kept set."""
    rows = []
    for b in range(logits.shape[0]):
        z, kept, _ = warp_row(logits[b], temperature, top_k, top_p, banned_ids)
        rows.append(z.masked_fill(~kept, float("-inf")))
    return torch.stack(rows)
