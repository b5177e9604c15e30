"""The scoring rule of the device scorer (dl_decode_score, csrc/score.hip), written once in plain torch / Python integers.

Same role as sampling.py has for dl_decode_sample: this file is the contract the kernel is tested against; it runs on the CPU (and on
any torch device).  The quantity is the reference's generation-time perplexity driver (llava/dynamic_eval/model_lvis_for_ppl.py:136-191):
forward, take the logits of the last position, record the label, feed the label, repeat, exp(mean cross-entropy).

One step of one row, `reference_step(logits_row, label)`:

1. x_v = float32(logit_v); m = max_v x_v; top1 = the lowest index attaining m (dl_decode_advance's tie rule).
2. w_v = exp(x_v - m), the subtraction and the exponential in fp32.
3. mass_v = floor(w_v * 2^40) as a 64-bit integer (S_BITS of sampling.py; zero, denormal and NaN weights give 0, as sample_mass in
   csrc/fixed_mass.h does).
4. M = sum_v mass_v: an integer sum -- exact, so independent of the order of summation, the same however threads, waves or launch forms
   split the row.  M >= 2^40 (the maximum contributes exactly 2^40) and M < 2^57 for V <= 65536.
5. lse = log(float32(M) * 2^-40): the 64-bit integer converts to fp32 with round-to-nearest-even, the scaling is exact, the logarithm is fp32.
6. d = m - x_label; nll = d + lse: two fp32 operations, in this order.

A logit of -inf has mass 0; a label whose logit is -inf scores +inf.  The row needs one finite maximum: NaN logits are not supported
(as in the greedy argmax), nor is +inf.  V <= 65536 (sampling.MAX_VOCAB).

`IGNORE` (-100) marks "no label": score() accepts it only as the tail of a row, and the kernel treats every label outside [0, V) as
"this row's labels are exhausted" (finished, pad_id fed, nothing written)."""
from __future__ import annotations

import torch

from .sampling import MAX_VOCAB, S_BITS

IGNORE = -100  # config.IGNORE_INDEX


def masses(logits_row):
    """Steps 1-3: (m fp32 scalar, top1 int, mass int64 [V])."""
    assert logits_row.dim() == 1 and 0 < logits_row.shape[0] <= MAX_VOCAB
    x = logits_row.float()
    m = x.max()
    top1 = int(torch.nonzero(x == m)[0])
    w = torch.exp(x - m)  # fp32
    mass = torch.floor(w.double() * float(2**S_BITS))
    mass = torch.where(w == w, mass, torch.zeros_like(mass)).to(torch.int64)  # (a denormal weight is below 2^-86 after the scaling: floor gives 0)
    return m, top1, mass


def lse_of(M):
    """Step 5 for an integer M."""
    return torch.log(torch.tensor(int(M), dtype=torch.int64).to(torch.float32) * torch.tensor(2.0**-S_BITS, dtype=torch.float32))


def reference_step(logits_row, label):
    """One scored step of one row -> (nll fp32 scalar tensor, top1 int, details: m, M, lse, d)."""
    m, top1, mass = masses(logits_row)
    M = int(mass.sum())
    lse = lse_of(M)
    d = m.cpu() - logits_row[int(label)].float().cpu()
    nll = d + lse
    return nll, top1, dict(m=m, M=M, lse=lse, d=d, mass=mass)


def reference_row_labels(logits_row, labels):
    """One row scored against several labels (the masses are summed once) -> (nll fp32 [n], top1 int, lse fp32 scalar)."""
    m, top1, mass = masses(logits_row)
    lse = lse_of(int(mass.sum()))
    d = m.cpu() - logits_row[torch.as_tensor(labels, dtype=torch.int64)].float().cpu()
    return d + lse, top1, lse


def reference_rows(logits, labels):
    """A batch [B, V] with int labels [B] -> (nll fp32 [B] with 0 where there is no label, top1 int64 [B] with -1 there)."""
    B = logits.shape[0]
    nll, top1 = torch.zeros(B, dtype=torch.float32), torch.full((B,), -1, dtype=torch.int64)
    for b in range(B):
        lab = int(labels[b])
        if 0 <= lab < logits.shape[1]:
            n, t, _ = reference_step(logits[b], lab)
            nll[b], top1[b] = n, t
    return nll, top1


def validate_labels(labels, batch, vocab_size):
    """score()'s label check, before any launch: int64 [B, T], T >= 1, B == batch; every entry in [0, V) or IGNORE; IGNORE only as the tail of
    a row, never in column 0.  -> n_labels int64 [B] (CPU)."""
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.dtype != torch.int64:
        raise ValueError("labels must be an int64 tensor [B, T]")
    if labels.shape[0] != int(batch):
        raise ValueError(f"{labels.shape[0]} rows of labels for {int(batch)} rows of input_ids")
    if labels.shape[1] < 1:
        raise ValueError("labels needs at least one column")
    lab = labels.detach().cpu()
    real = lab != IGNORE
    if bool(((lab < 0) | (lab >= int(vocab_size)))[real].any()):
        raise ValueError(f"labels must lie in [0, {int(vocab_size)}) or be {IGNORE} (no label)")
    if not bool(real[:, 0].all()):
        raise ValueError(f"column 0 of labels must hold a label in every row ({IGNORE} is allowed only as the tail of a row)")
    if bool((real[:, 1:] & ~real[:, :-1]).any()):
        raise ValueError(f"{IGNORE} is allowed only as the tail of a row of labels (a label follows a hole)")
    return real.sum(dim=1)
