"""Classifier-free guidance on paired rows (dl_logits_guide, csrc/guide.hip), written once in plain torch / Python.

Same role as logprobs.py and constraints.py have for their kernels: this file is the contract the kernel is tested against; it runs on the CPU.  The quantity
is HF's UnbatchedClassifierFreeGuidanceLogitsProcessor -- log_softmax of the conditional and of the negative ("unconditional") step logits, then
scale * (cond - uncond) + uncond -- which is also the formula of visual contrastive decoding (Leng et al., CVPR 2024: the step's logits with the image against
the logits without it, or with a degraded one) together with that paper's adaptive plausibility cutoff.  It is the FIRST logits processor, as in HF's
_get_logits_processor: repetition penalty, n-gram and bad-word bans, the constraint, the EOS ban of min_new_tokens, temperature, top-k and top-p act on its
result.

One step of one pair, `guide_row(c, u, scale, cutoff)`: c are the conditional row's raw logits, u the negative row's.

1. lc(v) = logprob_c(v) and lu(v) = logprob_u(v) for every v: exactly logprobs.py step 2, -((m - x_v) + lse) with scoring.masses / scoring.lse_of.  The guided
   score is therefore built from the same bits `output_logprobs` reports.
2. g(v) = s * (lc - lu) + lu: three fp32 operations in this order, each rounded (no fused multiply-add); s is the scale rounded to fp32.  An entry that is
   -inf in either row is -inf in g (the model's own rows are finite).
3. With a cutoff beta in (0, 1): v is kept only if lc(v) >= (-lse_c) + log_beta, one fp32 addition, where log_beta = math.log(beta) rounded to fp32 on the
   host (`log_beta`); every other entry is -inf.  -lse_c is the conditional argmax's log-probability (-((m - m) + lse)), so that entry is always kept.
4. g is the score of BOTH rows of the pair.

Either row needs one finite maximum (no NaN, no +inf), V <= 65536 (sampling.MAX_VOCAB)."""
from __future__ import annotations

import math
import struct

import torch

from .scoring import lse_of, masses

KEYWORDS = ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask", "negative_images", "guidance_cutoff")


def log_beta(beta) -> float:
    """math.log(beta) rounded to fp32 (as a Python float): the one value host rule and device kernel add."""
    return struct.unpack("<f", struct.pack("<f", math.log(float(beta))))[0]


def row_logprobs(row):
    """Step 1 for one row -> (logprob fp32 [V], lse fp32 scalar tensor), on the CPU."""
    x = row.detach().float().cpu()
    m, _, mass = masses(x)
    lse = lse_of(int(mass.sum()))
    return -((m - x) + lse), lse


def guide_row(c, u, scale, cutoff=None, lse=None):
    """One step of one pair -> g fp32 [V] on the CPU.  lse: (lse_c, lse_u) fp32 scalars taken from elsewhere in the place of step 1's own (the values
    dl_decode_logprobs reports on the device: its exponentials and logarithm are the device's), everything else as written above."""
    xc, xu = c.detach().float().cpu(), u.detach().float().cpu()
    if lse is None:
        lc, lse_c = row_logprobs(xc)
        lu, _ = row_logprobs(xu)
    else:
        lse_c, lse_u = (torch.as_tensor(v, dtype=torch.float32).reshape(()) for v in lse)
        lc, lu = -((xc.max() - xc) + lse_c), -((xu.max() - xu) + lse_u)
    s = torch.tensor(float(scale), dtype=torch.float32)
    g = s * (lc - lu) + lu  # three rounded fp32 operations
    ninf = torch.full_like(g, float("-inf"))
    g = torch.where(torch.isneginf(xc) | torch.isneginf(xu), ninf, g)
    if cutoff is not None:
        thr = (-lse_c) + torch.tensor(log_beta(cutoff), dtype=torch.float32)
        g = torch.where(lc >= thr, g, ninf)
    return g


def apply(cond, uncond, scale, cutoff=None):
    """A batch of pairs: cond [B, V] and uncond [B, V] raw logits -> the guided scores fp32 [B, V], on cond's device."""
    assert cond.dim() == 2 and cond.shape == uncond.shape
    return torch.stack([guide_row(cond[b], uncond[b], scale, cutoff) for b in range(cond.shape[0])]).to(cond.device)


def error_bound(scale, lc, lu):
    """Per-element bound of |g - g_exact| for the rule evaluated in fp32 against exact arithmetic on the same logits, given the (approximately) exact
    log-probabilities lc, lu (float64 tensors).  With u = 2^-24 (half an ulp, relative): each of logprobs.py's two operations and each of step 2's three rounds
    once.  lse itself, 0 <= lse <= log(65536) < 12, is within E_LSE = 34 u absolute: logf within one ulp of a value below 16 (16 u), expf within two ulps of
    every weight (4 u relative to the sum), the floors of the masses (V * 2^-40 <= u), the conversion of M to fp32 (u), and the rounded exponents m - x_v, whose
    relative errors u * (m - x_v) enter the sum weighted by the softmax: u * (H(p) - lse) <= 12 u.
        e(l) = u * |m - x| + u * |l| + E_LSE <= 2 u |l| + 12 u + E_LSE      (either log-probability; |m - x| <= |l| + lse)
        e(g) = s * (e(lc) + e(lu) + u * |lc - lu|) + u * s * |lc - lu| + e(lu) + u * |g|
    DESIGN.md section 4p derives it."""
    u, e_lse = 2.0**-24, 34 * 2.0**-24
    s = float(scale)
    e = lambda l: 2 * u * l.abs() + 12 * u + e_lse  # |m - x| <= |l| + |lse|, |lse| < 12
    d = (lc - lu).abs()
    g = s * (lc - lu) + lu
    return s * (e(lc) + e(lu) + u * d) + u * s * d + e(lu) + u * g.abs()


def validate(kwargs):
    """generate()'s check of the guidance keywords, before any launch -> None (no guidance: no keyword, or guidance_scale None / 1.0 with nothing else that
    needs it) or (scale float, cutoff float | None)."""
    s = kwargs.get("guidance_scale")
    beta = kwargs.get("guidance_cutoff")
    has_neg = kwargs.get("negative_prompt_ids") is not None or kwargs.get("negative_images") is not None
    if kwargs.get("_score_labels") is not None and any(kwargs.get(k) is not None for k in KEYWORDS):
        raise ValueError(f"score() takes no guidance ({', '.join(k for k in KEYWORDS if kwargs.get(k) is not None)}): a label is scored on the model's own logits")
    if s is not None:
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(float(s)) or float(s) < 0:
            raise ValueError(f"guidance_scale must be a finite float >= 0 (got {s!r})")
    active = s is not None and float(s) != 1.0
    if beta is not None:
        if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 < float(beta) < 1.0:
            raise ValueError(f"guidance_cutoff must lie in (0, 1) (got {beta!r})")
        if not active:
            raise ValueError("guidance_cutoff needs an active guidance_scale (not None, not 1.0)")
    if kwargs.get("negative_prompt_attention_mask") is not None and kwargs.get("negative_prompt_ids") is None:
        raise ValueError("negative_prompt_attention_mask belongs to negative_prompt_ids, which is missing")
    if not active:
        return None
    if not has_neg:
        raise ValueError("guidance_scale needs negative_prompt_ids= or negative_images=: HF's default negative prompt (the prompt's last token alone) has no "
                         "meaning next to an image placeholder")
    n = kwargs.get("num_return_sequences")
    if n is not None and n != 1:
        raise NotImplementedError("guidance_scale with num_return_sequences > 1 is not built: the pair layout and the fork both widen the decode batch")
    if kwargs.get("past_key_values") is not None:
        raise NotImplementedError("guidance_scale with past_key_values is not built: the negative prompt has no cache of earlier turns")
    neg = kwargs.get("negative_prompt_ids")
    if neg is not None and not (torch.is_tensor(neg) and neg.dim() == 2 and neg.dtype == torch.int64 and neg.shape[1] >= 1):
        raise ValueError("negative_prompt_ids must be an int64 tensor [B, Wn] or [1, Wn]")
    return float(s), None if beta is None else float(beta)


def negative_inputs(kwargs, inputs, images, image_token):
    """The negative rows of a guided request -> (ids int64 [B, Wn], attention mask or None, images of the rows that hold a placeholder or None, pre-computed image
    features or None).  negative_prompt_ids [1, Wn] is broadcast over the prompts; without it the negative ids are the inputs (same text, another image: VCD's
    form).  negative_images defaults to the request's images (or its image_features); a negative prompt without the placeholder is text-only and takes none."""
    B = inputs.shape[0]
    neg, mask = kwargs.get("negative_prompt_ids"), kwargs.get("negative_prompt_attention_mask")
    if neg is None:
        neg, mask = inputs, kwargs.get("attention_mask")
    if neg.shape[0] not in (1, B):
        raise ValueError(f"negative_prompt_ids has {neg.shape[0]} rows for {B} prompts (1 or {B})")
    if neg.shape[0] != B:
        neg = neg.expand(B, -1).contiguous()
        mask = mask if mask is None else mask.expand(B, -1).contiguous()
    has_image = bool((neg == image_token).any())
    n_images = kwargs.get("negative_images")
    if not has_image:
        return neg, mask, None, None
    if n_images is not None:
        return neg, mask, n_images, None
    return neg, mask, images, kwargs.get("image_features")
