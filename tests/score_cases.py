"""Shared by the scoring tests (not a test module): the logit-row families, their labels, and the error bounds with their derivations."""
import math

import torch

VOCABS = [320, 32000, 32003, 50000, 65536]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def ulp32(y):
    """The fp32 ulp of y: 2^(floor(log2 |y|) - 23) (the smallest normal's binade for anything below it); 0 for 0, inf and NaN."""
    y = abs(float(y))
    if y == 0.0 or math.isinf(y) or math.isnan(y):
        return 0.0
    return 2.0 ** (max(math.floor(math.log2(y)), -126) - 23)


def ulp32_up(y):
    """An upper bound of the fp32 ulp of every number within a factor of two of |y| (a computed value may sit in the binade above its float64 reference)."""
    return 2.0 * ulp32(y)


def families(V, dtype, seed=0):
    """-> [(name, row [V] in dtype)].  Every row has a finite maximum (the rule's precondition)."""
    g = torch.Generator().manual_seed(1000 * seed + V)
    out = []
    for sigma in (1.0, 6.0, 30.0):
        out.append((f"gauss{int(sigma)}", (torch.randn(V, generator=g) * sigma).to(dtype)))
    dom = torch.randn(V, generator=g)
    dom[int(torch.randint(V, (1,), generator=g))] = 120.0  # exceeds every other entry by more than 88: their fp32 weights underflow to 0
    out.append(("dominant", dom.to(dtype)))
    out.append(("equal", torch.full((V,), 1.75).to(dtype)))
    # a shifted row: fp32 holds 1e4 + noise (spacing 2^-10), fp16 holds 6e4 + noise on its 32-wide grid (thousands of ties).  bf16's grid at 6e4 is 256 wide: nothing
    # of a unit-variance row survives the rounding, so that dtype has no shifted family
    if dtype == torch.float32:
        out += [("shift+", (torch.randn(V, generator=g) + 1e4).to(dtype)), ("shift-", (torch.randn(V, generator=g) - 1e4).to(dtype))]
    elif dtype == torch.float16:
        out += [("shift+", (torch.randn(V, generator=g) * 40 + 6e4).clamp(max=65504.0).to(dtype)), ("shift-", (torch.randn(V, generator=g) * 40 - 6e4).clamp(min=-65504.0).to(dtype))]
    ninf = (torch.randn(V, generator=g) * 3).to(dtype)
    ninf[torch.randperm(V, generator=g)[: V // 3]] = float("-inf")
    out.append(("neginf", ninf))
    return out


def labels_for(row, seed=0):
    """argmax, minimum, index 0, index V - 1, random."""
    V = row.shape[0]
    g = torch.Generator().manual_seed(seed + V)
    return [int(row.float().argmax()), int(row.float().argmin()), 0, V - 1, int(torch.randint(V, (1,), generator=g))]


def truth64(row, label):
    """-log_softmax in float64 -> (nll, lse relative to the maximum, d = max - x_label)."""
    x = row.double()
    m = x.max()
    lse = float(torch.log(torch.exp(x - m).sum()))
    d = float(m - x[label])
    return float(-torch.log_softmax(x, dim=0)[label]), lse, d


def rule_bound(V, lse, d):
    """|rule - float64 truth| for one element, term by term (lse, d: the float64 values):
      * d = m - x_label is one fp32 operation: at most one ulp of d;
      * every weight: the fp32 subtraction x - m is off by at most 2^-24 |x - m|, and only terms with |x - m| < 28 have a non-zero mass (e^-28 * 2^40 < 1), so
        the exponent is off by at most 28 * 2^-24; exp itself by one ulp (2^-23 relative; the HIP math API's expf and torch's CPU exp alike); together a relative
        error of the sum of at most e_w = 28 * 2^-24 + 2^-23;
      * floor() loses less than one unit of 2^-40 per token, V * 2^-40 relative to M * 2^-40 >= 1;
      * the 64-bit integer rounds to fp32: 2^-24 relative;
      * log of (1 + e) S is off by at most e / (1 - e) <= e (1 + 2^-16) for the e <= 4e-6 above (second-order terms included);
      * log itself: one ulp of lse; the final addition: one ulp of nll (ulps taken in the binade above the float64 value's: ulp32_up)."""
    e = (28 * 2.0**-24 + 2.0**-23) + V * 2.0**-40 + 2.0**-24
    return ulp32_up(d) + e * (1 + 2.0**-16) + ulp32_up(lse) + ulp32_up(d + lse)


def device_tol(V, lse_ref, nll_ref):
    """|kernel - host rule| on the same logits: m, top1, x_label and the subtractions are exact in both, so the difference comes only from the two exponentials
    (one ulp each: 2 * 2^-23 relative on the sum), a floor unit per token (V * 2^-40), the fp32 rounding of M when the two sums land on different sides of a
    rounding boundary (2^-23), the two logarithms (one ulp of lse each) and the rounding of the final sum (one ulp of nll):
        tol = (2 * 2^-23 + V * 2^-40 + 2^-23) + 2 ulp32(lse_ref) + ulp32(nll_ref)."""
    return (2 * 2.0**-23 + V * 2.0**-40 + 2.0**-23) + 2 * ulp32(lse_ref) + ulp32(nll_ref)
