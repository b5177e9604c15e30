"""The table of policy-attention launches that tests/test_train_policy_gpu.py asserts on: the forward and the two-pass backward of
csrc/train_policy.hip at every length edge, mask form, layout and backward geometry, on the hard inputs of oracle/train_truth.py, against
the fp64 truth (row maximum held constant: what the kernels specify) under the derived per-element bound.  `ops` is
dynamic_llava_amd.hip_ops and `sdpa` is train_ops.scaled_dot_product_attention_with_policy (passed in: the oracle does not import the product).

Every entry first asserts the backward wave count it was written for (ops.attn_policy_bwd_waves, the query the launch itself calls),
runs twice on the same inputs and requires the same bits (the header promises no atomics), and -- through the C ABI -- runs on padded
rows into sentinel-filled buffers whose slack and guard bands must come back untouched."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from oracle import train_truth as tt

LENGTHS = (1, 15, 17, 63, 64, 65, 127, 128, 129, 200)
MASKS = ("causal", "additive", "bool", "none")
DTYPES = (torch.bfloat16, torch.float16)
GUARD = 4096        # elements behind every output buffer
ROW_SLACK = 8       # elements between two rows of the padded layout (row stride H * d + 8)
SENTINEL = -1234.0  # exact in bf16, f16 and fp32


@dataclass
class Entry:
    B: int
    H: int
    L: int
    d: int
    kind: str              # mask: causal, additive, bool, none, soft, batch1, keypad, leftpad (train_truth.make_bias)
    dist: str
    policy: str
    layout: str = "module"  # module: [B,L,H,d] storage; contig: contiguous [B,H,L,d] q/k/v, output in the module layout; abi: the C ABI on padded rows
    waves: int = 4          # the backward form this entry was written for
    n_eps_mult: int = 1     # n_for_eps = n_eps_mult * L (abi only)

    @property
    def id(self):
        return f"B{self.B}H{self.H}L{self.L}d{self.d}-{self.kind}-{self.dist}-{self.policy}-{self.layout}-w{self.waves}" + (f"-N{self.n_eps_mult}L" if self.n_eps_mult != 1 else "")


def _sweep():
    out, i = [], 0
    for d in (64, 128):
        for L in LENGTHS:
            out.append(Entry(2, 2, L, d, MASKS[i % 4], tt.INPUTS[i % len(tt.INPUTS)], tt.POLICIES[i % len(tt.POLICIES)]))
            i += 1 if L != 200 else 2  # (so that d = 128 pairs each length with another mask, input and policy than d = 64)
    return out


TABLE = _sweep() + [
    Entry(2, 3, 129, 128, "additive", "leak_rows", "pattern"),
    Entry(2, 3, 65, 64, "causal", "leak_rows", "edges"),
    # the 8-wave backward: head_dim 128 and B * H * ceil(L / 128) >= 256 -- its smallest launches, and the 4-wave twin just below
    Entry(2, 64, 130, 128, "causal", "leak_rows", "pattern", waves=8),
    Entry(2, 64, 130, 128, "none", "gauss", "frac", waves=8),
    Entry(1, 86, 257, 128, "additive", "late_peak", "edges", waves=8),  # 86 * 3 = 258 workgroups, the third key workgroup holds one key
    Entry(1, 86, 257, 128, "causal", "sink", "pattern", waves=8),
    Entry(2, 63, 130, 128, "causal", "leak_rows", "pattern", waves=4),
    # layouts
    Entry(2, 2, 129, 64, "causal", "gauss", "pattern", layout="contig"),
    Entry(2, 3, 200, 128, "soft", "late_peak", "frac", layout="contig"),
    Entry(2, 2, 65, 64, "causal", "leak_rows", "pattern", layout="abi"),
    Entry(2, 3, 200, 128, "soft", "v_outlier", "edges", layout="abi"),
    Entry(2, 2, 17, 128, "none", "gauss", "zeros", layout="abi"),
    Entry(2, 2, 150, 64, "causal", "leak_rows", "pattern", layout="abi", n_eps_mult=2),
    Entry(2, 2, 150, 128, "keypad", "leak_rows", "frac", layout="abi", n_eps_mult=2),
    # bias forms: soft values on the causal mask, batch broadcast, row broadcast (key padding), right padding (additive / bool), left padding
    Entry(2, 2, 129, 64, "soft", "gauss", "pattern"),
    Entry(2, 2, 200, 128, "soft", "leak_rows", "ones"),
    Entry(2, 2, 129, 128, "batch1", "late_peak", "pattern"),
    Entry(2, 2, 65, 64, "batch1", "leak_rows", "frac"),
    Entry(2, 2, 129, 64, "keypad", "plateau", "pattern"),
    Entry(2, 2, 200, 128, "keypad", "leak_rows", "edges"),
    Entry(2, 2, 130, 64, "leftpad", "gauss", "pattern"),
    Entry(2, 2, 200, 128, "leftpad", "leak_rows", "frac"),
    Entry(2, 2, 64, 128, "leftpad", "sink", "zeros"),
]


def build_case(e: Entry, dtype, seed=0):
    return tt.make_case(e.dist, e.B, e.H, e.L, e.d, dtype, e.kind, e.policy, seed=seed, n_eps=e.n_eps_mult * e.L if e.n_eps_mult != 1 else 0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _to_device(bias):
    """A mask on the device with the strides it has here (an expanded key-padding mask keeps its row stride 0)."""
    if bias is None:
        return None
    if bias.stride(2) == 0 and bias.shape[2] > 1:
        return bias[:, :, :1].contiguous().cuda().expand(bias.shape)
    return bias.cuda()


def _run_module(sdpa, e: Entry, c: tt.Case, dtype, seed=0):
    """Through the autograd function, as the attention module calls it.  The mask goes in as the test's kind has it (bool masks as bool)."""
    mask = tt.make_bias(e.kind, e.B, e.L, dtype, seed)  # (the case's bias, before a bool mask became -inf)
    mask = _to_device(mask)
    if e.kind == "keypad" and e.L > 1:
        assert mask.stride(2) == 0  # the expanded key-padding mask: the wrapper passes its row stride 0 on
    outs = []
    for _ in range(2):
        q, k, v = ((t.contiguous() if e.layout == "contig" else t).cuda().requires_grad_(True) for t in (c.q, c.k, c.v))
        if e.layout == "contig":
            assert q.is_contiguous()
        else:
            assert q.transpose(1, 2).is_contiguous()
        pol = c.policy.to(dtype)[:, :, None].cuda().requires_grad_(True)
        o = sdpa(q, k, v, attn_mask=mask, is_causal=e.kind == "causal", policy=pol)
        assert o.shape == (e.B, e.H, e.L, e.d) and o.transpose(1, 2).is_contiguous()
        o.backward(c.do.cuda())
        torch.cuda.synchronize()
        outs.append(dict(out=o.detach().cpu(), dq=q.grad.cpu(), dk=k.grad.cpu(), dv=v.grad.cpu(), dpolicy=pol.grad.cpu()[:, :, 0]))
    return outs, True


def _padded(x):
    """[B,H,L,d] -> a flat buffer with row stride H * d + ROW_SLACK and GUARD elements behind it; slack and guard hold NaN (never read)."""
    B, H, L, d = x.shape
    rs = H * d + ROW_SLACK
    flat = torch.full((B * L * rs + GUARD,), float("nan"), dtype=x.dtype)
    flat.as_strided((B, H, L, d), (L * rs, d, rs, 1)).copy_(x)
    return flat


def _run_abi(ops, e: Entry, c: tt.Case, dtype):
    """dl_attn_policy_fwd / _bwd directly: padded rows, every output buffer sentinel-filled with a guard band behind it."""
    B, H, L, d = c.shape
    rs = H * d + ROW_SLACK
    view = lambda flat: flat.as_strided((B, H, L, d), (L * rs, d, rs, 1))
    ins = {n: _padded(getattr(c, n)).cuda() for n in ("q", "k", "v", "do")}
    pol = c.policy.cuda()
    bias = _to_device(c.bias)
    n_ws = ops.attn_policy_workspace(B, H, L, d, "cuda").numel()
    keep = torch.ones(B, H, L, d, dtype=torch.bool)
    mask16 = torch.ones(B * L * rs + GUARD, dtype=torch.bool)
    mask16.as_strided((B, H, L, d), (L * rs, d, rs, 1))[keep] = False  # True: slack or guard
    outs = []
    for _ in range(2):
        buf = {n: torch.full((B * L * rs + GUARD,), SENTINEL, dtype=dtype, device="cuda") for n in ("out", "dq", "dk", "dv")}
        st = {n: torch.full((B * H * L + GUARD,), SENTINEL, dtype=torch.float32, device="cuda") for n in ("row_max", "row_denom", "dpol")}
        ws = torch.full((n_ws + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        stv = {n: x[: B * H * L].view(B, H, L) for n, x in st.items()}
        ops.attn_policy_fwd(view(ins["q"]), view(ins["k"]), view(ins["v"]), view(buf["out"]), pol, bias, stv["row_max"], stv["row_denom"], ws[:n_ws],
                            e.kind == "causal", c.scale, c.eps, c.N)
        ops.attn_policy_bwd(view(ins["q"]), view(ins["k"]), view(ins["v"]), view(buf["out"]), view(ins["do"]), view(buf["dq"]), view(buf["dk"]), view(buf["dv"]),
                            pol, bias, stv["row_max"], stv["row_denom"], stv["dpol"], ws[:n_ws], e.kind == "causal", c.scale, c.eps, c.N)
        torch.cuda.synchronize()
        for n, x in buf.items():
            xc = x.cpu()
            assert bool((xc[mask16] == SENTINEL).all()), f"{e.id}: {n}: the slack between rows or the guard band was written"
        for n, x in list(st.items()) + [("workspace", ws)]:
            assert bool((x.cpu()[-GUARD:] == SENTINEL).all()), f"{e.id}: {n}: the guard band was written"
        got = {n: view(x.cpu()).clone() for n, x in buf.items()}
        got["dpolicy"] = stv["dpol"].cpu().sum(dim=1)  # fp32, as the caller sums it
        outs.append(got)
    return outs, False


def run_entry(ops, sdpa, e: Entry, dtype, seed=0):
    """One table entry: asserts the wave count, bit-equal repetition and (abi) untouched slack and guard bands; returns
    {output: (worst err / tol, that element's error in ULP, its index)}."""
    assert ops.attn_policy_bwd_waves(e.B, e.H, e.L, e.d) == e.waves, f"{e.id}: the backward runs {ops.attn_policy_bwd_waves(e.B, e.H, e.L, e.d)} waves per workgroup"
    c = build_case(e, dtype, seed)
    if e.dist == "leak_rows":
        tt.check_property(c)
    (a, b), rounded = _run_abi(ops, e, c, dtype) if e.layout == "abi" else _run_module(sdpa, e, c, dtype, seed)
    for n in a:
        assert torch.equal(_bits(a[n]), _bits(b[n])), f"{e.id}: {n} differs between two launches on the same inputs"
    return tt.evaluate(c, a, dpolicy_rounded=rounded)
