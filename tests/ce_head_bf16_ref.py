"""fp64 reference, per-element error bounds and a CPU emulation in the kernels' own order for the masked-token loss head
under bf16 autocast, csrc/ce_head_bf16.hip (amk_ce_head_bf16_fwd / _bwd, ops.linear_cross_entropy inside
torch.autocast("cuda", bfloat16)).  Targets, input families, the host's slicing and the measures come from
tests/ce_head_ref.py; the inputs are that module's, rounded to bf16.

The reference is fp64 on the bf16 values the kernels read.  u = 2^-24 (f32), U16 = 2^-8 (the project's bf16 unit: a bf16
rounding is charged 2 U16 |value|, tests/bf16_dense_ref.py).  No bound is relative to a tensor's maximum.  Semantics as
tests/ce_head_ref.py restates them from include/amk.h.

Hard tier, composed as in tests/ce_head_ref.py with these changes (A = |x| |w|^T, p the fp64 softmax of a valid row,
s = d_loss / count):
* a bf16 x bf16 product is exact in f32, so a logit is one f32 chain over the staged contraction, K rounded up to the
  stage depth of 32 (the tail is zeros), plus one: n_K = 32 ceil(K / 32) + 1 (the rule of tests/bf16_dense_ref.py),
      ez = gamma_(n_K) A.
  The logits are never rounded to bf16: the unnormalised weights, the sums and merges, lse, loss_r and the mean are the
  f32 head's, with the same n_sum and n_rows (the tile, lane-half and slice structure is the same).
* g in f32 as the f32 head:  eg32 = |s| (p (ez + ebar + C u (1 + |z - lse|)) + 3 u |p - [v = t]| + 2^-120); its one
  rounding to bf16 is relative to the computed value:
      eg = eg32 + 2 U16 (|g| + eg32).
* dx: one f32 chain over v ascending (V + 1), then one rounding to bf16, relative to the computed value:
      edx32 = eg |w| + gamma_(V+1) |g| |w|,      edx = edx32 + 2 U16 (|dx| + edx32).
* dw: one f32 chain over the compacted rows ascending (count + 1), written as f32:
      eg^T |x| + gamma_(count+1) |g|^T |x|.

Tight tier.  S of an output is its bound with every gamma_n replaced by u (the U16 terms stay as they are), as
tests/ce_head_ref.py.  q = (|got - ref| - n 2^-126) / S is held to TIGHT_FACTOR x Q_EMU, the worst q of the CPU emulation
below (f32 chains in ascending order on bf16 values, tile order, lane halves, slice merge, the chunked row sum, g and dx
rounded once to bf16) over every family and shape class of tests/test_ce_head_bf16_bounds.py: measured from the
emulation, never from the kernel.

Measured on the MI355X, worst over tests/test_ce_head_bf16_gpu.py -- hard ratio, q / (4 Q_EMU):
    loss 0.010, 0.178        dx 0.434, 0.244        dw 0.469, 0.227
(dx and dw sit near 0.45 of the hard bound on every shape: the bound charges a bf16 rounding 2 U16 = 2^-7, the
rounding itself is at most 2^-8, and the G rounding dominates both gradients).
"""
import torch

import ce_head_ref as base
from ce_head_ref import (C_EXP, CPU_FAMILIES, F32, F64, FAMILIES, FTZ, SCAN, TILE, TINY, U32, gamma, make_target,  # noqa: F401
                         measures, slices)

U16 = 2.0 ** -8
BF16 = torch.bfloat16
TIGHT_FACTOR = 4.0
STAGE_K = 32

# worst q of the emulation per output (tests/test_ce_head_bf16_bounds.py::test_emulation_defines_q)
Q_EMU = {"loss": 0.4, "dx": 0.46, "dw": 0.54}


def logit_chain(K):
    return STAGE_K * ((K + STAGE_K - 1) // STAGE_K) + 1


def make_inputs(family, M, V, K, target, seed=0):
    """(x (M, K), w (V, K)) bf16 on the CPU: the family of tests/ce_head_ref.py rounded to bf16."""
    x, w = base.make_inputs(family, M, V, K, target, seed)
    return x.to(BF16).contiguous(), w.to(BF16).contiguous()


# ---------------------------------------------------------------------------------------------- reference
def reference(x, w, target, ignore_index=-1, d_loss=1.0):
    """{"loss", "dx", "dw", "bound_*", "unit_*", "abs_*", "count", "zmax"} in fp64 on x's device; zmax is the mean over
    the rows that count of max_v |z| (the cap of the comparison with the library path)."""
    X, W = x.detach().to(F64), w.detach().to(F64)
    M, K = X.shape
    V = W.shape[0]
    valid = target != ignore_index
    oor = valid & ((target < 0) | (target >= V))
    good = valid & ~oor
    count = int(valid.sum())
    rows = good.nonzero().flatten()
    R = {"count": count, "rows": rows, "poisoned": bool(oor.any()) or count == 0, "zmax": 0.0}
    dx = torch.zeros(M, K, dtype=F64, device=X.device)
    dw = torch.zeros(V, K, dtype=F64, device=X.device)
    zero = torch.zeros((), dtype=F64, device=X.device)
    for name, t in (("dx", dx), ("dw", dw)):
        R[name], R["bound_" + name], R["unit_" + name], R["abs_" + name] = t, torch.zeros_like(t), torch.zeros_like(t), 0.0
    R["loss"], R["bound_loss"], R["unit_loss"], R["abs_loss"] = zero + float("nan"), zero.clone(), zero.clone(), 0.0
    if rows.numel() == 0:
        return R
    Xr, t = X[rows], target[rows]
    z = Xr @ W.t()
    A = Xr.abs() @ W.abs().t()
    m = z.max(1).values
    lse = torch.logsumexp(z, 1)
    p = torch.exp(z - lse[:, None])
    zt = z.gather(1, t.view(-1, 1)).flatten()
    loss_r = lse - zt
    s = float(d_loss) / count
    onehot = torch.zeros_like(p).scatter_(1, t.view(-1, 1), 1.0)
    g = (p - onehot) * s
    if not R["poisoned"]:
        R["loss"] = loss_r.sum() / count
    R["zmax"] = float(z.abs().max(1).values.mean())
    dx[rows] = g @ W
    dw += g.t() @ Xr
    nsplit, vper = slices(M, V)
    T = vper // TILE
    n_sum = 66 * T + (T + nsplit + 1) * (C_EXP + 3) + 2
    n_rows = (count + SCAN - 1) // SCAN + 12
    n_k = logit_chain(K)

    def lin(gm):
        ez = gm(n_k) * A
        eps = ez + C_EXP * U32 * (1 + (z - m[:, None]).abs())
        ebar = (p * eps).sum(1) + gm(n_sum) + U32 * (lse.abs() + 2 * (lse - m).abs())
        row = ebar + ez.gather(1, t.view(-1, 1)).flatten() + U32 * (loss_r.abs() + lse.abs() + zt.abs())
        b_loss = row.sum() / count + gm(n_rows) * loss_r.abs().sum() / count
        eg32 = abs(s) * (p * (ez + ebar[:, None] + C_EXP * U32 * (1 + (z - lse[:, None]).abs())) + 3 * U32 * (p - onehot).abs() + TINY)
        eg = eg32 + 2 * U16 * (g.abs() + eg32)
        b_dx = torch.zeros_like(dx)
        edx32 = eg @ W.abs() + gm(V + 1) * (g.abs() @ W.abs())
        b_dx[rows] = edx32 + 2 * U16 * (dx[rows].abs() + edx32)
        b_dw = eg.t() @ Xr.abs() + gm(count + 1) * (g.abs().t() @ Xr.abs())
        return b_loss, b_dx, b_dw

    hard = lin(gamma)
    unit = lin(lambda n: U32)
    for name, h, un, n in zip(("loss", "dx", "dw"), hard, unit, (n_k + n_sum + n_rows, V + 1, count + 1)):
        R["abs_" + name] = n * FTZ
        R["bound_" + name] = h + n * FTZ
        R["unit_" + name] = un
    return R


def violations(got, R, name):
    """Elements outside either tier."""
    nbad, _, q = measures(got, R, name)
    return nbad + (1 if q > TIGHT_FACTOR * Q_EMU[name] else 0)


# ---------------------------------------------------------------------------------------------- CPU emulation
def round_bits(t, bits):
    """t rounded to `bits` significant bits (bf16 keeps 8)."""
    mant, e = torch.frexp(t.to(F32))
    return torch.ldexp(torch.round(mant * 2.0 ** bits) / 2.0 ** bits, e)


def emulate(x, w, target, ignore_index=-1, d_loss=1.0, mut=None):
    """(loss f32, dx bf16, dw f32) on the CPU in the kernels' order.  mut plants a fault: "mean_over_M",
    "ignore_not_honoured" (ignored rows take part with their target wrapped into the vocabulary), "target_off_by_one",
    "bits7" (every bf16 operand of the three products -- x, w and G -- rounded to 7 significant bits instead of bf16's
    8), "bf16_logits" (the library path's semantics: the logits rounded to bf16 before the softmax)."""
    x, w = x.to(F32), w.to(F32)
    M, K = x.shape
    V = w.shape[0]
    if mut == "bits7":
        x, w = round_bits(x, 7), round_bits(w, 7)
    if mut == "ignore_not_honoured":
        target = torch.where(target == ignore_index, target % V, target)
    valid = target != ignore_index
    rows = valid.nonzero().flatten()
    cnt = int(rows.numel())
    t = target[rows]
    if mut == "target_off_by_one":
        t = (t + 1) % V
    oor = (t < 0) | (t >= V)
    nan = torch.tensor(float("nan"), dtype=F32)
    dx = torch.zeros(M, K, dtype=BF16)
    if cnt == 0:
        return nan, dx, torch.zeros(V, K, dtype=F32)
    xr = x[rows]
    z = base._chain(xr, w.t().contiguous())                 # (cnt, V): f32 chain in ascending k, exact products
    if mut == "bf16_logits":
        z = z.to(BF16).to(F32)
    nsplit, vper = slices(M, V)
    T = vper // TILE
    zp = torch.full((cnt, nsplit * vper), float("-inf"), dtype=F32)
    zp[:, :V] = z
    # word v0 + 32 b + 8 g + 4 hf + e is accumulator register 4 g + e of block b in lane half hf
    zl = zp.view(cnt, nsplit, T, 4, 4, 2, 4).permute(0, 1, 2, 5, 3, 4, 6).reshape(cnt, nsplit, T, 2, 64)
    m = torch.full((cnt, nsplit, 2), float("-inf"), dtype=F32)
    s = torch.zeros(cnt, nsplit, 2, dtype=F32)
    for ti in range(T):
        tile = zl[:, :, ti]
        mn = torch.maximum(m, tile.max(-1).values)
        live = mn > float("-inf")
        mref = torch.where(live, mn, torch.zeros_like(mn))
        add = torch.zeros_like(s)
        for j in range(64):
            add = add + torch.exp(tile[..., j] - mref)
        scale = torch.where(m > float("-inf"), torch.exp(m - mref), torch.zeros_like(m))
        s = torch.where(live, base._fma(add, s, scale), s)
        m = mn
    mm = torch.maximum(m[..., 0], m[..., 1])

    def part(h):
        on = m[..., h] > float("-inf")
        return torch.where(on, s[..., h] * torch.exp(torch.where(on, m[..., h], mm) - mm), torch.zeros_like(mm))

    ps, pm = part(0) + part(1), mm
    mrow, srow = pm[:, 0], ps[:, 0]
    for sl in range(1, nsplit):
        om, os_ = pm[:, sl], ps[:, sl]
        m2 = torch.maximum(mrow, om)
        srow = base._fma(os_ * torch.exp(om - m2), srow, torch.exp(mrow - m2))
        mrow = m2
    lse = mrow + torch.log(srow)
    tc = t.clamp(0, V - 1)
    loss_r = torch.where(oor, nan, lse - z.gather(1, tc.view(-1, 1)).flatten())
    red = torch.zeros(SCAN, dtype=F32)
    for c0 in range(0, cnt, SCAN):
        chunk = loss_r[c0:c0 + SCAN]
        red[:chunk.numel()] = red[:chunk.numel()] + chunk
    o = SCAN // 2
    while o >= 1:
        red[:o] = red[:o] + red[o:2 * o]
        o //= 2
    denom = torch.tensor(float(M if mut == "mean_over_M" else cnt), dtype=F32)
    loss = red[0] / denom
    sc = torch.tensor(float(d_loss), dtype=F32) / denom
    onehot = torch.zeros_like(z).scatter_(1, tc.view(-1, 1), 1.0)
    g = (torch.exp(z - lse[:, None]) - onehot) * sc
    g = torch.where(oor[:, None], torch.zeros_like(g), g).to(BF16).to(F32)     # G: one rounding
    if mut == "bits7":
        g = round_bits(g, 7)                                                    # (G is the third bf16 operand)
    dxr = base._chain(g, w).to(BF16)                                            # dx: one rounding
    dx[rows] = torch.where(oor[:, None], torch.zeros_like(dxr), dxr)
    dw = base._chain(g.t().contiguous(), xr)
    return loss, dx, dw
