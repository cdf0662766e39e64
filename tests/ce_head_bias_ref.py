"""fp64 reference, per-element error bounds, bias families and a CPU emulation in the kernels' own order for the loss
head WITH A BIAS: amk_ce_head_bias_fwd / _bwd (csrc/ce_head.hip) and amk_ce_head_bias_bf16_fwd / _bwd
(csrc/ce_head_bf16.hip), ops.linear_cross_entropy(..., bias=b).  Targets, input families, the host's slicing, the
measures and every constant come from tests/ce_head_ref.py and tests/ce_head_bf16_ref.py, which this file imports and
does not change; `bf16=True` selects the second head everywhere (x and w are then bf16 values, the bias stays f32).

Semantics: z[m, v] = sum_k x[m, k] w[v, k] + b[v]; everything downstream as tests/ce_head_ref.py restates it;
db[v] = sum over the compacted rows of G[i, v] (f32), zeros when no row is valid; an out-of-range row's G row is zero, so
it gives nothing to db either.

Where the kernels add the bias: the accumulator of the logits tile is PRELOADED with b[v] instead of being cleared, so the
bias is the first term of the MFMA chain (one more rounded addition than the biasless chain, no separate rounding of a
biasless logit).  The f32 master bias is never rounded to bf16.

Hard tier, composed exactly as the parent files compose it, with these changes (A = |x| |w|^T):
* logit:  ez = gamma_(K+2) (A + |b|)   (f32)      ez = gamma_(n_K+1) (A + |b|)   (bf16, n_K = 32 ceil(K / 32) + 1).
  That covers the preload (a chain of K + 1 terms) and an addition after the chain alike.
* every downstream term (eps, n_sum, ebar, the row loss, the mean, eg, dx, dw; under bf16 the rounding of G and of dx) is
  the parent file's expression on the biased z.
* db (ce_bwd_db: thread (column, q) adds rows q, q + 32, q + 64, ... of G in ascending order -- ceil(count / 32) terms --
  then the 32 partial sums of a column fold as a binary tree in LDS, five levels):
      n_db = ceil(count / 32) + 5,      edb = sum_i eg_iv + gamma_(n_db) sum_i |g_iv|.
  Under bf16 eg carries the one rounding of G (2 U16 (|g| + eg32)) as it does for dw: db sums the same rounded values.

Tight tier: as the parent files (S = the bound with every gamma_n replaced by u); q is held to TIGHT_FACTOR x Q_EMU, the
worst q of the emulation below over tests/test_ce_head_bias_bounds.py: measured from the emulation, never from the kernel.

Bias families (make_bias), crossed with the input families of tests/ce_head_ref.py:
    zero      b = 0 (the faults that need a bias to show cannot show here)
    unit      randn
    dominant  randn x 30: the bias decides the softmax
    needle    b[v] = 30 + D on every word v that is the target of some valid row, 0 elsewhere, D the largest amount by
              which a row's target logit trails that row's best logit: in every row the target leads every word that is
              nobody's target by at least 30, and that lead comes from the bias alone
    offset    3000 + randn: a common offset (which the softmax cancels) over a unit spread (which it does not)

Measured on the MI355X, worst over tests/test_ce_head_bias_gpu.py and tests/test_ce_head_bias_bf16_gpu.py -- hard ratio,
q / (4 Q_EMU):
    f32:   loss 0.018, 0.176      dx 0.069, 0.212      dw 0.242, 0.169      db 0.248, 0.085
    bf16:  loss 0.007, 0.129      dx 0.453, 0.254      dw 0.474, 0.149      db 0.474, 0.172
(under bf16 dx, dw and db sit near 0.47 of the hard bound as in the biasless head: the bound charges the rounding of G
2 U16 = 2^-7, the rounding itself is at most 2^-8.  Against the library path under autocast at (129, 1000, 264) the fused
loss is off by 1.6e-7 / 7.5e-5 / 4.2e-6 / 2.1e-6 on unit x unit / large x unit / unit x dominant / peaked x offset, the
library's by 1.2e-3 / 5.7 / 1.7e-2 / 7.5.)
"""
import torch

import ce_head_bf16_ref as base16
import ce_head_ref as base
from ce_head_ref import (C_EXP, CPU_FAMILIES, F32, F64, FAMILIES, FTZ, SCAN, TILE, TINY, U32, gamma, make_target,  # noqa: F401
                         measures, slices)

U16 = base16.U16
BF16 = torch.bfloat16
TIGHT_FACTOR = 4.0
DB_GROUPS = 32                       # row groups of ce_bwd_db (threads per column)
BIAS_FAMILIES = ("zero", "unit", "dominant", "needle", "offset")
NAMES = ("loss", "dx", "dw", "db")
FAULTS = ("bias_dropped", "bias_shifted_by_one", "bias_on_forward_only", "db_over_all_rows", "db_mean_over_M")
NEED_A_BIAS = ("bias_dropped", "bias_shifted_by_one", "bias_on_forward_only")   # cannot show on the zero family

# worst q of the emulation per output (tests/test_ce_head_bias_bounds.py::test_emulation_defines_q)
Q_EMU = {False: {"loss": 0.43, "dx": 7.0, "dw": 9.0, "db": 8.7},
         True: {"loss": 0.37, "dx": 0.46, "dw": 0.82, "db": 0.71}}


def n_db(count):
    return (count + DB_GROUPS - 1) // DB_GROUPS + 5


def make_inputs(family, M, V, K, target, seed=0, bf16=False):
    return (base16 if bf16 else base).make_inputs(family, M, V, K, target, seed)


def make_bias(family, x, w, target, seed=0, ignore_index=-1):
    """b (V,) f32 on the CPU for CPU inputs x, w (either dtype)."""
    V = w.shape[0]
    g = torch.Generator().manual_seed(5000 + int(seed))
    r = torch.randn(V, generator=g)
    if family == "zero":
        b = torch.zeros(V)
    elif family == "unit":
        b = r
    elif family == "dominant":
        b = r * 30
    elif family == "offset":
        b = 3000 + r
    elif family == "needle":
        good = (target != ignore_index) & (target >= 0) & (target < V)
        b = torch.zeros(V)
        if bool(good.any()):
            z = x[good].double() @ w.double().t()
            zt = z.gather(1, target[good].view(-1, 1)).flatten()
            b[target[good]] = 30 + float((z.max(1).values - zt).max())
    else:
        raise ValueError(family)
    return b.to(F32).contiguous()


# ---------------------------------------------------------------------------------------------- reference
def reference(x, w, b, target, ignore_index=-1, d_loss=1.0, bf16=False):
    """{"loss", "dx", "dw", "db", "bound_*", "unit_*", "abs_*", "count", "zmax"} in fp64 on x's device."""
    X, W, B = x.detach().to(F64), w.detach().to(F64), b.detach().to(F64)
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
    db = torch.zeros(V, dtype=F64, device=X.device)
    zero = torch.zeros((), dtype=F64, device=X.device)
    for name, t in (("dx", dx), ("dw", dw), ("db", db)):
        R[name], R["bound_" + name], R["unit_" + name], R["abs_" + name] = t, torch.zeros_like(t), torch.zeros_like(t), 0.0
    R["loss"], R["bound_loss"], R["unit_loss"], R["abs_loss"] = zero + float("nan"), zero.clone(), zero.clone(), 0.0
    if rows.numel() == 0:
        return R
    Xr, t = X[rows], target[rows]
    z = Xr @ W.t() + B
    A = Xr.abs() @ W.abs().t() + B.abs()
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
    db += g.sum(0)
    nsplit, vper = slices(M, V)
    T = vper // TILE
    n_sum = 66 * T + (T + nsplit + 1) * (C_EXP + 3) + 2
    n_rows = (count + SCAN - 1) // SCAN + 12
    n_z = (base16.logit_chain(K) if bf16 else K + 1) + 1
    ndb = n_db(count)

    def lin(gm):
        ez = gm(n_z) * A
        eps = ez + C_EXP * U32 * (1 + (z - m[:, None]).abs())
        ebar = (p * eps).sum(1) + gm(n_sum) + U32 * (lse.abs() + 2 * (lse - m).abs())
        row = ebar + ez.gather(1, t.view(-1, 1)).flatten() + U32 * (loss_r.abs() + lse.abs() + zt.abs())
        b_loss = row.sum() / count + gm(n_rows) * loss_r.abs().sum() / count
        eg = abs(s) * (p * (ez + ebar[:, None] + C_EXP * U32 * (1 + (z - lse[:, None]).abs())) + 3 * U32 * (p - onehot).abs() + TINY)
        if bf16:
            eg = eg + 2 * U16 * (g.abs() + eg)
        b_dx = torch.zeros_like(dx)
        edx = eg @ W.abs() + gm(V + 1) * (g.abs() @ W.abs())
        b_dx[rows] = edx + 2 * U16 * (dx[rows].abs() + edx) if bf16 else edx
        b_dw = eg.t() @ Xr.abs() + gm(count + 1) * (g.abs().t() @ Xr.abs())
        b_db = eg.sum(0) + gm(ndb) * g.abs().sum(0)
        return b_loss, b_dx, b_dw, b_db

    hard = lin(gamma)
    unit = lin(lambda n: U32)
    for name, h, un, n in zip(NAMES, hard, unit, (n_z + n_sum + n_rows, V + 1, count + 1, ndb)):
        R["abs_" + name] = n * FTZ
        R["bound_" + name] = h + n * FTZ
        R["unit_" + name] = un
    return R


def violations(got, R, name, bf16=False):
    """Elements outside either tier."""
    nbad, _, q = measures(got, R, name)
    return nbad + (1 if q > TIGHT_FACTOR * Q_EMU[bf16][name] else 0)


# ---------------------------------------------------------------------------------------------- CPU emulation
def _chain_from(acc, Amat, Bmat):
    """acc + sum_k A[:, k] B[k, :] as one MFMA chain in ascending k that starts from the preloaded accumulator."""
    acc = acc.to(F32).clone()
    for k in range(Amat.shape[1]):
        acc = base._fma(acc, Amat[:, k:k + 1], Bmat[k:k + 1, :])
    return acc


def column_sums(G, cnt):
    """ce_bwd_db's order on G (cnt, V) f32: 32 interleaved row groups, each ascending, then a five-level binary tree."""
    V = G.shape[1]
    n = (cnt + DB_GROUPS - 1) // DB_GROUPS
    pad = torch.zeros(n * DB_GROUPS, V, dtype=F32)
    pad[:cnt] = G[:cnt]
    pad = pad.view(n, DB_GROUPS, V)
    part = torch.zeros(DB_GROUPS, V, dtype=F32)
    for j in range(n):
        part = part + pad[j]
    o = DB_GROUPS // 2
    while o >= 1:
        part[:o] = part[:o] + part[o:2 * o]
        o //= 2
    return part[0].clone()


def emulate(x, w, b, target, ignore_index=-1, d_loss=1.0, mut=None, bf16=False):
    """(loss f32, dx f32 / bf16, dw f32, db f32) on the CPU in the kernels' order.  mut plants one of FAULTS."""
    x, w, b = x.to(F32), w.to(F32), b.to(F32)
    M, K = x.shape
    V = w.shape[0]
    DX = BF16 if bf16 else F32
    if mut == "bias_dropped":
        b = torch.zeros_like(b)
    if mut == "bias_shifted_by_one":
        b = torch.roll(b, -1)                                 # word v takes b[v + 1]
    valid = target != ignore_index
    rows = valid.nonzero().flatten()
    cnt = int(rows.numel())
    t = target[rows]
    oor = (t < 0) | (t >= V)
    nan = torch.tensor(float("nan"), dtype=F32)
    dx = torch.zeros(M, K, dtype=DX)
    if cnt == 0:
        return nan, dx, torch.zeros(V, K, dtype=F32), torch.zeros(V, dtype=F32)
    xr = x[rows]
    wt = w.t().contiguous()
    z = _chain_from(b.expand(cnt, V), xr, wt)                 # (cnt, V): the bias is the chain's first term
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
    denom = torch.tensor(float(cnt), dtype=F32)
    loss = red[0] / denom
    sc = torch.tensor(float(d_loss), dtype=F32) / denom
    onehot = torch.zeros_like(z).scatter_(1, tc.view(-1, 1), 1.0)
    zb = base._chain(xr, wt) if mut == "bias_on_forward_only" else z       # ce_bwd_g's own logits tile
    g = (torch.exp(zb - lse[:, None]) - onehot) * sc
    g = torch.where(oor[:, None], torch.zeros_like(g), g)
    if bf16:
        g = g.to(BF16).to(F32)                                              # G: one rounding
    dxr = _chain_from(torch.zeros(cnt, K), g, w).to(DX)
    dx[rows] = torch.where(oor[:, None], torch.zeros_like(dxr), dxr)
    dw = _chain_from(torch.zeros(V, K), g.t().contiguous(), xr)
    if mut == "db_over_all_rows":      # G rows for the ignored rows too, their targets wrapped into the vocabulary
        ign = (~valid).nonzero().flatten()
        zi = _chain_from(b.expand(ign.numel(), V), x[ign], wt)
        pi = torch.softmax(zi, 1) - torch.zeros_like(zi).scatter_(1, (target[ign] % V).view(-1, 1), 1.0)
        gi = pi * sc
        g_all = torch.zeros(M, V, dtype=F32)
        g_all[rows], g_all[ign] = g, (gi.to(BF16).to(F32) if bf16 else gi)
        db = column_sums(g_all, M)
    else:
        db = column_sums(g, cnt)
    if mut == "db_mean_over_M":
        db = db * torch.tensor(cnt / M, dtype=F32)
    return loss, dx, dw, db
