"""fp64 reference, per-element error bounds, input families, a restatement of the host's slicing and an f32 emulation
of the kernels' own order for the masked-token loss head of csrc/ce_head.hip (amk_ce_head_fwd / _bwd,
ops.linear_cross_entropy), as tests/dense_f32_ref.py does it for the dense GEMMs.

The reference is fp64 on the f32 values the kernels read (any device).  u = 2^-24.  No bound is relative to a tensor's
maximum.  Semantics restated from include/amk.h: a row is valid when target != ignore_index; count is the number of valid
rows; a valid row whose target is outside [0, V) makes the loss NaN, has a zero dx row and adds nothing to dw, while
s = d_loss / count still divides by the count that includes it; count == 0 gives loss NaN and zero gradients.

Hard tier (a theorem): gamma_n S + n 2^-126 per chain of n rounded operations (gamma_n = n u / (1 - n u)), composed
through the loss head to first order, every n read off csrc/ce_head.hip.  With A = |x| |w|^T, p the fp64 softmax of a
valid row, m its maximum, t its target, s = d_loss / count:
* logit (product(), mma_stage: one v_mfma_f32_32x32x2_f32 chain over K in ascending k, the K tail staged as zeros):
      ez = gamma_(K+1) A.
* unnormalised weight exp(z - ref) = __expf(z - ref): the subtraction (u |z - ref|), the multiplication by log2(e) inside
  __expf and that constant's own rounding (1.5 u |z - ref|), v_exp_f32 within one ulp (2 u): at most
  C u (1 + |z - ref|) with C = 4.  The running maximum only rises (tile by tile, then the lane-half merge, then the slice
  merges), each rise multiplies the sum by __expf(old - new), and the |old - new| of a word's path add up to |z - m|:
      eps_rv = ez_rv + C u (1 + |z_rv - m_r|)
  with the constant parts of the further factors counted in n_sum below.
* the sum and the merges, per row: a lane half adds 64 words per tile (64) and folds them into the running sum (2), T =
  vper / 128 tiles per slice; one lane-half merge and nsplit - 1 slice merges of two multiplications and an addition;
  T + nsplit + 1 rescale factors of C u each:
      n_sum = 66 T + (T + nsplit + 1) (C + 3) + 2
  lse = m + logf(s): logf within one ulp (2 u |lse - m|) and the addition (u |lse|):
      ebar_r = sum_v p eps + gamma_(n_sum) + u (|lse| + 2 |lse - m|).
* loss_r = lse - z_t:  ebar_r + ez_(r,t) + u (|loss_r| + |lse| + |z_t|).
* loss = (sum of the rows) / count: thread i of 1024 adds rows i, i + 1024, ... (ceil(count / 1024)), ten levels of the
  LDS tree, the division:  n_rows = ceil(count / 1024) + 12,
      loss: mean(row bounds) + gamma_(n_rows) mean |loss_r|.
* g = (exp(z - lse) - [v = t]) s in ce_bwd_g: the subtraction of the one-hot, the multiplication and s = d_loss / count
  round once each (3 u); weights that flush to zero in f32 are covered by 2^-120:
      eg_rv = |s| (p_rv (ez_rv + ebar_r + C u (1 + |z_rv - lse_r|)) + 3 u |p_rv - [v = t]| + 2^-120).
* dx (ce_bwd_dx: one chain over v ascending, V + 1):   eg |w| + gamma_(V+1) |g| |w|.
* dw (ce_bwd_dw: one chain over the compacted rows ascending, count + 1):   eg^T |x| + gamma_(count+1) |g|^T |x|.

Tight tier.  S of an output is its bound with every gamma_n replaced by u, over u: the chain parts as sum |t_i|, the
fixed parts in units of u (the `_mixed` form of tests/dense_f32_ref.py).  q = (|got - ref| - n 2^-126) / (u S) is held to
TIGHT_FACTOR x Q_EMU, the worst q of the f32 CPU emulation below (tile order, lane halves, slice merge, the chunked row
sum, the two gradient chains) over every family and shape class of tests/test_ce_head_bounds.py: measured from the
emulation, never from the kernel.

Measured on the MI355X, worst over tests/test_ce_head_gpu.py -- hard ratio, q / (4 Q_EMU):
    loss 0.015, 0.156        dx 0.071, 0.400        dw 0.151, 0.173
(the dx q grows with the length of its chain over the vocabulary: 5.3 at V = 8192, K = 36 against the emulation's 3.2 on
the same shape class; the hard ratios are largest where one or a few rows are valid).

Input families: unit (logit std 1), peaked (logit std about 10), large (a common offset of 3000 on every logit),
needle+30 / needle-30 / needle+90 (the target logit leads or trails the rest by that much), climb (the logits rise by
6.4 per 128-word tile, so the row maximum moves in every vocabulary tile).
"""
import math

import torch

U32 = 2.0 ** -24
FTZ = 2.0 ** -126
TINY = 2.0 ** -120
C_EXP = 4.0
TIGHT_FACTOR = 4.0
F64 = torch.float64
F32 = torch.float32
FAMILIES = ("unit", "peaked", "large", "needle+30", "needle-30", "climb")
CPU_FAMILIES = FAMILIES + ("needle+90",)
TILE = 128
SCAN = 1024

# worst q of the f32 emulation per output (tests/test_ce_head_bounds.py::test_emulation_defines_q)
Q_EMU = {"loss": 0.4, "dx": 3.3, "dw": 6.0}


def gamma(n):
    return n * U32 / (1 - n * U32)


def slices(M, V):
    """(nsplit, vper) of amk_ce_head_fwd: slices of whole 128-word tiles, no empty slice."""
    nrt = (M + TILE - 1) // TILE
    nvt = (V + TILE - 1) // TILE
    want = max(1, min((512 + nrt - 1) // nrt, 16, nvt))
    per = (nvt + want - 1) // want
    return (nvt + per - 1) // per, per * TILE


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ---------------------------------------------------------------------------------------------- inputs
def make_target(M, V, pattern, seed=0, ignore_index=-1):
    g = _gen(1000 + seed)
    t = torch.randint(0, V, (M,), generator=g)
    keep = torch.zeros(M, dtype=torch.bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "last_tile":
        keep[(M - 1) // TILE * TILE:] = True
    elif pattern == "random64":
        keep = torch.rand(M, generator=g) < 0.64
    elif pattern == "none":
        pass
    elif pattern == "edges":
        keep[:] = True
        _, vper = slices(M, V)
        edge = [0, V - 1, 127, 128, vper - 1, vper, 2 * vper - 1, 2 * vper, V - 2, 4, 3, 31, 32]
        edge = torch.tensor([min(max(e, 0), V - 1) for e in edge])
        t = edge[torch.arange(M) % len(edge)]
    else:
        raise ValueError(pattern)
    return torch.where(keep, t, torch.full_like(t, ignore_index))


def make_inputs(family, M, V, K, target, seed=0):
    """(x (M, K), w (V, K)) f32 on the CPU."""
    g = _gen(seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(V, K, generator=g) / math.sqrt(K)
    if family == "peaked":
        w = w * 10
    elif family == "large":
        x[:, 0] = 30.0
        w[:, 0] = 100.0
    elif family.startswith("needle"):
        a = float(family[len("needle"):])
        t = target.clamp(0, V - 1)
        wt = w[t]
        z_t = (x * wt).sum(1, keepdim=True)
        others = x @ w.t()
        top = others.scatter(1, t.view(-1, 1), float("-inf")).max(1, keepdim=True).values if V > 1 else z_t
        ref = top if a > 0 else others.scatter(1, t.view(-1, 1), float("inf")).min(1, keepdim=True).values if V > 1 else z_t
        x = x + (ref + a - z_t) * wt / (wt * wt).sum(1, keepdim=True).clamp_min(1e-6)
    elif family == "climb":
        if K >= 8:
            x[:, 1] = 1.0
            w[:, 1] = 0.05 * torch.arange(V, dtype=F32)
        else:
            x[:, 0] = 1.0
            w[:, 0] = 0.05 * torch.arange(V, dtype=F32)
    elif family != "unit":
        raise ValueError(family)
    return x.to(F32).contiguous(), w.to(F32).contiguous()


# ---------------------------------------------------------------------------------------------- reference
def reference(x, w, target, ignore_index=-1, d_loss=1.0):
    """{"loss", "dx", "dw", "bound_*", "unit_*" (= u S), "abs_*", "count"} in fp64 on x's device."""
    X, W = x.detach().to(F64), w.detach().to(F64)
    M, K = X.shape
    V = W.shape[0]
    valid = target != ignore_index
    oor = valid & ((target < 0) | (target >= V))
    good = valid & ~oor
    count = int(valid.sum())
    rows = good.nonzero().flatten()
    R = {"count": count, "rows": rows, "poisoned": bool(oor.any()) or count == 0}
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
    dx[rows] = g @ W
    dw += g.t() @ Xr
    nsplit, vper = slices(M, V)
    T = vper // TILE
    n_sum = 66 * T + (T + nsplit + 1) * (C_EXP + 3) + 2
    n_rows = (count + SCAN - 1) // SCAN + 12

    def lin(gm):
        ez = gm(K + 1) * A
        eps = ez + C_EXP * U32 * (1 + (z - m[:, None]).abs())
        ebar = (p * eps).sum(1) + gm(n_sum) + U32 * (lse.abs() + 2 * (lse - m).abs())
        row = ebar + ez.gather(1, t.view(-1, 1)).flatten() + U32 * (loss_r.abs() + lse.abs() + zt.abs())
        b_loss = row.sum() / count + gm(n_rows) * loss_r.abs().sum() / count
        eg = abs(s) * (p * (ez + ebar[:, None] + C_EXP * U32 * (1 + (z - lse[:, None]).abs())) + 3 * U32 * (p - onehot).abs() + TINY)
        b_dx = torch.zeros_like(dx)
        b_dx[rows] = eg @ W.abs() + gm(V + 1) * (g.abs() @ W.abs())
        b_dw = eg.t() @ Xr.abs() + gm(count + 1) * (g.abs().t() @ Xr.abs())
        return b_loss, b_dx, b_dw

    hard = lin(gamma)
    unit = lin(lambda n: U32)
    for name, h, un, n in zip(("loss", "dx", "dw"), hard, unit, (K + n_sum + n_rows, V + 1, count + 1)):
        R["abs_" + name] = n * FTZ
        R["bound_" + name] = h + n * FTZ
        R["unit_" + name] = un
    return R


def measures(got, R, name):
    """(elements outside the hard bound, worst hard ratio, worst q).  A NaN reference (poisoned loss) asks for NaN."""
    ref = R[name]
    got = got.detach().to(ref.device, F64).reshape(ref.shape)
    if name == "loss" and R["poisoned"]:
        return (0 if bool(torch.isnan(got)) else 1), 0.0, 0.0
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    bound, unit = R["bound_" + name], R["unit_" + name]
    zero_b = bound <= R["abs_" + name]     # rows that take no gradient: exact zeros
    nbad = int(((err > bound) | (zero_b & (err != 0))).sum())
    ratio = float((err / bound.clamp_min(FTZ)).max())
    q = float(((err - R["abs_" + name]).clamp_min(0) / unit.clamp_min(FTZ)).max())
    return nbad, ratio, q


def violations(got, R, name):
    """Elements outside either tier."""
    nbad, _, q = measures(got, R, name)
    return nbad + (1 if q > TIGHT_FACTOR * Q_EMU[name] else 0)


# ---------------------------------------------------------------------------------------------- f32 emulation
def _fma(acc, a, b):
    return (acc.double() + a.double() * b.double()).to(F32)


def _chain(Amat, Bmat):
    """sum_k A[:, k] B[k, :] as one MFMA chain in ascending k, one rounding per product (lane half 0's then half 1's)."""
    acc = torch.zeros(Amat.shape[0], Bmat.shape[1], dtype=F32)
    for k in range(Amat.shape[1]):
        acc = _fma(acc, Amat[:, k:k + 1], Bmat[k:k + 1, :])
    return acc


def emulate(x, w, target, ignore_index=-1, d_loss=1.0, mut=None):
    """(loss, dx, dw) in f32 on the CPU in the kernels' order.  mut plants a fault: "bf16" (operands rounded to bf16),
    "mean_over_M", "ignore_not_honoured" (ignored rows take part with their target wrapped into the vocabulary),
    "target_off_by_one"."""
    x, w = x.to(F32), w.to(F32)
    M, K = x.shape
    V = w.shape[0]
    if mut == "bf16":
        x, w = x.to(torch.bfloat16).to(F32), w.to(torch.bfloat16).to(F32)
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
    dx = torch.zeros(M, K, dtype=F32)
    if cnt == 0:
        return nan, dx, torch.zeros(V, K, dtype=F32)
    xr = x[rows]
    z = _chain(xr, w.t().contiguous())                      # (cnt, V)
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
        s = torch.where(live, _fma(add, s, scale), s)
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
        srow = _fma(os_ * torch.exp(om - m2), srow, torch.exp(mrow - m2))
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
    g = torch.where(oor[:, None], torch.zeros_like(g), g)
    dxr = _chain(g, w)
    dx[rows] = torch.where(oor[:, None], torch.zeros_like(dxr), dxr)
    dw = _chain(g.t().contiguous(), xr)
    return loss, dx, dw
