"""fp64 reference, per-element error bounds and a CPU emulation in the kernels' own order for the fused GroupNorm + Swish of
the conv VQGAN, csrc/gn_act.hip (amk_gnact_fwd / _bwd, ops.group_norm_act).

Semantics (tests/gn_act_spec.py).  Per run (n, g) of m = cpg HW contiguous values, cpg = C / G:
    mu = mean x,  var = mean (x - mu)^2,  r = (var + eps)^-1/2,  xh = (x - mu) r,  y = gamma_c xh + beta_c,
    z = act(y): act 0 identity, act 1 swish y sigma(y);  a' = act'(y), swish' = sigma (1 + y (1 - sigma)),  gy = gz a'
    dbeta_c = sum_{n,hw} gy,  dgamma_c = sum_{n,hw} gy xh,  S1 = sum_run gamma_c gy,  S2 = sum_run gamma_c gy xh,
    gx = r (gamma_c gy - A - xh B),  A = S1 / m,  B = S2 / m.
The reference is gn_act_spec.fwd / bwd in fp64 on the f32 values of every input; eps is the f32 value the C ABI receives.

Geometry.  make_geo / seg_of / plane_steps restate the kernel's work split: a run is cpg planes of HW values; it is cut into
S segments (PP whole planes each, or Q pieces of L elements per plane once HW > 4096), and workgroup run S + s walks every
plane of its segment as a scalar head, a float4 body and a scalar tail; thread t adds the body runs t, t + 256, ... (four
elements each, in order) and then at most one edge element per plane.  T_seg is the longest such chain over a segment, T_pl
over one plane of a segment (the backward's partials are per plane).  A block reduction is a 6-level butterfly and 3 adds over
the waves; a fold of k partials is ceil(k / 256) adds per thread and a block reduction.  So no sum passes through more than
    D1 = T_seg + 9                          roundings for a segment's sum (the forward statistics),
    d_chan = min(ceil(S / 256) + 8, S - 1)  Chan merges on the path of any segment's statistics,
    Dp = T_pl + 9                           for a plane partial of the backward,
    Dn = Dp + ceil(N Q / 256) + 9           for dbeta (dgamma: + 1 for the product gy xh),
    Dg = Dp + ceil(cpg Q / 256) + 9 + 1     for S1 (the product gamma_c partial; S2: + 1 for gy xh).

Bounds.  w = 2^-24, gamma_k = k w / (1 - k w).  Every E is an absolute bound on |computed - exact|; sums of absolute values
run over the run (or the segment, index s).  The last rounding of an element-wise output is charged 2 w, and
tests/test_gn_act_bounds.py holds the emulation under HALF of every bound.

Statistics, as in tests/discr_norm_ref.py (the same two-pass segment statistics and Chan merge, a run in place of a channel):
    E_ms = gamma_(D1+1) mean_s |x|,   E_d = E_ms + w |d|  (d = x - m_s from the computed segment mean),
    E_qs = sum_s (2 |d| E_d + E_d^2) + gamma_(D1+2) (q_s + the sum before),
    E_mu = sum_s cnt_s E_ms / m + gamma_(d_chan) (mmax + 3 dm)      (mmax = max_s |m_s|, dm = max_s m_s - min_s m_s),
    E_M2 = sum_s E_qs + (dm e + e^2 / 2) m d_chan + gamma_(2 d_chan + 6) (M2 + sum_s E_qs),  e = 2 E_mu + w dm,
    E_var = E_M2 / m + w var,   delta = E_var / (var + eps),   rho = delta / (2 (1 - delta)) + 4 w   (relative error of rstd:
    the add, rsqrtf at 1 ulp; no bound (inf) once delta >= 0.9),       bound(mean) = E_mu,  bound(rstd) = r rho.
(`offset`: x = 100 + N(0, 1); the segment means are taken first, so var's error stays at gamma_(D1+2) var plus the squares of
E_d = 100 gamma_(D1+1): cancellation costs nothing.  `constant`: var = 0, r = eps^-1/2 = 1000, and y = beta only to within
|gamma| r E_mu: the mean of m equal values c is c only to within gamma_(D1+1) |c|.)

y = fmaf(x, scale, shift), scale = fl(gamma_c r), shift = fl(beta_c - fl(mu scale)); rs = rho + w (1 + rho):
    E_y = |gamma| r (|x - mu| rs + (1 + rs) E_mu) + w (1 + rs) (|x| + |mu|) |gamma| r + 2 w |y|.        act 0: bound(z) = E_y.

Swish.  sigma = rcp(fl(1 + e)), e = exp2(fl(-y fl(log2 e))) on v_exp_f32 and v_rcp_f32, 1 ulp = 2 w each.  The rounded
constant and the rounded product move the exponent by at most 2 w |y| in relative terms:
    de = 2 w |y| + 2 w                               relative error of e,
    ds = (1 - sigma) de + 3 w                        of sigma (the sum's rounding, the reciprocal's ulp).
e = inf (y < -88.7) gives sigma = 0 and z = -0 against |z| < 1e-36; a subnormal e or sigma may be flushed to 0, an absolute
error below 2^-125 (1 + |y|), which TINY covers.  swish'' = sigma (1 - sigma) (2 + y (1 - 2 sigma)), |swish''| <= 1/2:
    bound(z) = |swish'(y)| E_y + E_y^2 / 4 + |z| (ds + 2 w) + TINY.
a' = sigma p, p = 1 + v, v = y u, u = 1 - sigma; |swish'''| <= 1/2:
    E_u = sigma ds + w u,   E_v = |y| E_u + w |v|,   E_p = E_v + w |p|,
    E_a = |swish''(y)| E_y + E_y^2 / 4 + sigma E_p + |a'| (ds + w) + TINY              (act 0: E_a = 0),
    E_gy = |gz| E_a + w |gy|.
(u is formed as 1 - sigma, not e sigma, so that e = inf never meets sigma = 0; the price is an absolute 3 w on u, which at
y = 200 is 200 * 3 w = 3.6e-5 on a' = 1.  The bound says so.)

Backward, with the forward's f32 mean and rstd.  xh = fl(fl(x - mu) r):     E_xh = r (1 + rho) E_mu + |xh| (rho + 2 w)
    bound(dbeta)  = sum E_gy + gamma_Dn (sum |gy| + sum E_gy)
    bound(dgamma) = sum (|gy| E_xh + E_gy |xh|) + gamma_(Dn+1) (sum |gy xh| + the sum before)
    E_S1 = sum |gamma| E_gy + gamma_Dg (sum |gamma gy| + the sum before)
    E_S2 = sum |gamma| (|gy| E_xh + E_gy |xh|) + gamma_(Dg+1) (sum |gamma gy xh| + the sum before)
    A = fl(S1 fl(1 / m)):  E_A = E_S1 / m + 2 w |A|,  E_B alike
    I = fl(gamma gy) - A - fl(xh B):  E_I = |gamma| E_gy + E_A + |xh| E_B + |B| E_xh + E_xh E_B
                                            + w (2 |gamma gy| + |A| + |xh B| + |I|)
    bound(gx) = r (1 + rho) E_I + |gx| (rho + 2 w).
Every bound is multiplied by 1 + 2^-10 for the terms of relative order w left out above and gets the floor 1e-5 max |ref| of its
tensor, as elsewhere in the project.  Swish has no kink, so no element's branch is undetermined.

The constants are derived, not fitted: tests/test_gn_act_bounds.py holds the CPU emulation below (f32 torch ops in the
kernels' order, torch's exp2 and a correctly rounded division for the two hardware instructions) under HALF of every bound on
every family and case, and shows that four defects planted in the fp64 spec fall outside.  The emulation rounds after every
product and every sum, except in the explicit fmaf; the compiler may contract others into FMAs on the device, which only
removes roundings.

Measured on the MI355X, worst |got - ref| / bound over tests/test_gn_act_gpu.py, and the emulation's worst over
tests/test_gn_act_bounds.py below it:
    MI355X      z 0.167    mean 0.045    rstd 0.016    gx 0.155    dgamma 0.047    dbeta 0.036
    emulation   z 0.168    mean 0.045    rstd 0.016    gx 0.155    dgamma 0.047    dbeta 0.041
(All of them on `constant`, where r = 1000 multiplies the mean's error; on `diffuse` nothing passes 0.03.  The bounds are worst
cases over 20 to 40 roundings per sum, each charged its full w; the errors met add up like a random walk.)
"""
import functools

import torch

import gn_act_spec as spec
from discr_norm_ref import _block_sum, _chan_fold, _fmaf, _fold_sums, gamma_n

F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24
FLOOR = 1e-5
SLACK = 1.0 + 2.0 ** -10
TINY = 2.0 ** -125
BLOCK, SEG = 256, 4096
LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=F32))
EPS = float(torch.tensor(1e-6, dtype=F32))

FAMILIES = ("diffuse", "offset", "constant", "saturated", "gamma0")
TENSORS = ("z", "mean", "rstd", "gx", "dgamma", "dbeta")
# (N, C, H, W, G)
CASES = [(2, 32, 3, 3, 32),        # cpg 1, runs of 9: unaligned starts, tail only
         (1, 64, 1, 1, 32),        # HW = 1
         (3, 64, 5, 7, 32),        # odd HW, head + body + tail
         (2, 128, 16, 16, 32),     # a run of 1024
         (2, 512, 16, 16, 32),     # a run of 4096: the VQGAN bottleneck
         (1, 256, 33, 31, 32),     # a run just past a segment edge
         (1, 128, 256, 256, 32),   # a run of 262 144 over many segments: the largest layer
         (2, 48, 6, 6, 1), (2, 48, 6, 6, 48)]   # G = 1 and G = C
ALL_FAMILY_CASES = [CASES[0], CASES[4], CASES[5]]


def family_cases():
    """[(family, case)]: diffuse on every case, the other families on the first, the fifth and the sixth."""
    return [("diffuse", c) for c in CASES] + [(f, c) for f in FAMILIES[1:] for c in ALL_FAMILY_CASES]


WORST = {}


# ---------------------------------------------------------------------------------------------- geometry
def make_geo(C, HW, G):
    cpg = C // G
    if HW <= SEG:
        PP = min(SEG // HW, cpg)
        Q, L, S = 1, HW, (cpg + PP - 1) // PP
    else:
        PP = 1
        Q = (HW + SEG - 1) // SEG
        L = (((HW + Q - 1) // Q) + 3) & ~3
        S = cpg * Q
    return dict(C=C, G=G, cpg=cpg, HW=HW, PP=PP, Q=Q, L=L, S=S)


def seg_of(g, s):
    """(p0, p1, q, e0, e1): planes [p0, p1) of the run, piece q, elements [e0, e1) of each plane."""
    if g["Q"] == 1:
        p0 = s * g["PP"]
        return p0, min(g["cpg"], p0 + g["PP"]), 0, 0, g["HW"]
    p0, q = s // g["Q"], s % g["Q"]
    e0 = min(g["HW"], q * g["L"])
    return p0, p0 + 1, q, e0, min(g["HW"], e0 + g["L"])


def ws_floats(N, C, HW, G):
    return N * C * make_geo(C, HW, G)["Q"] * 2


def plane_steps(base, ln, pad, drop_tail=False):
    """(steps, 256) flat offsets thread t adds, in order, for `ln` elements at `base`; `pad` where it adds nothing."""
    head = min((4 - (base & 3)) & 3, ln)
    nv = (ln - head) >> 2
    tail = ln - head - 4 * nv
    it = (nv + BLOCK - 1) // BLOCK
    blk = torch.full((4 * it + 1, BLOCK), pad, dtype=torch.int64)
    i = torch.arange(nv)
    for k in range(4):
        blk[(i // BLOCK) * 4 + k, i % BLOCK] = base + head + 4 * i + k
    t = torch.arange(head)
    blk[4 * it, t] = base + t
    if not drop_tail:
        t = torch.arange(head, head + tail)
        blk[4 * it, t] = base + 4 * nv + t
    return blk


def _stack(rows, pad):
    T = max(r.shape[0] for r in rows)
    idx = torch.full((len(rows), T, BLOCK), pad, dtype=torch.int64)
    for k, r in enumerate(rows):
        idx[k, :r.shape[0]] = r
    return idx


@functools.lru_cache(maxsize=4)
def _plans(N, C, HW, G):
    """(seg (N G, S, T_seg, 256), plane (N C, Q, T_pl, 256)): the flat NCHW offset thread t adds at its step i of a segment
    and of one (plane, piece) of it, or N C HW (a zero) for none."""
    g = make_geo(C, HW, G)
    pad = N * C * HW
    seg_rows, plane_rows = [], {}
    for run in range(N * G):
        for s in range(g["S"]):
            p0, p1, q, e0, e1 = seg_of(g, s)
            steps = []
            for p in range(p0, p1):
                pl = run * g["cpg"] + p
                blk = plane_steps(pl * HW + e0, e1 - e0, pad)
                plane_rows[(pl, q)] = blk
                steps.append(blk)
            seg_rows.append(torch.cat(steps))
    seg = _stack(seg_rows, pad)
    plane = _stack([plane_rows[(pl, q)] for pl in range(N * C) for q in range(g["Q"])], pad)
    return seg.view(N * G, g["S"], -1, BLOCK), plane.view(N * C, g["Q"], -1, BLOCK)


@functools.lru_cache(maxsize=None)
def _segmap(C, HW, G):
    """(segid (m) of every element of a run in memory order, cnt (S))."""
    g = make_geo(C, HW, G)
    segid = torch.empty(g["cpg"], HW, dtype=torch.int64)
    cnt = []
    for s in range(g["S"]):
        p0, p1, _, e0, e1 = seg_of(g, s)
        segid[p0:p1, e0:e1] = s
        cnt.append((p1 - p0) * (e1 - e0))
    return segid.reshape(-1), torch.tensor(cnt, dtype=F64)


def depths(N, C, HW, G):
    """(D1, d_chan, Dp, Dn, Dg) of the module docstring."""
    g = make_geo(C, HW, G)
    seg, plane = _plans(N, C, HW, G)
    trips = lambda k: (k + BLOCK - 1) // BLOCK  # noqa: E731
    Dp = plane.shape[2] + 9
    return (seg.shape[2] + 9, min(trips(g["S"]) + 8, g["S"] - 1), Dp, Dp + trips(N * g["Q"]) + 9,
            Dp + trips(g["cpg"] * g["Q"]) + 10)


# ---------------------------------------------------------------------------------------------- inputs
def make_inputs(family, case, seed=0):
    """dict of CPU f32 tensors: x, gz (N, C, H, W), gamma, beta (C)."""
    N, C, H, W, G = case
    gen = torch.Generator().manual_seed(100003 * seed + 7919 * FAMILIES.index(family) + 31 * N + 17 * C + 1009 * H + W + 13 * G)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    x, gz = rn(N, C, H, W), rn(N, C, H, W)
    gamma, beta = rn(C), rn(C)
    if family == "offset":
        x = 100 + x
    elif family == "constant":
        x = rn(N, G, 1).expand(N, G, (C // G) * H * W).reshape(N, C, H, W).contiguous()
    elif family == "saturated":           # xh of a uniform x lies in +-sqrt(3): y = gamma xh + beta spreads over +-200
        x = 2 * torch.rand(N, C, H, W, generator=gen) - 1
        sign = torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
        gamma = sign * (200 / 3 ** 0.5) * (0.5 + 0.5 * torch.rand(C, generator=gen))
    elif family == "gamma0":
        gamma[1::3] = 0.0
        beta[4::6] = 0.0                  # every other gamma == 0 channel has beta == 0 as well
    return dict(x=x, gz=gz, gamma=gamma, beta=beta)


# ---------------------------------------------------------------------------------------------- reference
def reference(inp, G, act):
    """{name: fp64 reference, "bound_" + name: per-element bound} for name in TENSORS."""
    x = inp["x"].to(F64)
    N, C, H, W = x.shape
    HW, cpg = H * W, C // G
    m, R = cpg * HW, N * G
    w = U32
    gam, bet, gz = inp["gamma"].to(F64), inp["beta"].to(F64), inp["gz"].to(F64)
    z, mu, r = spec.fwd(x, gam, bet, G, EPS, act)
    gx, dgamma, dbeta = spec.bwd(gz, x, gam, bet, mu, r, G, act)
    Rf = dict(z=z, mean=mu, rstd=r, gx=gx, dgamma=dgamma, dbeta=dbeta)

    rm = lambda t: t.reshape(R, m)  # noqa: E731
    chan = lambda v: v.view(1, G, cpg, 1).expand(N, G, cpg, HW).reshape(R, m)  # noqa: E731   per-channel -> (R, m)
    tot = lambda t: t.sum(1, keepdim=True)  # noqa: E731
    per_c = lambda t: t.reshape(N, G, cpg, HW).sum((0, 3)).reshape(C)  # noqa: E731
    X, GZ = rm(x), rm(gz)
    GAM, BET = chan(gam), chan(bet)
    mu, r = mu.reshape(R, 1), r.reshape(R, 1)
    D1, d_chan, Dp, Dn, Dg = depths(N, C, HW, G)
    segid, cnt = _segmap(C, HW, G)
    S = cnt.numel()
    segsum = lambda v: torch.zeros(R, S, dtype=F64).index_add_(1, segid, v)  # noqa: E731

    m_s = segsum(X) / cnt
    E_ms = gamma_n(D1 + 1) * segsum(X.abs()) / cnt
    mmax = m_s.abs().max(1, keepdim=True).values
    dm = m_s.max(1, keepdim=True).values - m_s.min(1, keepdim=True).values
    E_mu = tot(E_ms * cnt) / m + gamma_n(d_chan) * (mmax + 3 * dm)
    ds = X - m_s[:, segid]
    E_d = E_ms[:, segid] + w * ds.abs()
    dq = segsum(2 * ds.abs() * E_d + E_d * E_d)
    E_qs = tot(dq + gamma_n(D1 + 2) * (segsum(ds * ds) + dq))
    d = X - mu
    M2 = tot(d * d)
    var = M2 / m
    e = 2 * E_mu + w * dm
    E_M2 = E_qs + (dm * e + e * e / 2) * m * d_chan + gamma_n(2 * d_chan + 6) * (M2 + E_qs)
    E_var = E_M2 / m + w * var
    delta = E_var / (var + EPS)
    rho = torch.where(delta < 0.9, delta / (2 * (1 - delta.clamp(max=0.9))) + 4 * w, torch.full_like(delta, float("inf")))
    B = {"mean": E_mu, "rstd": r * rho}

    rs = rho + w * (1 + rho)
    gr = GAM.abs() * r
    xh = d * r
    y = GAM * xh + BET
    E_y = gr * (d.abs() * rs + (1 + rs) * E_mu) + w * (1 + rs) * (X.abs() + mu.abs()) * gr + 2 * w * y.abs()
    Z = rm(z)
    if act == 1:
        sg = torch.sigmoid(y)
        u = torch.sigmoid(-y)                       # 1 - sigma without cancellation
        de = 2 * w * y.abs() + 2 * w
        dsg = u * de + 3 * w
        sw1 = sg * (1 + y * u)
        sw2 = sg * u * (2 + y * (u - sg))
        B["z"] = sw1.abs() * E_y + E_y * E_y / 4 + Z.abs() * (dsg + 2 * w) + TINY
        v = y * u
        E_u = sg * dsg + w * u
        E_v = y.abs() * E_u + w * v.abs()
        E_p = E_v + w * (1 + v).abs()
        E_a = sw2.abs() * E_y + E_y * E_y / 4 + sg * E_p + sw1.abs() * (dsg + w) + TINY
        a1 = sw1
    else:
        B["z"] = E_y
        E_a = torch.zeros_like(y)
        a1 = torch.ones_like(y)
    gy = GZ * a1
    E_gy = GZ.abs() * E_a + w * gy.abs()
    E_xh = r * (1 + rho) * E_mu + xh.abs() * (rho + 2 * w)
    B["dbeta"] = per_c(E_gy) + gamma_n(Dn) * (per_c(gy.abs()) + per_c(E_gy))
    t0 = gy.abs() * E_xh + E_gy * xh.abs()
    B["dgamma"] = per_c(t0) + gamma_n(Dn + 1) * (per_c((gy * xh).abs()) + per_c(t0))
    t1 = tot(GAM.abs() * E_gy)
    E_S1 = t1 + gamma_n(Dg) * (tot((GAM * gy).abs()) + t1)
    t2 = tot(GAM.abs() * t0)
    E_S2 = t2 + gamma_n(Dg + 1) * (tot((GAM * gy * xh).abs()) + t2)
    A, Bm = tot(GAM * gy) / m, tot(GAM * gy * xh) / m
    E_A, E_B = E_S1 / m + 2 * w * A.abs(), E_S2 / m + 2 * w * Bm.abs()
    gg = GAM * gy
    I = gg - A - xh * Bm  # noqa: E741
    E_I = (GAM.abs() * E_gy + E_A + xh.abs() * E_B + Bm.abs() * E_xh + E_xh * E_B
           + w * (2 * gg.abs() + A.abs() + (xh * Bm).abs() + I.abs()))
    B["gx"] = r * (1 + rho) * E_I + rm(gx).abs() * (rho + 2 * w)
    for name, b in B.items():
        ref = Rf[name]
        floor = FLOOR * float(ref.abs().max()) if ref.numel() else 0.0
        Rf["bound_" + name] = (b * SLACK + floor).reshape(ref.shape)
    return Rf


def ratios(got, R, names=TENSORS, record=True):
    """{name: worst |got - ref| / bound}; a non-finite value counts as inf."""
    out = {}
    for name in names:
        v = got[name].detach().to(F64).cpu().reshape(R[name].shape)
        q = (v - R[name]).abs() / R["bound_" + name]
        q = torch.where(torch.isfinite(v), q, torch.full_like(q, float("inf")))
        out[name] = float(q.max()) if q.numel() else 0.0
        if record:
            WORST[name] = max(WORST.get(name, 0.0), out[name])
    return out


# ---------------------------------------------------------------------------------------------- CPU emulation
def _sums(v, idx):
    """(A, B) sums of the f32 tensor v over idx (A, B, T, 256) in the kernel's order."""
    flat = torch.cat([v.reshape(-1), torch.zeros(1, dtype=F32)])
    acc = torch.zeros(idx.shape[0], idx.shape[1], BLOCK, dtype=F32)
    for i in range(idx.shape[2]):
        acc = acc + flat[idx[:, :, i]]
    return _block_sum(acc)


def _sigmoid(y):
    e = torch.exp2(-y * torch.tensor(LOG2E_F32, dtype=F32))
    return 1.0 / (1.0 + e)


def emulate(inp, G, act):
    """{name: f32 tensor for name in TENSORS} on the CPU: f32 torch ops in the kernels' order."""
    x, gz = inp["x"].to(F32), inp["gz"].to(F32)
    gamma, beta = inp["gamma"].to(F32), inp["beta"].to(F32)
    N, C, H, W = x.shape
    HW, cpg = H * W, C // G
    m, R = cpg * HW, N * G
    g = make_geo(C, HW, G)
    Q = g["Q"]
    seg, plane = _plans(N, C, HW, G)
    segid, cnt64 = _segmap(C, HW, G)
    cnt = cnt64.to(F32)
    f = lambda v: torch.tensor(v, dtype=F32)  # noqa: E731
    run_to_x = lambda v: v.reshape(N, G, 1).expand(N, G, cpg).reshape(N, C, 1, 1)  # noqa: E731
    ch = lambda v: v.view(1, C, 1, 1)  # noqa: E731

    # forward: stats_kernel, then the fold of fwd_apply_kernel
    seg_mean = _sums(x, seg) / cnt
    dd = x - seg_mean[:, segid].reshape(N, C, H, W)
    a = _chan_fold(cnt, seg_mean, _sums(dd * dd, seg))
    mu, r = a[:, 1], torch.rsqrt(a[:, 2] / a[:, 0] + f(EPS))
    MU, RR = run_to_x(mu), run_to_x(r)
    scale = ch(gamma) * RR
    shift = ch(beta) - MU * scale
    y = _fmaf(x, scale, shift)
    if act == 1:
        sg = _sigmoid(y)
        z = y * sg
        a1 = sg * (1.0 + y * (1.0 - sg))
    else:
        z, a1 = y, torch.ones_like(y)

    # backward: bwd_reduce_kernel, the fold of bwd_apply_kernel, param_grad_kernel
    xh = (x - MU) * RR
    gy = gz * a1
    p0, p1 = _sums(gy, plane), _sums(gy * xh, plane)                                 # (N C, Q)
    gpl = gamma.view(1, C, 1).expand(N, C, Q).reshape(N * C, Q)
    S1 = _fold_sums((gpl * p0).reshape(R, cpg * Q))
    S2 = _fold_sums((gpl * p1).reshape(R, cpg * Q))
    inv_m = f(1.0) / f(float(m))
    A, Bc = run_to_x(S1 * inv_m), run_to_x(S2 * inv_m)
    gx = RR * (ch(gamma) * gy - A - xh * Bc)
    by_c = lambda p: p.view(N, C, Q).permute(1, 0, 2).reshape(C, N * Q)  # noqa: E731
    return dict(z=z, mean=mu.view(N, G), rstd=r.view(N, G), gx=gx, dgamma=_fold_sums(by_c(p1)), dbeta=_fold_sums(by_c(p0)))
