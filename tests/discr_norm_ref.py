"""fp64 reference, per-element error bounds and a CPU emulation in the kernels' own order for the fused training-mode
BatchNorm2d + LeakyReLU of the PatchGAN discriminator, csrc/discr_norm.hip (amk_bnact_fwd / _bwd / _bwd_bwd,
ops.bn_leaky_relu): forward with running statistics, first-order backward, and the gradient penalty's double backward.

Semantics (tests/discr_norm_spec.py).  Per channel, n = N H W:
    mu = mean x,  var = mean (x - mu)^2,  r = (var + eps)^-1/2,  xh = (x - mu) r,  y = gamma xh + beta,
    z = y > 0 ? y : slope y,  s = dz/dy,  gy = s gz
    run_mean = (1 - m) run_mean + m mu,  run_var = (1 - m) run_var + m M2 / (n - 1),  M2 = n var
    gx = gamma r (gy - A - xh B),  dbeta = Sgy = n A,  dgamma = Sgyx = n B
    C, D, E = mean ggx, mean ggx xh, mean ggx gy
    g_gz = s [gamma r (ggx - C - xh D) + gg_gamma xh + gg_beta]
    g_x  = gg_gamma r (gy - A - xh B) - gamma r^2 [xh (E - AC - 3BD) + B (ggx - C) + D (gy - A)]
    g_gamma = n r (E - AC - BD)
The reference is discr_norm_spec.fwd / bwd / bwd_bwd in fp64 on the f32 values of every input; eps, momentum and slope are
the f32 values the C ABI receives.

Geometry.  make_geo / seg_of / plane_walk restate the kernel's work split: a channel is cut into S segments (PP whole
planes each, or Q pieces of L elements per plane once HW > 4096), and workgroup (s, c) walks every plane of its segment as a
scalar head, a float4 body and a scalar tail; thread t adds the body runs t, t + 256, ... (four elements each, in order) and
then at most one edge element per plane.  T_chain is the longest such chain over all segments (HW == 1: thread 0 adds every
plane of the segment).  The block reduction is a 6-level butterfly and 3 adds over the waves, so with
    D1 = T_chain + 9        no partial sum of a segment passes through more than D1 roundings, and with
    d_fold = ceil(S / 256) + 9,  D = D1 + d_fold        none of a channel sum (fold_sums adds the S partials the same way),
    d_chan = min(ceil(S / 256) + 8, S - 1)              Chan merges on the path of any segment's statistics.

Bounds.  w = 2^-24, gamma_k = k w / (1 - k w).  Every E is an absolute bound on |computed - exact|.  Sums of absolute values
run over the channel (or the segment, index s).  The last rounding of an element-wise output is charged 2 w: it is attained,
and tests/test_discr_norm_bounds.py holds the emulation under HALF of every bound.

Segment statistics (two passes).  m_s = fl(sum) / cnt:          E_ms = gamma_(D1+1) mean_s |x|.
d = x - m_s is formed from the computed mean:                   E_d  = E_ms + w |d|
    q_s = sum d^2:     E_qs = sum_s (2 |d| E_d + E_d^2) + gamma_(D1+2) (q_s + the sum before).
Chan's merge.  a1 += (b1 - a1) b0 / n: its inputs' errors enter as a convex combination, and the merge itself rounds the
difference, the fraction, the product and the sum.  Intermediate means lie between the segment means (mmax = max_s |m_s|,
dm = max_s m_s - min_s m_s):
    E_mu = sum_s cnt_s E_ms / n + gamma_(d_chan) (mmax + 3 dm).
a2 += b2 + d^2 a0 f.  Exactly, M2 = sum_s q_s + sum_s cnt_s (m_s - mu)^2.  The cross terms see d off by e = 2 E_mu + w dm, and
sum over merges of a0 b0 / (a0 + b0) <= n d_chan / 2; every merge rounds the products (5) and the two sums:
    E_M2 = sum_s E_qs + (dm e + e^2 / 2) n d_chan + gamma_(2 d_chan + 6) (M2 + sum_s E_qs),    E_var = E_M2 / n + w var
    rho  = delta / (2 (1 - delta)) + 4 w,  delta = E_var / (var + eps)    (relative error of rstd: the add, rsqrtf at 1 ulp;
           |(1 + t)^-1/2 - 1| <= |t| / (2 (1 - |t|)); no bound (inf) once delta >= 0.9, and then none on anything below)
    bound(mean) = E_mu,  bound(rstd) = r rho
    bound(run_mean) = m E_mu + gamma_4 (|(1 - m) run_mean| + |m mu|)
    bound(run_var)  = m (E_M2 / (n - 1) + w M2 / (n - 1)) + gamma_4 (|(1 - m) run_var| + |m M2 / (n - 1)|).

y = fmaf(x, scale, shift), scale = fl(gamma r), shift = fl(beta - fl(mu scale)); rs = rho + w (1 + rho) is scale's relative
error.  x scale - mu scale = scale (x - mu): the mean's error enters once, scale's only on the centred value; shift rounds
twice, at |mu scale| and at |shift| <= |y| + |x scale|; the fma rounds at |y|:
    E_y = |gamma| r (|x - mu| rs + (1 + rs) E_mu) + w (1 + rs) (|x| + |mu|) |gamma| r + 2 w |y|
    bound(z) = E_y (y > 0),  slope E_y + 2 w |z| (y <= 0).
(So a channel whose values are all one nonzero constant c gives y = beta only to within w |c gamma| r, r = eps^-1/2: shift
rounds at |c gamma r|.  With c == 0, or gamma == 0, y == beta to the bit.)

The kink.  K = {elements with |y| <= E_y and E_y > 0}: the f32 sign of y is not determined there (E_y == 0 only where
gamma == 0 and beta == 0: y == 0 exactly there, on the slope's side in f32 as in fp64).  For an element of K, z is held to
2 E_y + 2 w |z| and gx, g_gz, g_x to the nearer of the two branches of s, each with its own bound; every sum that contains s
gets (1 - slope) sum_K |term|.  reference()
asserts |K| <= KINK_CAP of the case's elements.  KINK_CAP is 1e-4, except for the `offset` family, where no seed can meet it:
there |mu| r = 10^3, so E_y is at least 2 w |mu gamma| r = 1.2e-4 |gamma| from shift's two roundings alone, and with the mean's
error, gamma_40 |mu| (D1 + 1 + d_chan <= 40 on the shapes tested), E_y is about 2.4e-3 |gamma|; y has density 0.4 / |gamma| at
0, so about 2 E_y 0.4 / |gamma| = 1.9e-3 of the elements fall into K (1.3e-3 to 2.1e-3 on the shapes tested).  Its cap is 4e-3,
twice that estimate.  The price is in the sums that contain s: with 2e-3 of the elements in K, (1 - slope) sum_K |term| makes
bound(dgamma), bound(dbeta) and bound(g_gamma) on `offset` 5e-2 of the tensor's maximum at best and more than the maximum on
the 300-segment shape (on `diffuse` they are 1e-4 to 3e-3 of it).  `offset` therefore holds the forward, the statistics and the
element-wise gx, g_gz and g_x (bounds of 2e-3 to 5e-3 of the maximum, 5e-2 for g_x), but the channel sums only loosely; those
are held by the other five families, whose K is at most a handful of elements.

Backward, with the forward's f32 mean and rstd.  xh = fl(fl(x - mu) r):     E_xh = r (1 + rho) E_mu + |xh| (rho + 2 w)
    gy = s gz:  E_gy = w |gy|
    E_Sgy  = sum E_gy + gamma_D (sum |gy| + sum E_gy) + (1 - slope) sum_K |gz|                                = bound(dbeta)
    E_Sgyx = sum (|gy| E_xh + E_gy |xh|) + gamma_(D+1) (sum |gy xh| + the sum before)
             + (1 - slope) sum_K |gz| (|xh| + E_xh)                                                           = bound(dgamma)
    A = fl(Sgy fl(1 / n)):  E_A = E_Sgy / n + 2 w |A|,  E_B alike
    I = gy - A - xh B:      E_I = E_gy + E_A + |xh| E_B + |B| E_xh + E_xh E_B + w (|gy| + |A| + |xh B| + |I|)
    bound(gx) = |gamma| r (1 + rs) E_I + |gx| (rs + 2 w).

Double backward, with the backward's f32 sums (A, B as above).
    E_C = gamma_D mean |ggx| + 2 w |C|
    E_D = mean |ggx| E_xh + gamma_(D+1) (mean |ggx xh| + the mean before) + 2 w |D|
    E_E = mean |ggx| E_gy + gamma_(D+1) (mean |ggx gy| + the mean before) + (1 - slope) sum_K |ggx gz| / n + 2 w |E|
    P(k) = E_E + |A| E_C + |C| E_A + E_A E_C + k (|B| E_D + |D| E_B + E_B E_D)
    E_T  = P(1) + gamma_3 (|E| + |AC| + |BD|),   E_k1 = P(3) + gamma_4 (|E| + |AC| + 3 |BD|)
    bound(g_gamma) = n r (1 + rho) E_T + |g_gamma| (rho + 3 w)
The means enter with the absolute values of their terms, so T = E - AC - BD gets what its conditioning warrants: with
cotangents of mean c and deviation 0.01 c (`mean_heavy`), |E| and |AC| are about c^2 while T is 10^-4 c^2.
    q = ggx - C:  E_q = E_C + w |q|;      J = q - xh D:  E_J = E_q + |D| E_xh + |xh| E_D + E_xh E_D + w (|xh D| + |J|)
    t1 = scale J: E_t1 = |gamma| r (1 + rs) E_J + |t1| (rs + w);      t2 = gg_gamma xh:  E_t2 = |gg_gamma| E_xh + w |t2|
    t = t1 + t2 + gg_beta:  E_t = E_t1 + E_t2 + w (|t1| + |t2|) + 2 w |t|
    bound(g_gz) = E_t (y > 0),  slope E_t + 2 w |g_gz| (y <= 0)
    u1 = fl(gg_gamma r) I:  E_u1 = |gg_gamma| r (1 + rho + w) E_I + |u1| (rho + 2 w)
    G = gy - A:  E_G = E_gy + E_A + w |G|
    V = xh k1 + B q + D G:  E_V = |k1| E_xh + |xh| E_k1 + E_xh E_k1 + |B| E_q + |q| E_B + E_q E_B + |D| E_G + |G| E_D + E_G E_D
                                  + gamma_3 (|xh k1| + |B q| + |D G|)
    u2 = fl(scale r) V, 1 + r2 = (1 + rs) (1 + rho) (1 + w):  E_u2 = |gamma| r^2 (1 + r2) E_V + |u2| (r2 + w)
    bound(g_x) = E_u1 + E_u2 + 2 w (|u1| + |u2|).
Every bound is multiplied by 1 + 2^-10 for the terms of relative order w left out above (a rounding unit times a relative
error already charged) and gets the floor 1e-5 max |ref| of its tensor, as elsewhere in the project.

The constants are derived, not fitted: tests/test_discr_norm_bounds.py holds the CPU emulation below (f32 torch ops in the
kernels' order) under HALF of every bound on every family and shape, and shows that planted defects fall outside.  The
emulation rounds after every product and every sum, except in the explicit fmaf.  The compiler is free to contract
`q += d * d`, `beta - mu * scale`, `gy - A - xh * B` or `E - A * Cc - B * D` into FMAs on the device, which only removes
roundings: the emulation is an upper model of the kernels' roundings, not their arithmetic bit for bit, and the two ratios of
one case differ.  (The exact cases do not depend on it: a term multiplied by scale == 0 contributes 0 either way.)

Measured on the MI355X, worst |got - ref| / bound over tests/test_discr_norm_bounds_gpu.py (all f32: no tensor has a
low-precision rounding, and none comes near 0.5), and the emulation's worst over tests/test_discr_norm_bounds.py below it:
    MI355X      z 0.074    mean 0.010    rstd 0.007    run_mean 0.014    run_var 0.009    gx 0.032    dgamma 0.024
                dbeta 0.006    g_gz 0.028    g_x 0.014    g_gamma 0.028
    emulation   z 0.032    mean 0.010    rstd 0.008    run_mean 0.011    run_var 0.008    gx 0.026    dgamma 0.018
                dbeta 0.005    g_gz 0.027    g_x 0.013    g_gamma 0.028
(The bounds are worst cases over D1 + d_fold = 20 to 40 roundings per sum, each charged its full w; the errors met add up
like a random walk.  g_gamma's 0.028 is `offset` at (1, 2, 1, 2) in both rows, a channel of two elements.)
On `mean_heavy` alone, where E - AC - BD and E - AC - 3BD cancel to 1e-4 of their terms (WORST_BY_FAMILY):
    MI355X      g_gamma 0.019    g_x 0.012    g_gz 0.028 (input_grad_only, no gg_gamma / gg_beta; 0.010 with them)    gx 0.016
    emulation   g_gamma 0.012    g_x 0.013    g_gz 0.010    gx 0.016
The kernel sits where the emulation does, far inside the allowance the absolute values of E, AC and BD give: it loses no more
to the uncentred means than the order of its sums predicts.
"""
import functools

import torch

import discr_norm_spec as spec

F32, F64 = torch.float32, torch.float64
U32 = 2.0 ** -24
FLOOR = 1e-5
SLACK = 1.0 + 2.0 ** -10
BLOCK, WAVES, SEG = 256, 4, 4096


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


EPS, MOMENTUM, SLOPE = _f32(1e-5), _f32(0.1), _f32(0.2)
FAMILIES = ("diffuse", "offset", "mean_heavy", "dead_channel", "flat_channel", "sparse_cotangent")
TENSORS = ("z", "mean", "rstd", "run_mean", "run_var", "gx", "dgamma", "dbeta", "g_gz", "g_x", "g_gamma")
TWO_BRANCH = ("gx", "g_gz", "g_x")
# (N, C, H, W).  CPU_SHAPES run in tests/test_discr_norm_bounds.py and on the GPU, GPU_SHAPES on the GPU only.
CPU_SHAPES = [(2, 3, 1, 1), (1, 2, 1, 2),
              (5, 4, 31, 31),        # PP = 4, S = 2, the last segment one plane
              (2, 3, 65, 65),        # Q = 2, odd HW: another head and tail on every plane
              (300, 2, 3, 683)]      # HW = 2049, PP = 1, S = 300 > 256: a second trip through the folds
GPU_SHAPES = [(9, 3, 33, 31),        # HW = 1023, PP = 4, segments of 4, 4 and 1 planes, a different head per plane
              (3, 7, 1, 1), (1, 2, 100, 101),
              (2, 5, 64, 64),        # HW == SEG
              (2, 3, 64, 65)]        # just over SEG
KINK_CAP = {"offset": 4e-3}
KINK_CAP_DEFAULT = 1e-4
DEAD_BETAS = (0.0, 0.3, -0.3)
FLAT_VALUES = (0.0, 1.5)

# worst |got - ref| / bound per tensor over everything `ratios` has seen in this process
WORST = {}
# the same per (family, tensor), for the calls that name their family
WORST_BY_FAMILY = {}


def gamma_n(n):
    return n * U32 / (1.0 - n * U32)


# ---------------------------------------------------------------------------------------------- geometry
def make_geo(N, C, HW):
    """The kernel's Geo as a dict: PP planes per segment (Q == 1) or Q pieces of L elements per plane, S segments."""
    if HW <= SEG:
        PP = min(SEG // HW, N)
        Q, L, S = 1, HW, (N + PP - 1) // PP
    else:
        PP = 1
        Q = (HW + SEG - 1) // SEG
        L = (((HW + Q - 1) // Q) + 3) & ~3
        S = N * Q
    return dict(N=N, C=C, HW=HW, PP=PP, Q=Q, L=L, S=S)


def seg_of(g, s):
    """(p0, p1, e0, e1): planes [p0, p1) and elements [e0, e1) of each that segment s owns."""
    if g["Q"] == 1:
        p0 = s * g["PP"]
        return p0, min(g["N"], p0 + g["PP"]), 0, g["HW"]
    p0 = s // g["Q"]
    e0 = min(g["HW"], (s % g["Q"]) * g["L"])
    return p0, p0 + 1, e0, min(g["HW"], e0 + g["L"])


def seg_count(g, s):
    p0, p1, e0, e1 = seg_of(g, s)
    return (p1 - p0) * (e1 - e0)


def plane_walk(g, c, s):
    """[(base, head, nv, tail)] per plane of segment s of channel c, as seg_walk splits it."""
    p0, p1, e0, e1 = seg_of(g, s)
    ln = e1 - e0
    out = []
    for p in range(p0, p1):
        base = (p * g["C"] + c) * g["HW"] + e0
        head = min((4 - (base & 3)) & 3, ln)
        nv = (ln - head) >> 2
        out.append((base, head, nv, ln - head - 4 * nv))
    return out


def ws_floats(N, C, HW):
    return C * make_geo(N, C, HW)["S"] * 3


def is_ragged(N, C, HW):
    """The last segment holds fewer planes than the others."""
    g = make_geo(N, C, HW)
    return g["Q"] == 1 and g["S"] > 1 and N % g["PP"] != 0


@functools.lru_cache(maxsize=None)
def _plan(N, C, HW, drop_tail=False):
    """idx (C, S, T, 256): the flat NCHW offset thread t adds at its step i of segment (c, s), or N C HW (a zero) for none."""
    g = make_geo(N, C, HW)
    S, pad = g["S"], N * C * HW
    rows = []
    T = 0
    for c in range(C):
        for s in range(S):
            steps = []
            for base, head, nv, tail in plane_walk(g, c, s):
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
                steps.append(blk)
            steps = torch.cat(steps)
            T = max(T, steps.shape[0])
            rows.append(steps)
    idx = torch.full((C * S, T, BLOCK), pad, dtype=torch.int64)
    for k, st in enumerate(rows):
        idx[k, :st.shape[0]] = st
    return idx.view(C, S, T, BLOCK)


@functools.lru_cache(maxsize=None)
def _segmap(N, C, HW):
    """(segid (N HW) of every element of a channel in (n, hw) order, cnt (S))."""
    g = make_geo(N, C, HW)
    segid = torch.empty(N, HW, dtype=torch.int64)
    for s in range(g["S"]):
        p0, p1, e0, e1 = seg_of(g, s)
        segid[p0:p1, e0:e1] = s
    cnt = torch.tensor([seg_count(g, s) for s in range(g["S"])], dtype=F64)
    return segid.reshape(-1), cnt


def depths(N, C, HW):
    """(D1, d_fold, d_chan) of the module docstring."""
    S = make_geo(N, C, HW)["S"]
    trips = (S + BLOCK - 1) // BLOCK
    return _plan(N, C, HW).shape[2] + 9, trips + 9, min(trips + 8, S - 1)


# ---------------------------------------------------------------------------------------------- inputs
def dead_channels(family, C, HW):
    """{channel: beta} of the gamma == 0 channels of `dead_channel`."""
    if family != "dead_channel":
        return {}
    return {c: DEAD_BETAS[(c // 2 + HW) % 3] for c in range(1, C, 2)}


def flat_channels(family, C):
    """{channel: constant} of the var == 0 channels of `flat_channel`."""
    if family != "flat_channel":
        return {}
    return {c: FLAT_VALUES[(c // 2) % 2] for c in range(1, C, 2)}


def make_inputs(family, shape, seed=0):
    """dict of CPU f32 tensors: x, gz, ggx (N, C, H, W), gg_gamma, gg_beta, gamma, beta, run_mean, run_var (C)."""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(100003 * seed + 7919 * FAMILIES.index(family) + 31 * N + 17 * C + 1009 * H + W)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    x = 0.7 + 1.3 * rn(*shape)
    gz, ggx = rn(*shape), rn(*shape)
    gg_gamma, gg_beta = rn(C), rn(C)
    gamma, beta = 1 + 0.3 * rn(C), 0.3 * rn(C)
    run_mean, run_var = 0.1 * rn(C), 1 + 0.1 * torch.rand(C, generator=gen)
    gamma[0] = -gamma[0].abs()                      # both signs of gamma in every family
    gamma[min(2, C - 1)] = gamma[min(2, C - 1)].abs()
    if family == "offset":
        x = 100 + 0.1 * rn(*shape)
    elif family == "mean_heavy":
        c1 = (0.5 + torch.rand(C, generator=gen)) * torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
        c2 = (0.5 + torch.rand(C, generator=gen)) * torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
        gz = c1.view(1, C, 1, 1) + 0.01 * rn(*shape)
        ggx = c2.view(1, C, 1, 1) + 0.01 * rn(*shape)
    elif family == "dead_channel":
        for c, b in dead_channels(family, C, H * W).items():
            gamma[c], beta[c] = 0.0, b
    elif family == "flat_channel":
        for c, v in flat_channels(family, C).items():
            x[:, c] = v
    elif family == "sparse_cotangent":
        gz[:N - 1] = 0.0
    return dict(x=x, gz=gz, ggx=ggx, gg_gamma=gg_gamma, gg_beta=gg_beta, gamma=gamma, beta=beta, run_mean=run_mean,
                run_var=run_var)


# ---------------------------------------------------------------------------------------------- reference
def reference(inp, family=None):
    """{name: fp64 reference, "bound_" + name: per-element bound} for name in TENSORS, {"alt_" + name, "bound_alt_" + name}
    for name in TWO_BRANCH (the other branch of s on the elements of K, the same values elsewhere), "kink": |K|."""
    x = inp["x"].to(F64)
    N, C, H, W = x.shape
    HW, n = H * W, N * H * W
    w, sl, mom = U32, SLOPE, MOMENTUM
    gam, bet = inp["gamma"].to(F64), inp["beta"].to(F64)
    gz, ggx = inp["gz"].to(F64), inp["ggx"].to(F64)
    ggg, ggb = inp["gg_gamma"].to(F64), inp["gg_beta"].to(F64)
    z, mu, r = spec.fwd(x, gam, bet, EPS, sl)
    gx, dgamma, dbeta = spec.bwd(gz, x, gam, bet, mu, r, sl)
    g_gz, g_x, g_gamma = spec.bwd_bwd(ggx, ggg, ggb, gz, x, gam, bet, mu, r, sl)
    M2u = ((x - mu.view(1, C, 1, 1)) ** 2).sum((0, 2, 3)) / (n - 1)
    R = dict(z=z, mean=mu, rstd=r, gx=gx, dgamma=dgamma, dbeta=dbeta, g_gz=g_gz, g_x=g_x, g_gamma=g_gamma,
             run_mean=(1 - mom) * inp["run_mean"].to(F64) + mom * mu, run_var=(1 - mom) * inp["run_var"].to(F64) + mom * M2u)

    # ---- bounds, on (C, n) views: a row per channel, per-channel values as (C, 1)
    cn = lambda t: t.permute(1, 0, 2, 3).reshape(C, n)  # noqa: E731
    back = lambda t: t.reshape(C, N, H, W).permute(1, 0, 2, 3).contiguous()  # noqa: E731
    col = lambda t: t.reshape(C, 1)  # noqa: E731
    tot = lambda t: t.sum(1, keepdim=True)  # noqa: E731
    X, GZ, Q = cn(x), cn(gz), cn(ggx)
    gam, bet, ggg, ggb, mu, r = col(gam), col(bet), col(ggg), col(ggb), col(mu), col(r)
    D1, d_fold, d_chan = depths(N, C, HW)
    D = D1 + d_fold
    segid, cnt = _segmap(N, C, HW)
    S = cnt.numel()
    segsum = lambda v: torch.zeros(C, S, dtype=F64).index_add_(1, segid, v)  # noqa: E731

    m_s = segsum(X) / cnt
    E_ms = gamma_n(D1 + 1) * segsum(X.abs()) / cnt
    mmax = m_s.abs().max(1, keepdim=True).values
    dm = m_s.max(1, keepdim=True).values - m_s.min(1, keepdim=True).values
    E_mu = tot(E_ms * cnt) / n + gamma_n(d_chan) * (mmax + 3 * dm)
    ds = X - m_s[:, segid]
    E_d = E_ms[:, segid] + w * ds.abs()
    dq = segsum(2 * ds.abs() * E_d + E_d * E_d)
    E_qs = tot(dq + gamma_n(D1 + 2) * (segsum(ds * ds) + dq))
    d = X - mu
    M2 = tot(d * d)
    var = M2 / n
    e = 2 * E_mu + w * dm
    E_M2 = E_qs + (dm * e + e * e / 2) * n * d_chan + gamma_n(2 * d_chan + 6) * (M2 + E_qs)
    E_var = E_M2 / n + w * var
    delta = E_var / (var + EPS)
    rho = torch.where(delta < 0.9, delta / (2 * (1 - delta.clamp(max=0.9))) + 4 * w, torch.full_like(delta, float("inf")))
    unb = M2 / (n - 1)
    B = {"mean": E_mu, "rstd": r * rho,
         "run_mean": mom * E_mu + gamma_n(4) * (((1 - mom) * col(inp["run_mean"].to(F64))).abs() + (mom * mu).abs()),
         "run_var": mom * (E_M2 / (n - 1) + w * unb) + gamma_n(4) * (((1 - mom) * col(inp["run_var"].to(F64))).abs() + mom * unb)}

    rs = rho + w * (1 + rho)
    gr = gam.abs() * r
    xh = d * r
    y = gam * xh + bet
    pos = y > 0
    E_y = gr * (d.abs() * rs + (1 + rs) * E_mu) + w * (1 + rs) * (X.abs() + mu.abs()) * gr + 2 * w * y.abs()
    K = (y.abs() <= E_y) & (E_y > 0)
    nk = int(K.sum())
    cap = KINK_CAP.get(family, KINK_CAP_DEFAULT)
    assert nk <= cap * X.numel(), f"{nk} of {X.numel()} elements within E_y of the kink (cap {cap})"
    Z = cn(z)
    B["z"] = torch.where(K, 2 * E_y + 2 * w * Z.abs(), torch.where(pos, E_y, sl * E_y + 2 * w * Z.abs()))

    E_xh = r * (1 + rho) * E_mu + xh.abs() * (rho + 2 * w)
    Kf = K.to(F64)
    kink = lambda term: (1 - sl) * tot(Kf * term)  # noqa: E731
    s_main = torch.where(pos, torch.ones_like(y), torch.full_like(y, sl))
    s_alt = torch.where(K, 1 + sl - s_main, s_main)
    A, Bm = col(dbeta) / n, col(dgamma) / n
    Cm, Dm, Em = tot(Q) / n, tot(Q * xh) / n, tot(Q * s_main * GZ) / n
    gy0 = s_main * GZ
    E_gy0 = w * gy0.abs()
    E_Sgy = tot(E_gy0) + gamma_n(D) * (tot(gy0.abs()) + tot(E_gy0)) + kink(GZ.abs())
    t0 = tot(gy0.abs() * E_xh + E_gy0 * xh.abs())
    E_Sgyx = t0 + gamma_n(D + 1) * (tot((gy0 * xh).abs()) + t0) + kink(GZ.abs() * (xh.abs() + E_xh))
    B["dbeta"], B["dgamma"] = E_Sgy, E_Sgyx
    E_A, E_B = E_Sgy / n + 2 * w * A.abs(), E_Sgyx / n + 2 * w * Bm.abs()
    E_C = gamma_n(D) * tot(Q.abs()) / n + 2 * w * Cm.abs()
    t0 = tot(Q.abs() * E_xh)
    E_D = (t0 + gamma_n(D + 1) * (tot((Q * xh).abs()) + t0)) / n + 2 * w * Dm.abs()
    t0 = tot(Q.abs() * E_gy0)
    E_E = (t0 + gamma_n(D + 1) * (tot((Q * gy0).abs()) + t0) + kink((Q * GZ).abs())) / n + 2 * w * Em.abs()
    P = lambda k: (E_E + A.abs() * E_C + Cm.abs() * E_A + E_A * E_C  # noqa: E731
                   + k * (Bm.abs() * E_D + Dm.abs() * E_B + E_B * E_D))
    AC, BD = (A * Cm).abs(), (Bm * Dm).abs()
    E_T = P(1) + gamma_n(3) * (Em.abs() + AC + BD)
    E_k1 = P(3) + gamma_n(4) * (Em.abs() + AC + 3 * BD)
    k1 = Em - A * Cm - 3 * Bm * Dm
    B["g_gamma"] = n * r * (1 + rho) * E_T + col(g_gamma).abs() * (rho + 3 * w)
    q = Q - Cm
    E_q = E_C + w * q.abs()
    J = q - xh * Dm
    E_J = E_q + Dm.abs() * E_xh + xh.abs() * E_D + E_xh * E_D + w * ((xh * Dm).abs() + J.abs())
    t1, t2 = gam * r * J, ggg * xh
    E_t1 = gr * (1 + rs) * E_J + t1.abs() * (rs + w)
    E_t2 = ggg.abs() * E_xh + w * t2.abs()
    t = t1 + t2 + ggb
    E_t = E_t1 + E_t2 + w * (t1.abs() + t2.abs()) + 2 * w * t.abs()
    r2 = (1 + rs) * (1 + rho) * (1 + w) - 1

    def branch(s):
        gy = s * GZ
        E_gy = w * gy.abs()
        I = gy - A - xh * Bm  # noqa: E741
        E_I = E_gy + E_A + xh.abs() * E_B + Bm.abs() * E_xh + E_xh * E_B + w * (gy.abs() + A.abs() + (xh * Bm).abs() + I.abs())
        vgx = gam * r * I
        b_gx = gr * (1 + rs) * E_I + vgx.abs() * (rs + 2 * w)
        vgg = s * t
        b_gg = torch.where(s == 1, E_t, sl * E_t + 2 * w * vgg.abs())
        u1 = ggg * r * I
        E_u1 = ggg.abs() * r * (1 + rho + w) * E_I + u1.abs() * (rho + 2 * w)
        G = gy - A
        E_G = E_gy + E_A + w * G.abs()
        V = xh * k1 + Bm * q + Dm * G
        E_V = (k1.abs() * E_xh + xh.abs() * E_k1 + E_xh * E_k1 + Bm.abs() * E_q + q.abs() * E_B + E_q * E_B
               + Dm.abs() * E_G + G.abs() * E_D + E_G * E_D + gamma_n(3) * ((xh * k1).abs() + (Bm * q).abs() + (Dm * G).abs()))
        u2 = gam * r * r * V
        E_u2 = gr * r * (1 + r2) * E_V + u2.abs() * (r2 + w)
        return {"gx": (vgx, b_gx), "g_gz": (vgg, b_gg), "g_x": (u1 - u2, E_u1 + E_u2 + 2 * w * (u1.abs() + u2.abs()))}

    main, alt = branch(s_main), branch(s_alt)
    for name in TWO_BRANCH:
        B[name] = main[name][1]
        R["alt_" + name] = back(torch.where(K, alt[name][0], cn(R[name])))
        B["alt_" + name] = alt[name][1]
    for name, b in B.items():
        base = name[4:] if name.startswith("alt_") else name
        ref = R[base]
        floor = FLOOR * float(ref.abs().max()) if ref.numel() else 0.0
        b = b * SLACK + floor
        R["bound_" + name] = back(b) if ref.dim() == 4 else b.reshape(C)
    R["kink"] = nk
    return R


def ratios(got, R, names=TENSORS, record=True, family=None):
    """{name: worst |got - ref| / bound}; for gx, g_gz and g_x the nearer of the two branches of s per element; a
    non-finite value counts as inf."""
    out = {}
    for name in names:
        v = got[name].detach().to(F64).cpu().reshape(R[name].shape)
        q = (v - R[name]).abs() / R["bound_" + name]
        if name in TWO_BRANCH:
            q = torch.minimum(q, (v - R["alt_" + name]).abs() / R["bound_alt_" + name])
        q = torch.where(torch.isfinite(v), q, torch.full_like(q, float("inf")))
        out[name] = float(q.max()) if q.numel() else 0.0
        if record:
            WORST[name] = max(WORST.get(name, 0.0), out[name])
            if family is not None:
                WORST_BY_FAMILY[(family, name)] = max(WORST_BY_FAMILY.get((family, name), 0.0), out[name])
    return out


# ---------------------------------------------------------------------------------------------- CPU emulation
_LANES = torch.arange(64)


def _block_sum(acc):
    """(..., 256) per-thread values -> (...): butterfly xor 32 ... 1 inside each wave, lane 0, the waves in order."""
    s = acc.reshape(*acc.shape[:-1], WAVES, 64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., _LANES ^ o]
    out = s[..., 0, 0]
    for k in range(1, WAVES):
        out = out + s[..., k, 0]
    return out


def _seg_sum(v, idx):
    """(C, S) per-segment sums of the (N, C, H, W) f32 tensor v in the kernel's order."""
    flat = torch.cat([v.reshape(-1), torch.zeros(1, dtype=F32)])
    acc = torch.zeros(idx.shape[0], idx.shape[1], BLOCK, dtype=F32)
    for i in range(idx.shape[2]):
        acc = acc + flat[idx[:, :, i]]
    return _block_sum(acc)


def _by_thread(part, limit):
    """(C, S) -> (C, trips, 256), zero-padded; `limit` keeps only the first `limit` partials."""
    C, S = part.shape
    if limit is not None and S > limit:
        part, S = part[:, :limit], limit
    trips = (S + BLOCK - 1) // BLOCK
    pad = torch.zeros(C, trips * BLOCK, dtype=part.dtype)
    pad[:, :S] = part
    return pad.view(C, trips, BLOCK)


def _fold_sums(part, limit=None):
    p = _by_thread(part, limit)
    acc = torch.zeros(p.shape[0], BLOCK, dtype=F32)
    for j in range(p.shape[1]):
        acc = acc + p[:, j]
    return _block_sum(acc)


def _chan(a, b, cross=True):
    """Chan's merge of (count, mean, M2) triples stacked on the last axis, as the kernel's struct Chan."""
    a0, a1, a2 = a.unbind(-1)
    b0, b1, b2 = b.unbind(-1)
    nn = a0 + b0
    f = b0 / torch.where(nn == 0, torch.ones_like(nn), nn)
    d = b1 - a1
    m2 = a2 + (b2 + d * d * a0 * f) if cross else a2 + b2
    new = torch.stack([nn, a1 + d * f, m2], -1)
    return torch.where((b0 == 0)[..., None], a, torch.where((a0 == 0)[..., None], b, new))


def _chan_fold(cnt, mean, m2, limit=None, cross=True):
    """(C, 3): the fold of fwd_apply_kernel over the S partials."""
    C = mean.shape[0]
    tri = torch.stack([_by_thread(cnt.expand(C, -1).contiguous(), limit), _by_thread(mean, limit), _by_thread(m2, limit)], -1)
    a = torch.zeros(C, BLOCK, 3, dtype=F32)
    for j in range(tri.shape[1]):
        a = _chan(a, tri[:, j], cross)
    a = a.view(C, WAVES, 64, 3)
    for o in (32, 16, 8, 4, 2, 1):
        a = _chan(a, a[:, :, _LANES ^ o], cross)
    out = a[:, 0, 0]
    for k in range(1, WAVES):
        out = _chan(out, a[:, k, 0], cross)
    return out


def _fmaf(a, b, c):
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def emulate(inp, mut=None):
    """{name: f32 tensor for name in TENSORS} on the CPU: f32 torch ops in the kernels' order.  mut plants a defect:
    "tail_dropped", "chan_no_cross_term", "biased_running_var", "uncentred_variance", "sign_from_xhat",
    "g_gz_without_slope", "k1_with_2BD", "fold_first_256_only", "last_segment_dropped"."""
    x, gz, ggx = inp["x"].to(F32), inp["gz"].to(F32), inp["ggx"].to(F32)
    N, C, H, W = x.shape
    HW = H * W
    g = make_geo(N, C, HW)
    S = g["S"]
    idx = _plan(N, C, HW, mut == "tail_dropped")
    segid, cnt64 = _segmap(N, C, HW)
    cnt = cnt64.to(F32)
    limit = BLOCK if mut == "fold_first_256_only" else None
    ch = lambda t: t.view(1, C, 1, 1)  # noqa: E731
    f = lambda v: torch.tensor(v, dtype=F32)  # noqa: E731
    eps, mom, sl = f(EPS), f(MOMENTUM), f(SLOPE)
    gamma, beta = inp["gamma"].to(F32), inp["beta"].to(F32)

    # forward: stats_kernel, then the fold of fwd_apply_kernel
    if mut == "uncentred_variance":
        nf = f(float(N * HW))
        mu = _fold_sums(_seg_sum(x, idx), limit) / nf
        m2 = (_fold_sums(_seg_sum(x * x, idx), limit) / nf - mu * mu) * nf
    else:
        seg_mean = _seg_sum(x, idx) / cnt
        dd = x - seg_mean[:, segid].view(C, N, H, W).permute(1, 0, 2, 3)
        q = _seg_sum(dd * dd, idx)
        fold_cnt = cnt.clone()
        if mut == "last_segment_dropped" and S > 1:
            fold_cnt[S - 1] = 0.0
        a = _chan_fold(fold_cnt, seg_mean, q, limit, mut != "chan_no_cross_term")
        nf, mu, m2 = a[:, 0], a[:, 1], a[:, 2]
    var = m2 / nf
    r = torch.rsqrt(var + eps)
    scale = gamma * r
    shift = beta - mu * scale
    run_mean = (1 - mom) * inp["run_mean"].to(F32) + mom * mu
    run_var = (1 - mom) * inp["run_var"].to(F32) + mom * (var if mut == "biased_running_var" else m2 / (nf - 1))
    y = _fmaf(x, ch(scale), ch(shift))
    z = torch.where(y > 0, y, sl * y)

    # backward: bwd_reduce_kernel, fold_sums, bwd_apply_kernel
    xh = (x - ch(mu)) * ch(r)
    pos = (ch(gamma) * xh > 0) if mut == "sign_from_xhat" else (y > 0)
    gy = torch.where(pos, gz, sl * gz)
    sgy = _fold_sums(_seg_sum(gy, idx), limit)
    sgyx = _fold_sums(_seg_sum(gy * xh, idx), limit)
    inv_n = f(1.0) / f(float(N * HW))
    A, B = ch(sgy * inv_n), ch(sgyx * inv_n)
    gx = ch(scale) * (gy - A - xh * B)

    # double backward: bwd_bwd_reduce_kernel, fold_sums, bwd_bwd_apply_kernel
    n32 = f(float(N * HW))
    Cc = _fold_sums(_seg_sum(ggx, idx), limit) * inv_n
    Dd = _fold_sums(_seg_sum(ggx * xh, idx), limit) * inv_n
    Ee = _fold_sums(_seg_sum(ggx * gy, idx), limit) * inv_n
    a1, b1 = sgy * inv_n, sgyx * inv_n
    g_gamma = n32 * r * (Ee - a1 * Cc - b1 * Dd)
    k1 = Ee - a1 * Cc - (2.0 if mut == "k1_with_2BD" else 3.0) * b1 * Dd
    gr2 = scale * r
    ggg, ggb = inp["gg_gamma"].to(F32), inp["gg_beta"].to(F32)
    gr = ggg * r
    qq = ggx - ch(Cc)
    t = ch(scale) * (qq - xh * ch(Dd)) + ch(ggg) * xh + ch(ggb)
    g_gz = t if mut == "g_gz_without_slope" else torch.where(pos, t, sl * t)
    g_x = ch(gr) * (gy - A - xh * B) - ch(gr2) * (xh * ch(k1) + B * qq + ch(Dd) * (gy - A))
    return dict(z=z, mean=mu, rstd=r, run_mean=run_mean, run_var=run_var, gx=gx, dgamma=sgyx, dbeta=sgy, g_gz=g_gz, g_x=g_x,
                g_gamma=g_gamma)
