"""fp64 reference, index licence, per-element bounds, input families and planted cases for csrc/vq.hip: the codebook
nearest-neighbour lookup (amk_vq_lookup_fwd), its backward (amk_vq_lookup_bwd / _bwd_rows) and amk_vq_gather.

Rules, as in tests/bf16_dense_ref.py and tests/row_f32_ref.py: the reference is fp64 on the f32 inputs; every rounded
f32 operation costs u = 2^-24 of its result, to first order; a sum of n terms costs n u sum|t| with n read off the
source; no term is relative to a tensor's maximum; every element is checked.  sqrtf and `/` are correctly rounded
(csrc/Makefile: -O3, no fast-math; see row_f32_ref.py).  hipcc may contract a * b + c: an FMA drops a rounding, so the
bounds hold for either form.  L = log2(C / 4) is the depth of a row's shuffle tree over its C / 4 lanes.

Reference (vq.hip:7-24).  zn = z / max(|z|, eps), en = E / max(|E_k|, eps), eps = 1e-12f,
    score[n, k] = <zn, en_k> - |en_k|^2 / 2,        idx[n] = first argmax_k score[n, k],
    zq = en[idx], out = zn + (zq - zn), mean_sq = sum (zq - zn)^2 / (N C)   (ops: loss = beta mean_sq + mean_sq).

Normalisations.
* zn (vq.hip:92-106): a half-wave sums C/2 squares, 4 at a time into a running sum (a square, 3 adds, C/8
  accumulations), one shuffle add: ss carries (C/8 + 5) u; sqrtf halves that and adds u: eps_zd = (C/16 + 3.5) u is
  the relative error of the row's denominator, COMMON to the row; the division adds u per element:
      bound_zn = (eps_zd + u) |zn|.     Under the clamp zn = z / eps: one rounding, inside the same bound.
* en (vq.hip:49-53), zq (vq.hip:291-295), gather (vq.hip:430-434): 4 squares and 3 adds in the lane, L shuffle adds:
  ss carries (4 + L) u, the denominator eps_ed = (3 + L / 2) u, common to the code:  bound_zq = (eps_ed + u) |zq|.
* ee (vq.hip:54-56) = sum en^2 on the f32 en: 2 (eps_ed + u) from en, (4 + L) u from the sum.

Index licence: tau(n; a, b), the f32 error of score_a - score_b as the kernel forms it.
* inputs.  The row's denominator scales every dot product alike: eps_zd |dot_a - dot_b|.  The row's divisions:
  u sum_c |zn_c| |en_ac - en_bc|.  Per code k: its denominator eps_ed |dot_k|, its divisions u A_k with
  A_k = sum_c |zn_c en_kc|, and ee_k / 2 ((2 eps_ed + 2 u) + (4 + L) u).
* the sweep (vq.hip:182-190): the accumulator starts at -ee_k / 2 and takes C / 2 steps of v_mfma_f32_32x32x2_f32,
  step s adding the products of channels s and C / 2 + s (the two half-waves).  How the instruction rounds inside a step
  is not documented: two roundings per step, each of a magnitude of at most |p_{s-1}| + |t_s| + |t'_s|, p the fp64
  partial sums in that order:   e_mfma(k) = 2 u sum_s (|p_{s-1}| + |t_s| + |t'_s|).
  This is the "n u sum|t|" rule with the partial sums the chain really passes through: on a clustered codebook the
  winner's chain climbs from -1/2 to +1/2 and never holds the sum|t| + 1/2 = 3/2 the plain rule charges C + 1 times.
* the winning group (vq.hip:281-289): the 4 codes of the group are ranked by a VALU dot: 4 products, 3 adds, L shuffle
  adds, the subtraction of 0.5 ee:   e_valu(k) = (5 + L) u (A_k + ee_k / 2).
* chain: the kernel's idx wins the VALU ranking in its group g against the group's MFMA maximum a, and a's group
  beat the group of the fp64 argmax m in the sweep:
      tau(n; idx, m) = inputs(idx, m) + e_valu(idx) + max_{k in g} e_valu(k) + max_{k in g} e_mfma(k) + e_mfma(m).
  Every row must satisfy score[n, idx] >= score[n, m] - tau(n; idx, m): no row is exempt.
* tau_row(n), independent of the kernel's answer: tau_loose(n) is the same sum with every per-code term at its maximum
  over the codebook and e_mfma at C u (ee / 2 + A); a code is plausible when score_m - score_k <= tau_loose.
  tau_row = the maximum of tau(n; k, m) over the plausible codes among ranks 2 .. 4, or tau_loose when rank 5 is
  plausible as well.  (An idx != m the licence admits is plausible, so tau_row >= score_m - score_idx >= the margin.)
  A row whose fp64 top-two margin exceeds tau_row must equal the fp64 argmax exactly; at most MAX_LICENSED = 10 % of
  the rows of any family and case may have a margin <= tau_row (asserted on the CPU, from the reference alone).

Other outputs, against the reference evaluated AT THE KERNEL'S INDEX (a licensed near-tie does not contaminate them):
    out = zn + (zq - zn) (vq.hip:296-298), both times the same f32 zn, whose own error therefore cancels:
        bound_out = bound_zq + u (|zq - zn| + bound_zn + bound_zq) + u |zq|     (the subtraction, which rounds the f32
        difference, and the addition)
    mean_sq: d = zq - zn carries dd = bound_zn + bound_zq + u |d|; the sum of squares runs over 4 in the lane, L
    shuffles, the 16 rows of a workgroup (vq.hip:300-310) and the P partials (torch.sum):
        bound = (sum 2 |d| dd + (6 + L + 16 + P) u sum d^2) / (N C) + 2 u mean_sq.

Backward (vq.hip:316-410), reference: fp64 derivative of the formulas above at the kernel's index, clamp form of
F.normalize (Jacobian (I - y y^T) / |x| above the clamp, I / eps below it), written out analytically because autograd
gives NaN for the norm of a zero row (the CPU test compares it with fp64 autograd on the other rows).
    coef = g_loss 2 / float(N C): 3 u.   d = zn - zq: dd as above (the kernel reads the forward's f32 zn and zq).
    dzn = go + (coef beta) d:  E_z = |coef beta| dd + 5 u |coef beta d| + u |dzn|
    dzq = coef (-d):           E_q = |coef| dd + 4 u |dzq|
    pz = sum_c zn dzn (a product, up to 3 adds in the lane, the shuffle tree: n_p = 5 + log2 C covers both kernels):
        dpz = sum (bound_zn |dzn| + |zn| E_z) + n_p u sum |zn dzn|
    |z| = sqrtf(sum z^2): eps_n = (n_p / 2 + 1) u
    gz = (dzn - zn pz) / |z|:  dv = E_z + bound_zn |pz| + |zn| dpz + 2 u |zn pz| + u |v|,   bound_dz = dv / |z| + |gz| (eps_n + u)
    under the clamp gz = dzn / eps:  E_z / eps + u |gz|.        ge likewise from zq, dzq and |E_idx|.
    dE[k] = sum of ge over the rows that chose k: bound = sum_rows bound_ge + (rows(k) + 1) u sum_rows |ge|, whatever
    the order (so it covers the atomics and the ordered sum of ops alike); a code no row chose is exactly zero.

Range.  The families stay where the f32 sum of squares neither overflows nor underflows: the sum of squares of a row or
a code lies between 1e-29 and 1e9, or is exactly zero (single elements may be smaller; what their squares lose is far below
u of the sum).  tiny_norm rows have norms of 1e-14 .. 3e-13, well below eps = 1e-12, so sqrtf(ss) <= eps on both
sides whatever the rounding.
"""
import math

import torch

import bf16_dense_ref as bf
from bf16_dense_ref import U32, _d, _gen, assert_within, ratios  # noqa: F401

WORST = bf.WORST
F32, F64 = torch.float32, torch.float64
EPS = float(torch.tensor(1e-12, dtype=F32))   # the f32 eps of the kernels, as a double
CS = (32, 64, 128, 256)
CODES_LDS = {32: 128, 64: 128, 128: 64, 256: 32}
FIN_ROWS = 16
MAX_LICENSED = 0.10
FAMILIES = ("gaussian", "clustered", "scaled", "tiny_norm")
SIGMA = 1e-2
NS = (1, 15, 16, 17, 127, 128, 129, 257)
NSPLITS_INVARIANT = (1, 2, 4, 16, 32)
# (K, nsplit) per C: the smallest that reach each branch (full and partial LDS tiles, one and several tiles per slice,
# the non-pipelined branch with several slices, slices of padding only, 16 slices and the loop beyond 16)
CASES = {
    32: [(128, 1), (96, 1), (160, 1), (416, 1), (1, 1), (5, 2), (40, 4), (320, 2), (500, 4), (512, 4), (512, 16), (768, 24),
         (1024, 32)],
    64: [(128, 1), (200, 1), (512, 16), (640, 20)],
    128: [(64, 1), (96, 1), (160, 2), (77, 1), (544, 17)],
    256: [(32, 1), (33, 1), (64, 2), (100, 3), (640, 20)],
}
ALL_CASES = [(C, K, ns) for C in CS for K, ns in CASES[C]]


def padded_codes(K, nsplit):
    q = 32 * nsplit
    return -(-K // q) * q


def num_partials(N):
    return -(-N // FIN_ROWS)


def position(C, K, nsplit, k):
    """Where code k sits in the sweep: (slice, LDS tile, sub-tile, half-wave, group of the half-wave, place in the group)."""
    kper = padded_codes(K, nsplit) // nsplit
    r = k % kper
    w = r % 32
    return (k // kper, r // CODES_LDS[C], (r % CODES_LDS[C]) // 32, (w % 8) // 4, w // 8, w % 4)


# ---------------------------------------------------------------------------------------------- families
def make_fwd(family, N, K, C, seed):
    """z (N, C), E (K, C): f32."""
    g = _gen(seed)
    z, E = torch.randn(N, C, generator=g), torch.randn(K, C, generator=g)
    if family == "clustered":
        cen = torch.nn.functional.normalize(torch.randn(16, C, generator=g), dim=1)
        z = cen[torch.randint(0, 16, (N,), generator=g)] + SIGMA * z
        E = cen[torch.randint(0, 16, (K,), generator=g)] + SIGMA * E
    elif family == "scaled":
        z = z * torch.where(torch.arange(N) % 2 == 0, 1e-3, 1e3).view(N, 1)
        E = E * torch.where(torch.arange(K) % 3 == 0, 1e3, 1e-3).view(K, 1)
    elif family == "tiny_norm":
        z[::3] *= 1e-14 / math.sqrt(C)
        E[1::4] *= 3e-14 / math.sqrt(C)
        z[N // 2] = 0.0
        E[K // 2] = 0.0
    return z, E


def make_planted(C, K, seed):
    """Row n = 1.5 E[n]: every code wins once, by an fp64 margin far above tau (asserted on the CPU)."""
    E = torch.randn(K, C, generator=_gen(seed))
    return 1.5 * E, E, torch.arange(K)


TIE_KINDS = ("group", "groups", "halves", "subtiles", "tiles", "slices", "three")


def _tie_kind(pa, pb):
    if pa[0] != pb[0]:
        return "slices"
    if pa[1] != pb[1]:
        return "tiles"
    if pa[2] != pb[2]:
        return "subtiles"
    if pa[3] != pb[3]:
        return "halves" if pa[4] == pb[4] else None
    if pa[4] != pb[4]:
        return "groups"
    return "group"


def tie_candidates(C, K, nsplit):
    """{kind: [(i, j)]}: every pair i < j of code positions at a distance in {1, 2, 3, 4, 8, 16, 24, 32, 64, 96,
    CODES_LDS, 2 CODES_LDS, kper, 2 kper, (nsplit - 1) kper}, by the kind of the pair, in ascending order."""
    kper = padded_codes(K, nsplit) // nsplit
    steps = sorted({1, 2, 3, 4, 8, 16, 24, 32, 64, 96, CODES_LDS[C], 2 * CODES_LDS[C], kper, 2 * kper, (nsplit - 1) * kper})
    found = {}
    for i in range(K):
        for d in steps:
            j = i + d
            if d <= 0 or j >= K:
                continue
            kind = _tie_kind(position(C, K, nsplit, i), position(C, K, nsplit, j))
            if kind:
                found.setdefault(kind, []).append((i, j))
    return found


def make_ties(C, K, nsplit, seed):
    """z, E, expected index, kinds: for every kind of pair the case holds, the first and the last candidate pair whose
    positions are still free get a code row of their own, copied to the later position, and a z row pointing at it
    (1.5 times the code); 'three': a pair of the finest kind plus a copy at a pair of the coarsest kind.  Copies never
    overlap.  The first index must win: known by construction."""
    E = torch.randn(K, C, generator=_gen(seed))
    cand = tie_candidates(C, K, nsplit)
    used, rows, kinds = set(), [], []

    def plant(t, kind):
        used.update(t)
        for j in t[1:]:
            E[j] = E[t[0]]
        rows.append(t[0])
        kinds.append(kind)

    for kind in TIE_KINDS[:-1]:
        for order in (cand.get(kind, []), reversed(cand.get(kind, []))):
            t = next((t for t in order if not used & set(t)), None)
            if t:
                plant(t, kind)
    have = [k for k in TIE_KINDS[:-1] if k in cand]
    if len(have) >= 2:
        far = {i: j for i, j in cand[have[-1]] if j not in used}
        t = next(((i, j, far[i]) for i, j in cand[have[0]] if i in far and far[i] > j and not used & {i, j, far[i]}), None)
        if t:
            plant(t, "three")
    if not rows:
        return None
    return 1.5 * E[rows], E, torch.tensor(rows), kinds


# ---------------------------------------------------------------------------------------------- forward reference
def _l(C):
    return math.log2(C // 4)


def ref_scores(z, E):
    """The fp64 reference up to the scores, with what the licence needs."""
    Z, Ed = _d(z), _d(E)
    zn = Z / Z.norm(dim=1, keepdim=True).clamp_min(EPS)
    en = Ed / Ed.norm(dim=1, keepdim=True).clamp_min(EPS)
    ee = (en * en).sum(1)
    dot = zn @ en.T
    score = dot - ee / 2
    K = E.shape[0]
    top = torch.topk(score, min(5, K), dim=1)
    # (first index among exactly equal fp64 scores: the planted ties; topk does not promise an order among them)
    arg = (score == top.values[:, :1]).to(torch.uint8).argmax(1)
    return dict(zn=zn, en=en, ee=ee, dot=dot, score=score, A=zn.abs() @ en.abs().T, argmax=arg, top=top, C=z.shape[1], K=K,
                N=z.shape[0], Z=Z, E=Ed)


def _per_code(R, k):
    """(inputs, e_valu, e_mfma) of code k[n] for row n: the errors of one score that do not cancel between codes."""
    C, L = R["C"], _l(R["C"])
    n = torch.arange(R["N"])
    dot, A, ee = R["dot"][n, k].abs(), R["A"][n, k], R["ee"][k]
    eps_ed = (3 + L / 2) * U32
    e_in = eps_ed * dot + U32 * A + ee / 2 * (2 * eps_ed + 2 * U32 + (4 + L) * U32)
    e_valu = (5 + L) * U32 * (A + ee / 2)
    t = R["zn"] * R["en"][k]
    t1, t2 = t[:, : C // 2], t[:, C // 2:]
    p = (-ee / 2).view(-1, 1) + torch.cumsum(t1 + t2, 1)
    p_prev = torch.cat([(-ee / 2).view(-1, 1), p[:, :-1]], 1)
    e_mfma = 2 * U32 * (p_prev.abs() + t1.abs() + t2.abs()).sum(1)
    return e_in, e_valu, e_mfma


def tau_pair(R, idx, m):
    """tau(n; idx[n], m[n]) of the module docstring."""
    C = R["C"]
    n = torch.arange(R["N"])
    eps_zd = (C / 16 + 3.5) * U32
    common = eps_zd * (R["dot"][n, idx] - R["dot"][n, m]).abs() + U32 * (R["zn"].abs() * (R["en"][idx] - R["en"][m]).abs()).sum(1)
    in_i, valu_i, _ = _per_code(R, idx)
    in_m, _, mfma_m = _per_code(R, m)
    gv = torch.zeros(R["N"], dtype=F64)
    gm = torch.zeros(R["N"], dtype=F64)
    for j in range(4):
        k = (idx // 4 * 4 + j).clamp_max(R["K"] - 1)
        _, v, mf = _per_code(R, k)
        gv, gm = torch.maximum(gv, v), torch.maximum(gm, mf)
    return common + in_i + in_m + valu_i + gv + gm + mfma_m


def tau_loose(R):
    C, L = R["C"], _l(R["C"])
    eps_zd, eps_ed = (C / 16 + 3.5) * U32, (3 + L / 2) * U32
    dot, A, ee = R["dot"].abs(), R["A"], R["ee"].view(1, -1)
    per = eps_ed * dot + U32 * A + ee / 2 * (2 * eps_ed + 2 * U32 + (4 + L) * U32) + (5 + L) * U32 * (A + ee / 2) \
        + C * U32 * (ee / 2 + A)
    return 2 * eps_zd * dot.max(1).values + 2 * U32 * A.max(1).values + 2 * per.max(1).values


def tau_row(R):
    """(tau_row, margin): see the module docstring.  K = 1 has no second code: margin inf."""
    loose = tau_loose(R)
    vals, ids = R["top"].values, R["top"].indices
    N, J = vals.shape
    if J == 1:
        return loose, torch.full((N,), math.inf, dtype=F64)
    m = R["argmax"]
    margin = vals[:, 0] - vals[:, 1]
    tau = torch.zeros(N, dtype=F64)
    for j in range(1, min(J, 4)):
        k = torch.where(ids[:, j] == m, ids[:, 0], ids[:, j])     # (exact ties: topk's order against the first index)
        t = tau_pair(R, k, m)
        assert bool((t <= loose * (1 + 1e-12)).all())
        tau = torch.where((vals[:, 0] - vals[:, j] <= loose) | (j == 1), torch.maximum(tau, t), tau)
    if J == 5:
        tau = torch.where(vals[:, 0] - vals[:, 4] <= loose, loose, tau)
    return tau, margin


def ref_outputs(R, idx):
    """zn, zq, out, mean_sq at the index `idx` (the kernel's own) with their bounds."""
    C, L, N = R["C"], _l(R["C"]), R["N"]
    zn, zq = R["zn"], R["en"][idx]
    bzn = ((C / 16 + 3.5) * U32 + U32) * zn.abs()
    bzq = ((3 + L / 2) * U32 + U32) * zq.abs()
    d = zq - zn
    dd = bzn + bzq + U32 * d.abs()
    P = num_partials(N)
    ms = (d * d).sum() / (N * C)
    bms = ((2 * d.abs() * dd).sum() + (6 + L + 16 + P) * U32 * (d * d).sum()) / (N * C) + 2 * U32 * ms
    return {"zn": zn, "bound_zn": bzn, "zq": zq, "bound_zq": bzq, "out": zq.clone(),
            "bound_out": bzq + U32 * (d.abs() + bzn + bzq) + U32 * zq.abs(),
            "mean_sq": ms.view(1), "bound_mean_sq": bms.view(1)}


FWD_OUT = ("zn", "zq", "out", "mean_sq")


def check_indices(R, idx, what=""):
    """The licence, for every row; exact equality where the margin exceeds tau_row.  Returns (rows licensed, worst
    (score_m - score_idx) / tau over the rows that differ)."""
    idx = idx.detach().cpu().long()
    assert bool(((idx >= 0) & (idx < R["K"])).all()), f"{what}: index outside the codebook"
    n = torch.arange(R["N"])
    m = R["argmax"]
    gap = R["score"][n, m] - R["score"][n, idx]
    tau = tau_pair(R, idx, m)
    bad = ~(gap <= tau)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} rows outside the licence, first {int(n[bad][0])}: " \
        f"idx {int(idx[bad][0])} argmax {int(m[bad][0])} gap {float(gap[bad][0]):.3g} tau {float(tau[bad][0]):.3g}"
    trow, margin = tau_row(R)
    must = margin > trow
    wrong = must & (idx != m)
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} rows with a margin above tau differ from the fp64 argmax"
    diff = idx != m
    worst = float((gap[diff] / tau[diff]).max()) if bool(diff.any()) else 0.0
    WORST["vq.licence"] = max(WORST.get("vq.licence", 0.0), worst)
    return int(diff.sum()), worst


def emulate_fwd(z, E):
    """The forward in f32 on the CPU (torch's summation order, not the kernel's): idx, zn, zq, out, mean_sq."""
    eps = torch.tensor(1e-12, dtype=F32)
    zn = z / torch.maximum(torch.sqrt((z * z).sum(1, keepdim=True)), eps)
    en = E / torch.maximum(torch.sqrt((E * E).sum(1, keepdim=True)), eps)
    score = zn @ en.T - 0.5 * (en * en).sum(1)
    idx = score.argmax(1)
    zq = en[idx]
    d = zq - zn
    return {"idx": idx, "zn": zn, "zq": zq, "out": zn + d, "mean_sq": ((d * d).sum() / (z.numel())).view(1)}


# ---------------------------------------------------------------------------------------------- backward
BWD_NK = [(1, 1), (7, 5), (129, 64), (1000, 1000), (129, 1), (1000, 5), (7, 1000)]
BWD_MODES = ("random", "one_code", "zero_row", "zero_code", "g_loss0", "g_out0", "binade")
BETAS = (0.0, 0.25, 1.0)


def make_bwd(mode, N, K, C, seed):
    """z, E, idx (int64), g_out (N, C), g_loss (scalar tensor): f32 inputs of the backward."""
    g = _gen(seed)
    z, E = torch.randn(N, C, generator=g), torch.randn(K, C, generator=g)
    idx = torch.randint(0, K, (N,), generator=g)
    go = torch.randn(N, C, generator=g)
    gl = torch.tensor(0.7)
    if mode == "one_code":
        idx[:] = K - 1
    elif mode == "zero_row":
        z[N // 2] = 0.0
        z[0] *= 1e-14 / math.sqrt(C)
    elif mode == "zero_code":
        E[int(idx[0])] = 0.0
        if K > 1:
            E[int(idx[N - 1])] *= 1e-14 / math.sqrt(C)
    elif mode == "g_loss0":
        gl = torch.tensor(0.0)
    elif mode == "g_out0":
        go = torch.zeros(N, C)
    elif mode == "binade":
        go = go * torch.exp2(torch.randint(-12, 13, (N, 1), generator=g).float())
        gl = torch.tensor(2.0 ** 7)
    return z, E, idx, go, gl


def f32v(v):
    return float(torch.tensor(v, dtype=F32))


def ref_bwd(z, E, idx, g_out, g_loss, beta):
    """dz, ge (the per-row codebook contributions), dE with their bounds; zn, zq: the fp64 forward at idx."""
    Z, Ed, GO = _d(z), _d(E), _d(g_out)
    N, C = Z.shape
    K = Ed.shape[0]
    L = _l(C)
    idx = idx.cpu().long()
    gl, beta = float(g_loss), f32v(beta)
    nz = Z.norm(dim=1, keepdim=True)
    Ei = Ed[idx]
    ne = Ei.norm(dim=1, keepdim=True)
    zn, zq = Z / nz.clamp_min(EPS), Ei / ne.clamp_min(EPS)
    bzn = ((C / 16 + 3.5) * U32 + U32) * zn.abs()
    bzq = ((3 + L / 2) * U32 + U32) * zq.abs()
    coef = gl * 2.0 / (N * C)
    d = zn - zq
    dd = bzn + bzq + U32 * d.abs()
    cb = coef * beta
    dzn = GO + cb * d
    Ez = abs(cb) * dd + 5 * U32 * (cb * d).abs() + U32 * dzn.abs()
    dzq = -coef * d
    Eq = abs(coef) * dd + 4 * U32 * dzq.abs()
    n_p = 5 + math.log2(C)
    eps_n = (n_p / 2 + 1) * U32

    def through(y, by, gy, Ey, nrm):
        p = (y * gy).sum(1, keepdim=True)
        dp = (by * gy.abs() + y.abs() * Ey).sum(1, keepdim=True) + n_p * U32 * (y * gy).abs().sum(1, keepdim=True)
        v = gy - y * p
        dv = Ey + by * p.abs() + y.abs() * dp + 2 * U32 * (y * p).abs() + U32 * v.abs()
        above = nrm > EPS
        safe = torch.where(above, nrm, torch.ones_like(nrm))
        gx = torch.where(above, v / safe, gy / EPS)
        bx = torch.where(above, dv / safe + (v / safe).abs() * (eps_n + U32), Ey / EPS + U32 * (gy / EPS).abs())
        return gx, bx, (gy.abs() + (y * p).abs()) / torch.where(above, safe, torch.full_like(nrm, EPS))

    dz, bdz, sdz = through(zn, bzn, dzn, Ez, nz)
    ge, bge, sge = through(zq, bzq, dzq, Eq, ne)
    dE = torch.zeros(K, C, dtype=F64).index_add_(0, idx, ge)
    cnt = torch.zeros(K, dtype=F64).index_add_(0, idx, torch.ones(N, dtype=F64))
    bdE = torch.zeros(K, C, dtype=F64).index_add_(0, idx, bge) \
        + (cnt + 1).view(K, 1) * U32 * torch.zeros(K, C, dtype=F64).index_add_(0, idx, ge.abs())
    bdE[cnt == 0] = 0.0
    return {"dz": dz, "bound_dz": bdz, "ge": ge, "bound_ge": bge, "dE": dE, "bound_dE": bdE, "zn": zn, "zq": zq, "count": cnt,
            # (the magnitudes before the projection cancels: what an fp64 evaluation in another order is compared on)
            "scale_dz": sdz, "scale_dE": torch.zeros(K, C, dtype=F64).index_add_(0, idx, sge)}


def autograd_bwd(z, E, idx, g_out, g_loss, beta):
    """dz, dE by fp64 autograd of the reference formula (rows and codes of norm zero give NaN there)."""
    Z, Ed = _d(z).requires_grad_(True), _d(E).requires_grad_(True)
    zn = Z / Z.norm(dim=1, keepdim=True).clamp_min(EPS)
    zq = torch.nn.functional.embedding(idx.cpu().long(), Ed / Ed.norm(dim=1, keepdim=True).clamp_min(EPS))
    out = zn + (zq - zn).detach()
    loss = f32v(beta) * ((zq.detach() - zn) ** 2).mean() + ((zq - zn.detach()) ** 2).mean()
    dz, dE = torch.autograd.grad((out, loss), (Z, Ed), (_d(g_out), _d(g_loss)))
    return dz, dE


def emulate_bwd(z, E, idx, g_out, g_loss, beta):
    """The backward in f32 on the CPU (torch's summation order) on f32 zn, zq of emulate-style normalisation."""
    eps = torch.tensor(1e-12, dtype=F32)
    N, C = z.shape
    Ei = E[idx]
    nz, ne = torch.sqrt((z * z).sum(1, keepdim=True)), torch.sqrt((Ei * Ei).sum(1, keepdim=True))
    zn, zq = z / torch.maximum(nz, eps), Ei / torch.maximum(ne, eps)
    coef = g_loss.float() * 2.0 / torch.tensor(float(N * C), dtype=F32)
    dzn = g_out + coef * torch.tensor(beta, dtype=F32) * (zn - zq)
    dzq = coef * (zq - zn)
    gz = torch.where(nz > eps, (dzn - zn * (zn * dzn).sum(1, keepdim=True)) / nz, dzn / eps)
    ge = torch.where(ne > eps, (dzq - zq * (zq * dzq).sum(1, keepdim=True)) / ne, dzq / eps)
    return {"dz": gz, "ge": ge, "dE": torch.zeros_like(E).index_add_(0, idx, ge), "zn": zn, "zq": zq}


def ref_gather(idx, E):
    """l2norm(E[idx]) for in-range idx, with its bound."""
    Ed = _d(E)
    C = Ed.shape[1]
    e = Ed[idx.cpu().long()]
    y = e / e.norm(dim=1, keepdim=True).clamp_min(EPS)
    return {"gather": y, "bound_gather": ((3 + _l(C) / 2) * U32 + U32) * y.abs()}
