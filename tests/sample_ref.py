"""fp64 reference, licences, bounds, logit families and the Philox stream for csrc/sample.hip (amk_sample_step).

Rules, as in tests/bf16_dense_ref.py: the reference is fp64 on the f32 inputs; every rounded f32 operation costs
u = 2^-24 of its result, to first order; a sum of n terms costs n u sum|t|, n read off the source; nothing is relative to
a tensor's maximum; every row is checked.

Reference (sample.hip:9-15, ops.sample_step):
    s = n + scale (l - n)   (s = l without guidance);   kept = {j : s_j >= the keep-th largest s}  (-0.0 == +0.0);
    pred = first argmax over kept of s + g   (0 when tau == 0);   score = softmax(s)[pred].

* s (sample.hip:84-88): d = l - n, scale d, n + . -- two roundings after d, or one FMA (hipcc may contract):
      ds = 2 u |scale d| + u |s|        (0 without guidance: s is the logit itself, and every check below is exact).
* threshold (sample.hip:106-130), exact by construction: with g = +G on one element of value equal to the keep-th largest
  and 0 elsewhere that element must be chosen; in the twin row +G sits on the largest element BELOW the threshold and
  +G / 2 on the row's maximum, which must be chosen.  G = 8 max|s| + 100 (over the finite s) separates the three
  outcomes in f32 whatever the magnitudes: 7 max|s| <= s_below + G, s_max + G / 2 <= 5 max|s| + 50.  Among equal values
  at the threshold the element is the first or the last of them (both are run): "all equal values are kept".
  With guidance only rows whose fp64 gap between ranks keep and keep + 1 exceeds ds_k + ds_k+1 are used
  (at most MAX_EXCLUDED = 1 % may be excluded, asserted on the CPU).
* prediction under random noise: y = s + g is one more rounding, dy = ds + u |y|.  lo = s - ds, hi = s + ds; element j
  is surely kept when fewer than keep OTHER elements have hi_i > lo_j, possibly kept when fewer than keep have
  lo_i > hi_j (without guidance both are the kept set itself).  Licence: pred is possibly kept and y_pred + dy_pred >= max over the surely kept of (y_j - dy_j).  A row
  whose two sets agree and whose gap of y between the top and the next distinct value exceeds the two dy must match the
  fp64 argmax (the first of exactly equal sums: equal real sums round to equal f32 sums) exactly; at most
  MAX_LICENSED = 1 % of rows may fall short of that (asserted on the CPU).
* score (sample.hip:97-104, 175): term j is __expf(s_j - m): the budget tests/ce_head_ref.py fixes, 2.5 u |s_j - m| + 2 u
  (subtraction, log2(e) scaling and its constant, v_exp_f32 within one ulp), plus ds_j: r_j.  The shift m is the same
  f32 number in every term and cancels.  Z: a lane adds ceil(V / 256) terms, 6 shuffle adds, 2 adds over the waves:
      rel(Z) = sum_j p_j r_j + (ceil(V / 256) + 8) u + V 2^-126 / Z   (the last: terms that underflow),
      bound_score = score (r_pred + rel(Z) + u) + 2^-149   (the last: a subnormal quotient),
  relative, for probabilities below 1e-20 as for the others; an argument below -104 gives exactly 0 on both sides.
* in-kernel noise (sample.hip:31-55, 143): Philox4x32-10, key = seed, counter = (low: row V / 4 + j / 4, high: offset),
  element j takes word j % 4; u = ((w >> 9) + 0.5) 2^-23, g = -log(-log u).  __logf is v_log_f32 times ln 2: nothing in
  the project fixes a budget for v_log_f32 -- ASSUMED one ulp, as the project does for v_exp_f32 -- so a = -log u
  carries 3.5 u |a| (the instruction, the constant, the product), the outer logarithm turns that into 3.5 u absolute
  and adds its own 3.5 u |g|:  dg = 4 u (1 + |g|).  Licence with equal logits 0 and keep = V: g_ref[pred] >= max g_ref
  - dg_pred - dg_max; at most 1 % of rows may have a top-two gap inside it (asserted on the CPU: none has).

Families (make_logits): gaussian; negative (all below zero); last_byte (1 + j 2^-23: all four radix passes decide);
wide (+-1e30 mixed with values near 1); denormal (f32 subnormals of both signs and zeros); neg_inf (a third of the logits
-inf, never with guidance); bf16_ties (values rounded to bf16: many equal values at the threshold); zero (+0.0 and -0.0
on both sides of the threshold between positive and negative values).
"""
import math

import numpy as np
import torch

import bf16_dense_ref as bf
from bf16_dense_ref import U32, _gen, assert_within, ratios  # noqa: F401

WORST = bf.WORST
F32, F64 = torch.float32, torch.float64
FAMILIES = ("gaussian", "negative", "last_byte", "wide", "denormal", "neg_inf", "bf16_ties", "zero")
GUIDED_FAMILIES = ("gaussian", "negative")
CFG_SCALE = 3.0
VS = (4, 64, 1000, 1024, 1028, 8192, 36864)
MAX_V = 36864
TAUS = (1.0, 1.0 / 18, 0.0)
MAX_EXCLUDED = 0.01
MAX_LICENSED = 0.01
NOISE_SHAPES = ((3, 64), (2, 1028), (1, 8192))
NOISE_KEYS = ((1234, 0), (1234, 7), (2 ** 40 + 99, 0), (2 ** 40 + 99, 7))
# a (seed, offset) whose stream over 8 rows of V = 8192 holds exactly one word with its top 24 bits set -- the word the
# 24-bit map sent to u = 1 and g = +inf -- and where: found by find_gumbel_hit(GUMBEL_HIT_SEED), which the CPU test reruns
GUMBEL_HIT_SEED = 950
GUMBEL_HIT_ROWS, GUMBEL_HIT_V = 8, 8192
GUMBEL_HIT = (353, 6, 4788)   # (offset, row, j)


def keeps(V):
    return sorted({1, min(2, V), math.ceil(0.1 * V), max(1, V - 1), V})


# ---------------------------------------------------------------------------------------------- Philox
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(seed, ctr_hi, ctr_lo):
    """(..., 4) uint32 words of Philox4x32-10 for the 64-bit counter halves ctr_lo (array), ctr_hi and the 64-bit key."""
    lo = np.asarray(ctr_lo, dtype=np.uint64)
    c = [lo & _MASK, lo >> np.uint64(32), np.full_like(lo, ctr_hi & 0xFFFFFFFF), np.full_like(lo, (ctr_hi >> 32) & 0xFFFFFFFF)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def words(seed, offset, rows, V):
    """(rows, V) uint32: the word element (row, j) of a call with this seed and offset draws."""
    ctr = np.arange(rows * (V // 4), dtype=np.uint64)      # row V / 4 + j / 4
    return philox4x32_10(seed, offset, ctr).reshape(rows, V)


def uniform_of(w):
    """The kernel's word -> uniform map; exact in f32, so the double is the f32 value."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def uniform_f32(top, bits):
    """f32 emulation of ((float)(w >> (32 - bits)) + 0.5f) * 2^-bits on the values `top` of w >> (32 - bits)."""
    return (top.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -bits)


def gumbel_of(w):
    u = uniform_of(w)
    return -np.log(-np.log(u))


def dg(g):
    return 4 * U32 * (1 + np.abs(g))


def find_gumbel_hit(seed, max_offset=4096):
    """The first offset whose stream over GUMBEL_HIT_ROWS x GUMBEL_HIT_V holds exactly one word with its top 24 bits
    set: (offset, row, j)."""
    for off in range(max_offset):
        w = words(seed, off, GUMBEL_HIT_ROWS, GUMBEL_HIT_V)
        hit = np.argwhere((w >> np.uint32(8)) == 0xFFFFFF)
        if len(hit) == 1:
            return off, int(hit[0, 0]), int(hit[0, 1])
    return None


# ---------------------------------------------------------------------------------------------- families
def make_logits(family, R, V, seed):
    """(R, V) f32 logits."""
    g = _gen(seed)
    x = 2.0 * torch.randn(R, V, generator=g)
    if family == "negative":
        x = -x.abs() - 1e-3
    elif family == "last_byte":
        x = (1.0 + torch.arange(V, dtype=F64) * 2.0 ** -23).float().repeat(R, 1)
        x = torch.stack([r[torch.randperm(V, generator=g)] for r in x])
    elif family == "wide":
        x = 1.0 + 0.1 * x
        sel = torch.rand(R, V, generator=g)
        x = torch.where(sel < 0.2, torch.full_like(x, 1e30), torch.where(sel > 0.8, torch.full_like(x, -1e30), x))
    elif family == "denormal":
        x = (x * 1e-40).float()
        x[:, ::5] = 0.0
    elif family == "neg_inf":
        x[torch.rand(R, V, generator=g) < 1 / 3] = -math.inf
        x[:, 0] = 0.5                                     # (never a row of -inf alone)
    elif family == "bf16_ties":
        x = (0.25 * x).to(torch.bfloat16).float()
    elif family == "zero":
        sel = torch.rand(R, V, generator=g)
        z = torch.where(torch.rand(R, V, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
        x = torch.where(sel < 0.9, z, x)      # (5 % positive, 5 % negative: keep = V / 10 puts the threshold at zero)
    return x.contiguous()


def make_gumbel(R, V, seed):
    return -torch.empty(R, V).exponential_(generator=_gen(seed)).log()


# ---------------------------------------------------------------------------------------------- reference
def scaled(logits, null, scale):
    """s in fp64 and ds."""
    L = logits.to(F64)
    if null is None:
        return L, torch.zeros_like(L)
    Nn = null.to(F64)
    sd = float(torch.tensor(scale, dtype=F32)) * (L - Nn)
    s = Nn + sd
    return s, 2 * U32 * sd.abs() + U32 * s.abs()


def kth_largest(x, k):
    return torch.topk(x, k, dim=1).values[:, k - 1:k]


def threshold_rows(s, ds, keep, pick):
    """The exact threshold check: (g_first, want_first, g_twin, want_twin, usable) per row; pick: 'first' or 'last' of the
    elements equal to the keep-th largest.  want_twin = -1: the row has nothing below its threshold (no twin)."""
    R, V = s.shape
    thr = kth_largest(s, keep)
    # (fewer than keep finite values: everything is kept, and the last element that can win is the smallest finite one)
    thr = torch.where(torch.isfinite(thr), thr, torch.where(torch.isfinite(s), s, torch.full_like(s, math.inf)).min(1, keepdim=True).values)
    fin = torch.where(torch.isfinite(s), s.abs(), torch.zeros_like(s))
    G = (8 * fin.max(1).values + 100).float()
    eq = s == thr                                         # (-0.0 == +0.0)
    ar = torch.arange(V).view(1, V)
    at = torch.where(eq, ar, torch.full_like(ar, -1 if pick == "last" else V))
    at = at.max(1).values if pick == "last" else at.min(1).values
    below = torch.where(s < thr, s, torch.full_like(s, -math.inf))
    has = torch.isfinite(below.max(1).values)
    nxt = below.argmax(1)
    top = s.argmax(1)
    n = torch.arange(R)
    g1 = torch.zeros(R, V)
    g1[n, at] = G
    g2 = torch.zeros(R, V)
    g2[n, top] = G / 2
    g2[n[has], nxt[has]] = G[has]
    gap_ok = torch.ones(R, dtype=torch.bool)
    if bool((ds != 0).any()):
        gap_ok = ~has | ((thr[:, 0] - below.max(1).values) > ds[n, at] + ds[n, nxt])
    return g1, at, g2, torch.where(has, top, torch.full_like(top, -1)), gap_ok


def ref_pred(s, ds, g, keep):
    """(argmax, possibly kept, y, dy, exact): the prediction licence of the module docstring."""
    y = s + g.to(F64)
    dy = ds + U32 * torch.where(torch.isfinite(y), y.abs(), torch.zeros_like(y))
    lo, hi = s - ds, s + ds
    V = s.shape[1]
    above = lambda srt, x: V - torch.searchsorted(srt, x.contiguous(), right=True)  # noqa: E731  (elements of a row > x)
    sure = above(torch.sort(hi, 1).values, lo) - (hi > lo).long() < keep
    poss = above(torch.sort(lo, 1).values, hi) < keep
    ninf = torch.full_like(y, -math.inf)
    floor = torch.where(sure, y - dy, ninf).max(1).values
    ys = torch.where(poss, y, ninf)
    t = ys.max(1, keepdim=True).values
    arg = (ys == t).to(torch.uint8).argmax(1)              # the first of exactly equal sums (equal in f32 as well)
    n = torch.arange(y.shape[0])
    lower = torch.where(ys < t, ys, ninf)                   # the next DISTINCT value
    second = lower.argmax(1)
    gap = torch.where(torch.isfinite(lower.max(1).values), t[:, 0] - lower.max(1).values, torch.full_like(t[:, 0], math.inf))
    exact = (sure == poss).all(1) & (gap > dy[n, arg] + dy[n, second])
    return dict(argmax=arg, poss=poss, y=y, dy=dy, floor=floor, exact=exact)


def check_pred(P, pred, tau, what=""):
    """pred (R,) against the licence; returns the number of rows that differ from the fp64 argmax."""
    pred = pred.cpu().long()
    n = torch.arange(len(pred))
    if tau == 0:
        assert bool((pred == 0).all()), f"{what}: tau = 0 must predict index 0"
        return 0
    assert bool(P["poss"][n, pred].all()), f"{what}: a prediction outside the kept set"
    ok = P["y"][n, pred] + P["dy"][n, pred] >= P["floor"]
    assert bool(ok.all()), f"{what}: rows {ok.logical_not().nonzero().view(-1).tolist()[:8]} outside the licence"
    wrong = P["exact"] & (pred != P["argmax"])
    assert not bool(wrong.any()), f"{what}: rows {wrong.nonzero().view(-1).tolist()[:8]} differ from the fp64 argmax"
    return int((pred != P["argmax"]).sum())


def ref_score(s, ds, pred):
    """softmax(s)[pred] with its bound, (R,)."""
    R, V = s.shape
    n = torch.arange(R)
    m = s.max(1, keepdim=True).values
    a = s - m
    e = torch.exp(a)
    Z = e.sum(1)
    p = e / Z.view(R, 1)
    live = a > -200
    r = torch.where(live, ds + 2.5 * U32 * a.abs() + 2 * U32, torch.zeros_like(a))
    relZ = (p * r).sum(1) + (math.ceil(V / 256) + 8) * U32
    pred = pred.cpu().long()
    sc = p[n, pred]
    return {"score": sc, "bound_score": sc * (r[n, pred] + relZ + U32 + V * 2.0 ** -126 / Z) + 2.0 ** -149}


# ---------------------------------------------------------------------------------------------- the cases of the tests
def noise_cases(V, guided):
    """[(family, keep, rows, tau, masked, unmasked_score, seed)]: every family x keep; rows, tau, mask go round."""
    out = []
    for fam in (GUIDED_FAMILIES if guided else FAMILIES):
        for keep in keeps(V):
            i = len(out)
            out.append((fam, keep, 1 if i % 4 == 3 else 5, TAUS[i % 3], i % 2 == 1, 1.0 if i % 4 == 1 else -1.0, 1000 + 17 * i + V))
    return out


def noise_problem(V, guided, case):
    """logits, null (or None), gumbel, mask (or None) of a case."""
    fam, keep, R, tau, masked, _, seed = case
    logits = make_logits(fam, R, V, seed)
    null = make_logits(fam, R, V, seed + 1) if guided else None
    mask = (torch.rand(R, generator=_gen(seed + 3)) < 0.6) if masked else None
    return logits, null, make_gumbel(R, V, seed + 2), mask


def make_small_prob(R, V, seed):
    """logits, gumbel, the index that must be chosen: an element 50 .. 80 below the row's maximum carries g = +200, so
    the chosen probability lies between e^-80 / Z and e^-50 / Z (below 1e-20), still a normal f32."""
    logits = make_logits("gaussian", R, V, seed)
    at = torch.randint(0, V, (R,), generator=_gen(seed + 1))
    n = torch.arange(R)
    logits[n, at] = -1e9
    logits[n, at] = logits.max(1).values - torch.linspace(50.0, 80.0, R)
    g = torch.zeros(R, V)
    g[n, at] = 200.0
    return logits, g, at


def emulate(logits, null, scale, g, keep, tau):
    """The kernel's op chain in f32 on the CPU, the softmax denominator in the kernel's order (a lane adds elements
    t, t + 256, ..., then the 64-lane butterfly, then the four waves): (pred, score)."""
    s = logits if null is None else null + torch.tensor(scale, dtype=F32) * (logits - null)
    R, V = s.shape
    y = torch.where(s >= kth_largest(s, keep), s + g, torch.full_like(s, -math.inf))
    pred = (y == y.max(1, keepdim=True).values).to(torch.uint8).argmax(1) if tau > 0 else torch.zeros(R, dtype=torch.long)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    pad = torch.zeros(R, -(-V // 256) * 256, dtype=F32)
    pad[:, :V] = e
    acc = torch.zeros(R, 256, dtype=F32)
    for chunk in pad.view(R, -1, 256).unbind(1):
        acc = acc + chunk
    acc = acc.view(R, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    z = (acc[:, 0, 0] + acc[:, 1, 0]) + (acc[:, 2, 0] + acc[:, 3, 0])
    return pred, e[torch.arange(R), pred] / z
