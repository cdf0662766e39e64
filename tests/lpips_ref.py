"""fp64 reference, per-element bounds and a CPU emulation for the LPIPS distance head of csrc/lpips.hip (amk_lpips_fwd / _bwd,
amk_lpips_bf16_*, ops.lpips_distance), and an fp64 restatement of the whole amk.models.lpips.LPIPS module.

The head.  a, b (N, C, H, W), w (C), eps = 1e-10.  Per sample n and pixel p, over the channels c:
    na = sqrt(sum_c a_c^2), ah_c = a_c / (na + eps);  nb, bh_c likewise;  e_c = ah_c - bh_c;
    d = sum_c w_c e_c^2;  t = sum_c w_c e_c ah_c;  out_n = (1 / HW) sum_p d.
Gradient for a, given the cotangent g_n of out_n, k = 2 g_n / HW:
    ga_c = k (w_c e_c - ah_c t (na + eps) / na) / (na + eps),   and ga_c = 0 for every c of a pixel with na = 0
(autograd gives NaN there: sqrt'(0) * 0).  head() and head_grad() are these formulas in fp64; test_lpips_bounds.py checks
head_grad against fp64 autograd away from zero-norm pixels.

Bounds (u = 2^-24; every formula is evaluated in fp64 on the reference's values, to first order in u, times 1.01 for the
higher orders: C u <= 3.1e-5 at C = 512).  The kernel's operations, one f32 rounding each:
  * sa = sum_c a_c^2 is a chain of fmaf over a channel slice, then a butterfly and three adds over the slices: at most C
    additions deep for every geometry (C >= slices), terms non-negative: relative error C u.  sqrt halves it and rounds
    (C/2 + 1), na + eps rounds (the f32 eps differs from 1e-10 by less than u/2 of itself: + 1 covers both), the
    reciprocal rounds: ia = 1 / (na + eps) carries (C/2 + 4) u.  ah = a ia rounds once more: (C/2 + 5) u |ah|.
  * e = ah - bh, one rounding u |e| <= u (|ah| + |bh|):
        delta_c = KE u (|ah_c| + |bh_c|),   KE = C/2 + 6.
  * d: we = w e rounds (u |w| e^2), fmaf(we, e, acc) rounds only its sum, C additions deep:
        b_d = sum_c |w_c| (2 |e_c| delta_c + delta_c^2) + (C + 1) u sum_c |w_c| e_c^2.
  * out_n: a thread adds its W <= 8 pixels, a wave butterfly (6), three waves (3): 17; the fold adds ceil(tiles / 256)
    partials per thread (tiles <= HW / 4 + 1), a butterfly and three waves again, then the division by HW:
    DP = 17 + ceil(HW / 1024) + 1 + 9 + 1 additions deep over terms bounded by sum_c |w_c| e_c^2:
        b_out_n = (1 / HW) (sum_p b_d + DP u sum_p sum_c |w_c| e_c^2) + floor.
  * t like d with ah in place of the second e (error (C/2 + 5) u |ah|):
        b_t = sum_c |w_c| (delta_c |ah_c| + (C/2 + 5) u |e_c| |ah_c|) + (C + 1) u sum_c |w_c| |e_c| |ah_c|.
    r = (na + eps) / na: na carries (C/2 + 1) u, the sum and the quotient round: (C/2 + 3) u; T = t r rounds:
        b_T = r b_t + (C/2 + 4) u |T|.
  * ga = k2 (w e - ah T) ia with k2 = 2 g / HW (u), w e (u), ah T (u, on top of ah's and T's errors), the difference (u),
    two products (2 u) and ia's (C/2 + 4) u.  With S_c = |w_c| |e_c| + |ah_c| |T| >= |w e - ah T|:
        b_ga = |k| ia (|w_c| delta_c + |ah_c| b_T + (C + 15) u S_c) + floor.
  * bf16 (a, b and ga bf16; the reference is taken on the bf16 values of a and b): the same, plus 2 U8 |ga|, U8 = 2^-8, for
    the one rounding of ga on the store.
  * floor = 1e-5 max |reference| of the tensor, as in tests/bf16_attention_ref.py.  The derived part alone is reported too
    ("tight" ratios), and the emulation is held to half of it as well.
At a pixel with na = 0 the reference and the kernel both give ga = 0; ah = 0 there, and the bound is the floor.

Families (make_inputs): relu -- post-ReLU normals; near -- b = a (1 + 1e-3 noise); identical; zero_pixels -- zero-norm pixels in
a only, in b only and in both; large -- values around 1e3; scaled -- a times 1e-6.  Weights: uniform non-negative ("pos") or of
mixed sign ("mixed").

emulate(): the kernels' f32 operations in the kernels' order on the CPU (make_geo restates csrc/lpips.hip's geometry; fmaf is
taken as the f32 rounding of the fp64 a b + c, whose product is exact).  tests/test_lpips_bounds.py holds it under half of
every bound on every family.
"""
import functools

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
U32, U8 = 2.0 ** -24, 2.0 ** -8
EPS = 1e-10
FLOOR = 1e-5
BLOCK, MIN_TILES = 256, 64
FAMILIES = ("relu", "near", "identical", "zero_pixels", "large", "scaled")
WEIGHTS = ("pos", "mixed")
WORST = {}


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


# ---------------------------------------------------------------------------------------------- inputs
def make_inputs(family, shape, weights="pos", seed=0, bf16=False):
    """{a, b (N, C, H, W) f32, w (C) f32, g (N) f32}; with bf16, a and b hold bf16 values."""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(seed * 7919 + FAMILIES.index(family) * 31 + WEIGHTS.index(weights))
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F32)  # noqa: E731
    a = torch.relu(rn(N, C, H, W))
    b = torch.relu(rn(N, C, H, W))
    if family == "near":
        b = a * (1 + 1e-3 * rn(N, C, H, W))
    elif family == "identical":
        b = a.clone()
    elif family == "zero_pixels":
        m = torch.rand(N, 1, H, W, generator=gen)
        a = a * ((m < 0.25) | (m >= 0.5))      # [0.25, 0.5): a only;  [0.5, 0.75): b only;  [0.75, 1): both
        b = b * (m < 0.5)
        a = a * (m < 0.75)
    elif family == "large":
        a, b = a * 1e3, b * 1e3
    elif family == "scaled":
        a = a * 1e-6
    w = torch.rand(C, generator=gen, dtype=F32)
    if weights == "mixed":
        w = w - 0.5
    g = rn(N)
    if bf16:
        a, b = bf16_round(a), bf16_round(b)
        if family == "identical":
            b = a.clone()
    return dict(a=a.contiguous(), b=b.contiguous(), w=w, g=g)


# ---------------------------------------------------------------------------------------------- fp64 reference
def _parts(a, b, w, eps):
    na = a.pow(2).sum(1, keepdim=True).sqrt()
    nb = b.pow(2).sum(1, keepdim=True).sqrt()
    ah, bh = a / (na + eps), b / (nb + eps)
    e = ah - bh
    wv = w.view(1, -1, 1, 1)
    return na, nb, ah, bh, e, wv


def head(a, b, w, eps=EPS):
    """out (N) in the dtype of the inputs (the autograd-able chain)."""
    _, _, _, _, e, wv = _parts(a, b, w, eps)
    return (wv * e * e).sum(1).mean([1, 2])


def head_grad(a, b, w, g, eps=EPS):
    """ga by the formula of the docstring, zero at zero-norm pixels."""
    na, _, ah, _, e, wv = _parts(a, b, w, eps)
    HW = a.shape[2] * a.shape[3]
    k = (2 * g / HW).view(-1, 1, 1, 1)
    t = (wv * e * ah).sum(1, keepdim=True)
    live = na > 0
    r = torch.where(live, (na + eps) / torch.where(live, na, torch.ones_like(na)), torch.zeros_like(na))
    ga = k * (wv * e - ah * t * r) / (na + eps)
    return torch.where(live, ga, torch.zeros_like(ga))


def reference(inp, bf16=False, eps=EPS):
    """{out, ga: fp64; bound_out, bound_ga: derived part plus floor; tight_out, tight_ga: the derived part alone}."""
    a, b, w, g = (inp[k].to(F64) for k in ("a", "b", "w", "g"))
    N, C, H, W = a.shape
    HW = H * W
    na, nb, ah, bh, e, wv = _parts(a, b, w, eps)
    aw = wv.abs()
    out, ga = head(a, b, w, eps), head_grad(a, b, w, g, eps)
    KE = C / 2 + 6
    delta = KE * U32 * (ah.abs() + bh.abs())
    we2 = (aw * e * e).sum(1)
    b_d = (aw * (2 * e.abs() * delta + delta * delta)).sum(1) + (C + 1) * U32 * we2
    DP = 17 + -(-HW // 1024) + 11
    t_out = 1.01 * (b_d.sum([1, 2]) + DP * U32 * we2.sum([1, 2])) / HW
    live = na > 0
    ia = torch.where(live, 1 / (na + eps), torch.zeros_like(na))
    r = torch.where(live, (na + eps) / torch.where(live, na, torch.ones_like(na)), torch.zeros_like(na))
    wea = (aw * e.abs() * ah.abs()).sum(1, keepdim=True)
    b_t = (aw * delta * ah.abs()).sum(1, keepdim=True) + (C / 2 + 5 + C + 1) * U32 * wea
    T = (wv * e * ah).sum(1, keepdim=True) * r
    b_T = r * b_t + (C / 2 + 4) * U32 * T.abs()
    S = aw * e.abs() + ah.abs() * T.abs()
    k = (2 * g / HW).abs().view(-1, 1, 1, 1)
    t_ga = 1.01 * k * ia * (aw * delta + ah.abs() * b_T + (C + 15) * U32 * S)
    if bf16:
        t_ga = t_ga + 2 * U8 * ga.abs()
    return dict(out=out, ga=ga, tight_out=t_out, tight_ga=t_ga,
                bound_out=t_out + FLOOR * float(out.abs().max()), bound_ga=t_ga + FLOOR * float(ga.abs().max()))


def ratios(got, R, record=None):
    """{out, ga: worst |got - ref| / bound; tight_out, tight_ga: against the derived part alone (0 / 0 counts as 0)}."""
    q = {}
    for name in ("out", "ga"):
        v = got[name].detach().to(F64).cpu().reshape(R[name].shape)
        err = (v - R[name]).abs()
        err = torch.where(torch.isfinite(v), err, torch.full_like(err, float("inf")))
        for kind in ("bound_", "tight_"):
            bd = R[kind + name]
            x = torch.where(err == 0, torch.zeros_like(err), err / bd)
            q[("" if kind == "bound_" else kind) + name] = float(x.max())
    if record is not None:
        for key, val in q.items():
            WORST[(record, key)] = max(WORST.get((record, key), 0.0), val)
    return q


# ---------------------------------------------------------------------------------------------- the kernels' geometry
def make_geo(C, HW, VW):
    """csrc/lpips.hip make_geo: W pixels per thread, PL pixel lanes, CS channel slices, TP pixels per tile, tiles per sample."""
    W = VW if HW % VW == 0 else 1
    PL = BLOCK
    while PL > 4 and -(-HW // (PL * W)) < MIN_TILES and BLOCK // (PL // 4) <= C:
        PL //= 4
    return dict(W=W, PL=PL, CS=BLOCK // PL, TP=PL * W, tiles=-(-HW // (PL * W)))


def ws_floats(N, C, HW, VW):
    return N * make_geo(C, HW, VW)["tiles"]


# ---------------------------------------------------------------------------------------------- CPU emulation
def _fma(x, y, acc):
    return (x.to(F64) * y.to(F64) + acc.to(F64)).to(F32)


def _butterfly(v, offsets):
    """v (..., m): v[i] += v[i ^ o] for o in offsets, every rounding in f32; all entries end equal."""
    idx = torch.arange(v.shape[-1])
    for o in offsets:
        v = v + v[..., idx ^ o]
    return v


def _slice_sum(parts, geo):
    """parts (CS, ...): the fixed-order sum over the channel slices."""
    CS, PL = geo["CS"], geo["PL"]
    if CS == 1:
        return parts[0]
    per_wave = max(1, 64 // PL)
    v = parts.reshape(4, per_wave, *parts.shape[1:]).movedim(1, -1)       # (4 waves, ..., slices of the wave)
    o, offs = 1, []
    while o < per_wave:
        offs.append(o)
        o *= 2
    v = _butterfly(v, offs)[..., 0]
    return ((v[0] + v[1]) + v[2]) + v[3]


def _block_sum(v):
    """v (..., 256) thread values -> the workgroup's sum: butterfly over lane distances 32 .. 1, then the waves in order."""
    v = _butterfly(v.reshape(*v.shape[:-1], 4, 64), (32, 16, 8, 4, 2, 1))[..., 0]
    return ((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]


def emulate(inp, bf16=False, eps=EPS):
    """{out (N), ga (N, C, H, W), rows (3, N, HW)} in f32, as the kernels compute them; with bf16, ga rounded to bf16."""
    a, b, w, g = (inp[k].to(F32) for k in ("a", "b", "w", "g"))
    N, C, H, Wd = a.shape
    HW = H * Wd
    geo = make_geo(C, HW, 8 if bf16 else 4)
    CS, W, PL, TP, tiles = (geo[k] for k in ("CS", "W", "PL", "TP", "tiles"))
    a3, b3 = a.reshape(N, C, HW), b.reshape(N, C, HW)
    epsf = torch.tensor(eps, dtype=F32)
    zero = torch.zeros(N, HW, dtype=F32)

    def sweep(fn):
        parts = []
        for s in range(CS):
            acc = [zero.clone(), zero.clone()]
            for c in range(s, C, CS):
                acc = fn(c, acc)
            parts.append(torch.stack(acc))
        return _slice_sum(torch.stack(parts), geo)

    sa, sb = sweep(lambda c, acc: [_fma(a3[:, c], a3[:, c], acc[0]), _fma(b3[:, c], b3[:, c], acc[1])])
    na, nb = sa.sqrt(), sb.sqrt()
    ia, ib = 1 / (na + epsf), 1 / (nb + epsf)
    live = na > 0
    r = torch.where(live, (na + epsf) / torch.where(live, na, torch.ones_like(na)), torch.zeros_like(na))

    def second(c, acc):
        ah = a3[:, c] * ia
        e = ah - b3[:, c] * ib
        we = w[c] * e
        return [_fma(we, e, acc[0]), _fma(we, ah, acc[1])]

    d, t = sweep(second)
    r0 = torch.where(live, ia, torch.zeros_like(ia))
    r2 = t * r
    # thread (tile, lane) adds its W pixels in order from 0; threads of slice 0 only; then the workgroup, then the fold
    dp = torch.zeros(N, tiles * TP, dtype=F32)
    dp[:, :HW] = d
    dp = dp.reshape(N, tiles, PL, W)
    th = torch.zeros(N, tiles, PL, dtype=F32)
    for k in range(W):
        th = th + dp[..., k]
    full = torch.zeros(N, tiles, BLOCK, dtype=F32)
    full[..., :PL] = th
    part = _block_sum(full)                                                # (N, tiles)
    trips = -(-tiles // BLOCK)
    pp = torch.zeros(N, trips * BLOCK, dtype=F32)
    pp[:, :tiles] = part
    pp = pp.reshape(N, trips, BLOCK)
    th = torch.zeros(N, BLOCK, dtype=F32)
    for j in range(trips):
        th = th + pp[:, j]
    out = _block_sum(th) / torch.tensor(float(HW), dtype=F32)

    k2 = ((2 * g) / torch.tensor(float(HW), dtype=F32)).view(N, 1, 1)
    ah = a3 * r0[:, None]
    e = ah - b3 * ib[:, None]
    ga = k2 * (w.view(1, C, 1) * e - ah * r2[:, None]) * r0[:, None]
    ga = ga.reshape(N, C, H, Wd)
    return dict(out=out, ga=bf16_round(ga) if bf16 else ga, rows=torch.stack([r0, ib, r2]))


# ---------------------------------------------------------------------------------------------- the module in fp64
_CONV_AT = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
_SLICE_OF = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}
_TAPS = (2, 7, 14, 21, 28)          # the convolution whose ReLU output is a level
_POOL_BEFORE = (5, 10, 17, 24)


def module_features(sd, x):
    """The five levels of the tower for x (N, 3, H, W) fp64, from a state_dict of amk.models.lpips.LPIPS."""
    x = (x - sd["scaling_layer.shift"].to(F64)) / sd["scaling_layer.scale"].to(F64)
    outs = []
    for i in _CONV_AT:
        if i in _POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        key = f"net.slice{_SLICE_OF[i]}.{i}"
        x = torch.relu(F.conv2d(x, sd[key + ".weight"].to(F64), sd[key + ".bias"].to(F64), padding=1))
        if i in _TAPS:
            outs.append(x)
    return outs


def module_value(sd, in0, in1, normalize=False):
    """LPIPS(in0, in1) (N, 1, 1, 1) in fp64, autograd-able in in0 (zero-norm pixels: see module_value_and_grad)."""
    in0, in1 = in0.to(F64), in1.to(F64)
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    f0, f1 = module_features(sd, in0), module_features(sd, in1)
    val = 0
    for k in range(5):
        val = val + _LevelHead.apply(f0[k], f1[k].detach(), sd[f"lin{k}.model.1.weight"].to(F64).reshape(-1))
    return val.view(-1, 1, 1, 1)


class _LevelHead(torch.autograd.Function):
    """head() with head_grad() as its backward: the zero-norm rule inside an fp64 autograd graph."""

    @staticmethod
    def forward(ctx, a, b, w):
        ctx.save_for_backward(a, b, w)
        return head(a, b, w)

    @staticmethod
    def backward(ctx, g):
        a, b, w = ctx.saved_tensors
        return head_grad(a, b, w, g), None, None


@functools.lru_cache(maxsize=2)
def _module_case(seed):
    """(state_dict, in0, in1, fp64 loss, fp64 d loss / d in0) for the seeded 2 x 3 x 32 x 32 case; loss = value.mean()."""
    from amk.models.lpips import LPIPS

    torch.manual_seed(seed)
    m = LPIPS()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    in0 = torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1
    in1 = (in0 + 0.1 * torch.randn(2, 3, 32, 32, generator=gen)).clamp(-1, 1)
    x = in0.to(F64).requires_grad_()
    loss = module_value(sd, x, in1).mean()
    (gx,) = torch.autograd.grad(loss, x)
    return sd, in0, in1, loss.detach(), gx


def module_case(seed=0):
    return _module_case(seed)
