"""fp64 references, per-element error bounds, input families and f32 CPU emulations for the f32 row kernels:
csrc/layernorm.hip (add + LayerNorm forward / backward, column sums), csrc/elementwise.hip (SwiGLU and GEGLU gates) and
csrc/optim.hip (squared-norm partials + the flat Adam / AdamW step).

Rules, as in tests/bf16_dense_ref.py (whose formulas are reused wherever the kernels share their form): the reference is
computed in fp64 on the f32 inputs; every rounded f32 operation contributes u32 = 2^-24 of the magnitude of its result,
propagated to first order; a sum of n terms contributes n u32 sum|t|, n read off the source; no term is relative to a
tensor's maximum and every element is checked.

Library functions.  csrc/Makefile compiles with `-O3` and no fast-math flag, and hipcc's defaults for HIP are
-fhip-fp32-correctly-rounded-divide-sqrt (on) and no -ffast-math / -fgpu-approx-transcendentals: sqrtf and `/` are
correctly rounded (u32) -- the code objects hold the v_div_scale / v_div_fmas / v_div_fixup sequence and v_sqrt_f32
with its two-FMA correction.  rsqrtf and expf: one ulp (2 u32), the budgets bf16_dense_ref.py fixes.  erff: nothing states the
device library's accuracy, so the hard budget is the OpenCL specification's limit for erf, 16 ulp = 32 u32 |erf| -- the
specification's limit, not a measurement.  hipcc contracts a * b + c into an FMA where it likes (-ffp-contract=fast): an
FMA drops one rounding, so the bounds hold for either form and the emulations below come in both.

* add_layernorm_fwd / _bwd: the chains are those of the mixed LayerNorm (one wave per row, a lane sums its 4 NCH
  elements, a 64-lane butterfly, times the rounded 1 / D; two-pass variance; rsqrtf), so bf16_dense_ref.ref_ln is the
  bound with its bf16 output roundings (2u |y|, dh16) removed:
      h = x + res: 2 u32 |h| (exact without a residual);   nl = 4 NCH + 6
      mean: (nl + 2) u32 mean|h| + mean(dh);    v = h - mean: dv = dh + dmean + u32 |v|
      var: dvar = 2 mean(|v| dv) + (nl + 3) u32 var + u32 (var + eps);  rstd: rstd (dvar / (2 (var + eps)) + 2 u32)
      y = (v rstd) gamma + beta:  |gamma| dxh + 2 u32 (|xhat gamma| + |y|),  dxh = rstd dv + |xhat| (eps_r + u32)
      dh = rstd (gy - c1 - xhat c2) (+ dh_in): the bracket cancels, its error is absolute (d_in of bf16_dense_ref)
      dgamma, dbeta: rows per wave ceil(M / 4P), a fold of 4 waves, P <= 2048 partials summed by torch:
          n = ceil(M / 4P) + P + 5;  dgamma: sum_m |dy| dxh + n u32 sum_m |dy xhat|,  dbeta: n u32 sum_m |dy|.
* colsum: rows per wave, a fold of 4 waves, P partials:  n u32 sum_m |x|,  n = ceil(M / 4P) + 4 + P.
* swiglu_fwd / _bwd: bf16_dense_ref's element-wise SwiGLU with exact inputs and no output rounding
  (eps_s = (1 - s) 2 u32 + 2 u32, E_sp absolute because silu' cancels near a = -1.278, under_x where the f32 sigmoid or
  the result underflows).
* geglu_fwd / _bwd: z = a * 0.70710678f carries 2 u32 |z| (the constant, the product), which erf turns into
  2 u32 |z| erf'(z); erff adds 32 u32 |erf|; 1 + erf rounds once.  The sum cancels in the tail, so its error is absolute:
      E1 = 32 u32 |erf(z)| + 2 u32 |z| (2 / sqrt pi) exp(-z^2) + u32 |1 + erf(z)|
      out = ((0.5 a) (1 + erf)) b:   |0.5 a b| E1 + 2 u32 |out| + under
      gelu' = 0.5 (1 + erf) + (a k) expf((-0.5 a) a), k = 0.39894228f.  T2 = a phi(a): a k carries 2 u32, the
      argument w = a^2 / 2 one rounding that expf turns into u32 w, expf 2 u32, the product u32:
      E_gp = 0.5 E1 + |T2| (5 + w) u32 + u32 |gelu'|            (absolute: gelu' has a zero near a = -0.7518)
      da = (g b) gelu':  |g b| E_gp + 2 u32 |da| + under,     db = g gelu(a):  |0.5 a g| E1 + 2 u32 |db| + under.
  Beyond |a| = 13.2 expf underflows; T2 is below 1e-37 there and the 32 u32 |erf| term covers it.
* sumsq_partials + adam_flat_step: the norm is a sum of squares, all terms positive, so its relative error is the
  number of roundings on the longest path times u32: the square, (x^2 + y^2) + (z^2 + w^2) and the accumulation (4), one
  more accumulation per further segment of the lane (ceil(ceil(nseg / 256) / 4) - 1), the butterfly (6), the fold of
  4 waves (2); then in the update kernel one addition per bucket sharing the partials, butterfly (6), fold (2):
      chain = 20 + (iters - 1) + buckets,   norm = sqrtf(sum):  (chain / 2 + 1) u32 norm.
  coef = min(1, max_norm / (norm + 1e-6f)): q = max_norm / d with d = norm + 1e-6f has the relative error
  (dnorm + u32 d) / d + u32; it enters gg = g coef (u32) and from there m', v' and p'.  The table entries
  lr / bias_correction1, sqrt(bias_correction2) and the decay factor are f32 roundings of fp64 values (u32 each).
      L2:  gg += wdf p (one FMA);    AdamW:  pp = p - wdf p:  2 u32 |wdf p| + u32 |pp|
      m' = m + omb1 (gg - m):  omb1 (dgg + u32 |gg - m|) + 2 u32 |omb1 (gg - m)| + u32 |m'|
      v' = beta2 v + (omb2 gg) gg:  2 |omb2 gg| dgg + 3 u32 omb2 gg^2 + u32 beta2 v + u32 v' + under_v'
          (v = 0 and a gradient of 1e-18 leave v' = 1e-39, a subnormal; sqrt(v') is then far below eps)
      denom = sqrtf(v') / bc2s + eps:  sqrt(v') (dv' / 2 v' + u32) / bc2s + 2 u32 sqrt(v') / bc2s + u32 denom
      p' = pp - step (m' / denom):  dpp + step (dm' / denom + |r| ddenom / denom + u32 |r|) + 2 u32 |upd| + u32 |p'|.
  A parameter without a gradient keeps p, m, v bitwise (bound 0).
* MARGIN.  The outputs of the gates and p', m', v' pass through 3 to 10 roundings, which do add up coherently -- one
  rounding alone reaches u32 |x| just above a power of two -- so a bound of u32 per rounding is met in practice and no
  emulation could stay under half of it.  Their bounds are the sums above times 2: the factor is the margin, as for
  the bf16 roundings of bf16_dense_ref and the last rounding in gn_act_ref, and "the emulation under half" then says
  that the emulation keeps the plain sum of u32 per rounding.  The sums (LayerNorm, colsum, the norm) carry no factor:
  their n u32 sum|t| is a worst case over chains whose errors add up like a random walk.

Families (make_* below), all inside the f32 range so that the fp64 reference is meaningful.  LayerNorm: the six of
bf16_dense_ref.LN_FAMILIES with gamma near 1 and one column in 16 at |gamma| < 1e-3.  colsum: unit, cancel (columns
alternating +-1e4 by row), binade (columns over 2^-12 .. 2^12).  Gates: unit (scale 2), saturate (|a| up to 300 with values
either side of 88.7 and 104), silu_zero (a in [-1.5, -1]), gelu_zero (a in [-0.9, -0.6]), gelu_tail (a in [-7, -2]),
binade (b and the cotangent over 2^-20 .. 2^20), zero (a = +-0).  Adam: unit, tiny (1e-12: sqrt v << eps), large (1e15:
g^2 finite), binade (segments over 2^-12 .. 2^12); t = 1 and 1000; clipping off, active and armed but inactive.
"""
import math

import torch

import bf16_dense_ref as bf
from bf16_dense_ref import LN_EPS, LN_FAMILIES, TINY, U32, _d, _gen, assert_within, ln_nch, ln_parts, ratios  # noqa: F401

WORST = bf.WORST           # assert_within records the worst ratios there
F32, F64 = torch.float32, torch.float64
ERF_ULP = 16               # the OpenCL specification's limit for erf
MARGIN = 2                 # on the bounds of the element-wise outputs (see the module docstring)
COL_FAMILIES = ("unit", "cancel", "binade")
GATE_FAMILIES = ("unit", "saturate", "silu_zero", "gelu_zero", "gelu_tail", "binade", "zero")
ADAM_FAMILIES = ("unit", "tiny", "large", "binade")
SEG = 256                  # elements per segment of csrc/optim.hip
NPART = 256                # squared-norm partials per bucket

LN_SHAPES = [(5, 4), (37, 256), (37, 260), (9, 512), (9, 516), (9, 1024), (9, 1028), (6, 2048), (6, 2052), (5, 4096),
             (8195, 8), (65541, 4)]
LN_ALL_FAMILY_SHAPES = [(37, 260), (9, 1028), (6, 2052)]
COL_SHAPES = [(1, 4), (3, 260), (8195, 256), (70, 1024), (70, 2048), (33, 4096)]
GATE_SHAPES = [(1, 4), (7, 20), (33, 96), (5, 1368)]
GATE_STRIDE_SHAPE = (2052, 4096)       # 2 101 248 float4 items > 8192 * 256
ADAM_NSEGS = (1, 3, 255, 256, 257, 1029, 8200)


def f32v(v):
    """The f32 value nearest to v, as a Python float: what a `float` argument of the C ABI carries."""
    return float(torch.tensor(v, dtype=F32))


def ln_cases():
    """(family, M, D, with res, with dh_in): all six families at three shapes, unit + offset at the rest; the four
    res x dh_in combinations go round."""
    out, k = [], 0
    for M, D in LN_SHAPES:
        for fam in (LN_FAMILIES if (M, D) in LN_ALL_FAMILY_SHAPES else ("unit", "offset")):
            out.append((fam, M, D, bool(k & 1), bool(k & 2)))
            k += 1
    return out


# ---------------------------------------------------------------------------------------------- LayerNorm
def make_ln(family, M, D, seed):
    """x, res (M, D), gamma, beta (D,), cy (the cotangent of y), ch (that of h: dh_in): f32."""
    x, res, gamma, beta, _, ch = bf.make_ln(family, M, D, seed, x_bf16=False)
    if family == "offset":
        x, res = res, x            # the offset travels in x, so that a run without a residual keeps it
    g = _gen(seed + 7)
    k = torch.randperm(D, generator=g)[: max(1, D // 16)]
    gamma[k] = 1e-3 * (torch.rand(len(k), generator=g) - 0.5)
    return x, res, gamma, beta, torch.randn(M, D, generator=g), ch


def ref_ln(x, res, gamma, beta, dy=None, dh_in=None, eps=LN_EPS):
    """h, y, mean, rstd and, with dy, dh, dgamma, dbeta of amk_add_layernorm_fwd / _bwd with their bounds:
    bf16_dense_ref.ref_ln without the bf16 roundings of its outputs."""
    R = bf.ref_ln(x, res, gamma, beta, dy, dh_in, eps)
    R["bound_y"] = R["bound_y"] - 2 * bf.U * R["y"].abs()      # (what remains is at least 2 u32 |y|: no cancellation)
    R.pop("dh16", None)
    R.pop("bound_dh16", None)
    return R


LN_FWD = ("y", "mean", "rstd")
LN_BWD = ("dh", "dgamma", "dbeta")


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _butterfly(s):
    """wave_sum over the last axis of 64 lanes: every lane ends with the same value."""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ o]
    return s[..., :1]


def _lanes(t, D):
    """(M, D) -> (M, NCH, 64, 4): element k of chunk lane + 64 j, zero beyond the row."""
    M = t.shape[0]
    W = 256 * ln_nch(D)
    p = torch.zeros(M, W, dtype=F32)
    p[:, :D] = t
    return p.view(M, W // 256, 64, 4)


def _lane_sum(t, s=None):
    """s += t.x + t.y + t.z + t.w chunk by chunk, then the butterfly: (M, 1)."""
    s = torch.zeros(t.shape[0], 64, dtype=F32) if s is None else s
    for j in range(t.shape[1]):
        s = s + (((t[:, j, :, 0] + t[:, j, :, 1]) + t[:, j, :, 2]) + t[:, j, :, 3])
    return _butterfly(s)


def _col_partials(t, fold_first=None):
    """Column sums the way the reducing kernels form them: (M, N) -> rows blockIdx * 4 + wave + k * 4P accumulated in
    order per (workgroup, wave), the 4 waves folded, the P partial rows summed (torch.sum)."""
    M, N = t.shape
    P = ln_parts(M)
    K = -(-M // (4 * P))
    p = torch.zeros(K * 4 * P, N, dtype=F32)
    p[:M] = t
    p = p.view(K, P, 4, N)
    acc = torch.zeros(P, 4, N, dtype=F32)
    for k in range(K):
        acc = acc + p[k]
    part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    return part.sum(0)


def emulate_ln(x, res, gamma, beta, dy=None, dh_in=None, eps=LN_EPS, fma=False):
    """The two kernels of csrc/layernorm.hip in f32 on the CPU, in their summation order; fma: the epilogues, the
    backward's bracket and the dgamma accumulation as fused multiply-adds."""
    M, D = x.shape
    h = x + res if res is not None else x
    mask = _lanes(torch.ones(M, D), D)
    gl, bl = _lanes(gamma.view(1, D), D), _lanes(beta.view(1, D), D)
    inv_d = torch.tensor(1.0, dtype=F32) / torch.tensor(float(D), dtype=F32)
    mean = _lane_sum(_lanes(h, D)) * inv_d
    v = (_lanes(h, D) - mean.view(M, 1, 1, 1)) * mask
    rstd = torch.rsqrt(_lane_sum(v * v) * inv_d + torch.tensor(eps, dtype=F32))
    r4 = rstd.view(M, 1, 1, 1)
    y = _fma(v * r4, gl, bl) if fma else (v * r4) * gl + bl
    out = {"h": h, "y": y.reshape(M, -1)[:, :D], "mean": mean[:, 0], "rstd": rstd[:, 0]}
    if dy is None:
        return out
    xh = ((_lanes(h, D) - mean.view(M, 1, 1, 1)) * r4) * mask
    d = _lanes(dy, D)
    gy = d * gl
    c1 = (_lane_sum(gy) * inv_d).view(M, 1, 1, 1)
    c2 = (_lane_sum(gy * xh) * inv_d).view(M, 1, 1, 1)
    o = r4 * (_fma(-xh, c2, gy - c1) if fma else (gy - c1) - xh * c2)
    o = o.reshape(M, -1)[:, :D]
    xhf = xh.reshape(M, -1)[:, :D]
    out.update({"dh": o + dh_in if dh_in is not None else o, "dgamma": _col_partials(dy * xhf), "dbeta": _col_partials(dy)})
    return out


# ---------------------------------------------------------------------------------------------- colsum
def make_colsum(family, M, N, seed):
    g = _gen(seed)
    x = torch.randn(M, N, generator=g)
    if family == "cancel":
        sign = 1.0 - 2.0 * (torch.arange(M) % 2).float()
        x = x + 1e4 * sign.view(M, 1) * (1.0 + torch.rand(N, generator=g))
    elif family == "binade":
        x = x * torch.exp2(torch.randint(-12, 13, (N,), generator=g).float())
    return x


def colsum_chain(M):
    P = ln_parts(M)
    return -(-M // (4 * P)) + 4 + P


def ref_colsum(x):
    X = _d(x)
    return {"colsum": X.sum(0), "bound_colsum": colsum_chain(X.shape[0]) * U32 * X.abs().sum(0)}


def emulate_colsum(x):
    return {"colsum": _col_partials(x)}


# ---------------------------------------------------------------------------------------------- gates
_EDGES = (-88.8, -88.6, 88.6, 88.8, -104.1, -103.9, 103.9, 104.1, -300.0, 300.0, -87.0, -13.3, 13.3, -13.1)


def make_gate(family, M, H, seed):
    """(a | b) (M, 2H) and the cotangent of the output (M, H), f32."""
    g = _gen(seed)
    ab = 2.0 * torch.randn(M, 2 * H, generator=g)
    cot = 2.0 * torch.randn(M, H, generator=g)
    u = torch.rand(M, H, generator=g)
    if family == "saturate":
        a = torch.linspace(-300.0, 300.0, M * H)[torch.randperm(M * H, generator=g)]
        a[: len(_EDGES)] = torch.tensor(_EDGES)[: M * H]
        ab[:, :H] = a.view(M, H)
    elif family == "silu_zero":
        ab[:, :H] = -1.0 - 0.5 * u
    elif family == "gelu_zero":
        ab[:, :H] = -0.6 - 0.3 * u
    elif family == "gelu_tail":
        ab[:, :H] = -2.0 - 5.0 * u
    elif family == "binade":
        ab[:, H:] *= torch.exp2(torch.randint(-20, 21, (M, H), generator=g).float())
        cot = cot * torch.exp2(torch.randint(-20, 21, (M, H), generator=g).float())
    elif family == "zero":
        ab[:, :H] = 0.0 * (1.0 - 2.0 * (torch.arange(M * H) % 2).float()).view(M, H)    # +0, -0, +0, ...
    return ab, cot


def ref_swiglu(ab, cot):
    """out = silu(a) b, da, db of amk_swiglu_fwd / _bwd with bounds: bf16_dense_ref's element-wise forms, no bf16."""
    AB, G = _d(ab), _d(cot)
    H = G.shape[1]
    A, B = AB[:, :H], AB[:, H:]
    s = torch.sigmoid(A)
    out = A * s * B
    da, db, bda, bdb = bf._swiglu_bwd(A, B, G, None, False, False)
    bout = out.abs() * (bf._eps_sigmoid(A, s, False) + 2 * U32) + bf._under(out, s)
    return {"out": out, "bound_out": MARGIN * bout, "da": da, "bound_da": MARGIN * (bda - 2 * bf.U * da.abs()),
            "db": db, "bound_db": MARGIN * (bdb - 2 * bf.U * db.abs())}


def ref_geglu(ab, cot):
    """out = gelu(a) b (exact erf GELU), da, db of amk_geglu_fwd / _bwd with bounds."""
    AB, G = _d(ab), _d(cot)
    H = G.shape[1]
    A, B = AB[:, :H], AB[:, H:]
    z = A / math.sqrt(2.0)
    one_erf = torch.special.erfc(-z)                       # 1 + erf(z) without the cancellation
    E1 = 2 * ERF_ULP * U32 * torch.erf(z).abs() + 2 * U32 * z.abs() * (2 / math.sqrt(math.pi)) * torch.exp(-z * z) \
        + U32 * one_erf
    gelu = 0.5 * A * one_erf
    w = 0.5 * A * A
    T2 = A * torch.exp(-w) / math.sqrt(2 * math.pi)
    gp = 0.5 * one_erf + T2
    E_gp = 0.5 * E1 + T2.abs() * (5 + w) * U32 + U32 * gp.abs()
    ones = torch.ones_like(A)
    out, da, db = gelu * B, G * B * gp, G * gelu
    return {"out": out, "bound_out": MARGIN * ((0.5 * A * B).abs() * E1 + 2 * U32 * out.abs() + bf._under(out, ones)),
            "da": da, "bound_da": MARGIN * ((G * B).abs() * E_gp + 2 * U32 * da.abs() + bf._under(da, ones)),
            "db": db, "bound_db": MARGIN * ((0.5 * A * G).abs() * E1 + 2 * U32 * db.abs() + bf._under(db, ones))}


REF_GATE = {"swiglu": ref_swiglu, "geglu": ref_geglu}
GATE_OUT = ("out", "da", "db")


def emulate_gate(kind, ab, cot):
    """The four kernels of csrc/elementwise.hip in f32 on the CPU (torch's expf / erff for the device library's)."""
    H = cot.shape[1]
    a, b, g = ab[:, :H], ab[:, H:], cot
    one = torch.tensor(1.0, dtype=F32)
    if kind == "swiglu":
        s = one / (one + torch.exp(-a))
        return {"out": a * s * b, "da": g * b * (s * (one + a * (one - s))), "db": g * (a * s)}
    c, k = torch.tensor(0.70710678118654752, dtype=F32), torch.tensor(0.39894228040143268, dtype=F32)
    one_erf = one + torch.erf(a * c)
    gelu = 0.5 * a * one_erf
    gp = 0.5 * one_erf + a * k * torch.exp(-0.5 * a * a)
    return {"out": gelu * b, "da": g * b * gp, "db": g * gelu}


# ---------------------------------------------------------------------------------------------- Adam
def adam_hyper(adamw=False, wd=0.0, table=True, max_norm=0.0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """The hyper-parameters as the f32 values the C ABI receives.  table: the decay factor travels in the parameter
    table (`decoupled` bit 1), else in the launch arguments."""
    return dict(adamw=bool(adamw), wd=f32v(wd), table=bool(table), max_norm=f32v(max_norm), lr=f32v(lr),
                beta1=f32v(beta1), beta2=f32v(beta2), eps=f32v(eps))


def adam_modes():
    """(adamw, wd, table): Adam and AdamW, wd = 0 and != 0, `decoupled` bit 1 set and clear."""
    return [(False, 0.0, True), (False, 0.05, True), (True, 0.05, True), (False, 0.05, False), (True, 0.05, False),
            (True, 0.0, False)]


def make_adam(family, nsegs, seed, t=1):
    """One step's state over the buckets of nsegs segments each (they share one partials array): flat p, g, m, v over
    all buckets, the segment -> parameter table, per parameter {active, t}.  Every bucket of 3 or more segments holds
    three parameters, the middle one without a gradient this step (its g is still read by the norm and zeroed)."""
    gen = _gen(seed)
    seg_param, active, pid = [], [], 0
    for ns in nsegs:
        sizes = [ns] if ns < 3 else [ns // 3, max(1, ns // 5), ns - ns // 3 - max(1, ns // 5)]
        for i, sz in enumerate(sizes):
            seg_param += [pid] * sz
            active.append(not (len(sizes) == 3 and i == 1))
            pid += 1
    n = SEG * sum(nsegs)
    rn = lambda: torch.randn(n, generator=gen)  # noqa: E731
    scale = {"unit": 1.0, "tiny": 1e-12, "large": 1e15, "binade": 1.0}[family]
    seg_scale = torch.ones(n)
    if family == "binade":
        seg_scale = torch.exp2(torch.randint(-12, 13, (n // SEG,), generator=gen).float()).repeat_interleave(SEG)
    g = rn() * scale * seg_scale
    m = rn() * scale * seg_scale * 0.5
    v = torch.rand(n, generator=gen) * (scale * seg_scale) ** 2
    v[::7] = 0.0
    p = rn() * torch.exp2(torch.randint(-12, 3, (n,), generator=gen).float())     # small elements too
    return dict(p=p, g=g, m=m, v=v, nsegs=list(nsegs), seg_param=torch.tensor(seg_param, dtype=torch.int32),
                active=torch.tensor(active), t=torch.full((pid,), int(t), dtype=torch.int64))


def adam_cases():
    """(family, nseg, t, mode index, clip): clip 0 off, 1 active, 2 armed but inactive, 3 tiny norm against the 1e-6."""
    out, k = [], 0
    modes = adam_modes()
    for nseg in ADAM_NSEGS:
        for fam in (ADAM_FAMILIES if nseg in (3, 257) else ("unit", "tiny")):
            out.append((fam, nseg, 1 if k % 2 else 1000, k % len(modes), k % 3))
            k += 1
    out += [("tiny", 257, 1, 1, 3), ("tiny", 3, 1000, 2, 3), ("large", 1029, 1, 3, 1), ("unit", 257, 1, 4, 1),
            ("unit", 3, 1000, 5, 2), ("binade", 1029, 1000, 1, 1)]
    return out


def adam_problem(fam, nseg, t, mode, clip):
    """(state, hyper-parameters): the bucket under test plus a second one of 5 segments on the same partials."""
    pr = make_adam(fam, [nseg, 5], 500 + nseg + mode, t)
    norm = float(pr["g"].to(F64).pow(2).sum().sqrt())
    max_norm = {0: 0.0, 1: norm / 3, 2: norm * 3, 3: 1e-7}[clip]
    adamw, wd, table = adam_modes()[mode]
    return pr, adam_hyper(adamw=adamw, wd=wd, table=table, max_norm=max_norm)


def adam_table(pr, hp, t_shift=0):
    """(P, 4) f32 {active, lr / bias_correction1, sqrt(bias_correction2), decay factor}, computed in fp64 and rounded
    once, as amk.optim.FlatAdam fills it."""
    t = (pr["t"] + t_shift).to(F64)
    tab = torch.zeros(len(t), 4, dtype=F64)
    tab[:, 0] = pr["active"].to(F64)
    tab[:, 1] = hp["lr"] / (1.0 - hp["beta1"] ** t)
    tab[:, 2] = torch.sqrt(1.0 - hp["beta2"] ** t)
    tab[:, 3] = hp["wd"] * hp["lr"] if hp["adamw"] else hp["wd"]
    return tab.to(F32)


def norm_chain(nsegs):
    """Roundings on the longest path of a squared element to the folded sum (see the module docstring)."""
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    iters = max(ceil(ceil(ns, NPART), 4) for ns in nsegs)
    return 20 + (iters - 1) + len(nsegs)


EPS_CLIP = f32v(1e-6)


def ref_adam(pr, hp):
    """norm, p', m', v' of amk_sumsq_partials + amk_adam_flat_step in fp64 with their bounds."""
    P, G, M_, V = (_d(pr[k]) for k in ("p", "g", "m", "v"))
    idx = pr["seg_param"].long().repeat_interleave(SEG)
    act = pr["active"][idx]
    t = pr["t"].to(F64)[idx]
    b1, b2, eps = hp["beta1"], hp["beta2"], hp["eps"]
    ss = hp["lr"] / (1.0 - b1 ** t)
    bc2s = torch.sqrt(1.0 - b2 ** t)
    N = float(torch.sqrt((G * G).sum()))
    eN = N * (norm_chain(pr["nsegs"]) / 2 + 1) * U32
    c, ec = 1.0, 0.0
    if hp["max_norm"] > 0:
        d = N + EPS_CLIP
        q = hp["max_norm"] / d
        rel = (eN + U32 * d) / d + U32
        c = min(1.0, q)
        ec = 0.0 if q * (1 - rel) >= 1 else rel * q
    gg = G * c
    e_gg = G.abs() * ec + U32 * gg.abs()
    pp, e_pp = P, torch.zeros_like(P)
    if hp["wd"] != 0:
        wdf = hp["wd"] * hp["lr"] if hp["adamw"] else hp["wd"]
        wp = wdf * P
        if hp["adamw"]:
            pp = P - wp
            e_pp = 2 * U32 * wp.abs() + U32 * pp.abs()
        else:
            gg = gg + wp
            e_gg = e_gg + U32 * wp.abs() + U32 * gg.abs()
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    d1 = gg - M_
    mm = M_ + omb1 * d1
    e_mm = omb1 * (e_gg + U32 * d1.abs()) + 2 * U32 * (omb1 * d1).abs() + U32 * mm.abs()
    vv = b2 * V + omb2 * gg * gg
    e_vv = 2 * (omb2 * gg).abs() * e_gg + 3 * U32 * omb2 * gg * gg + U32 * b2 * V + U32 * vv + bf._under(vv, torch.ones_like(vv))
    sq = torch.sqrt(vv)
    e_sq = sq * (torch.where(vv > 0, e_vv / vv.clamp_min(1e-300), torch.zeros_like(vv)) / 2 + U32)
    q1 = sq / bc2s
    den = q1 + eps
    e_den = e_sq / bc2s + 2 * U32 * q1 + U32 * den
    r = mm / den
    e_r = e_mm / den + r.abs() * e_den / den + U32 * r.abs()
    upd = ss * r
    pn = pp - upd
    e_pn = e_pp + ss * e_r + 2 * U32 * upd.abs() + U32 * pn.abs()
    z = torch.zeros_like(P)
    return {"norm": torch.tensor([N], dtype=F64), "bound_norm": torch.tensor([eN], dtype=F64),
            "p": torch.where(act, pn, P), "bound_p": torch.where(act, MARGIN * e_pn, z),
            "m": torch.where(act, mm, M_), "bound_m": torch.where(act, MARGIN * e_mm, z),
            "v": torch.where(act, vv, V), "bound_v": torch.where(act, MARGIN * e_vv, z)}


ADAM_OUT = ("norm", "p", "m", "v")


def emulate_sumsq(g, nsegs):
    """amk_sumsq_partials per bucket: (256 * buckets,) f32 partials in the kernel's order."""
    out, o = [], 0
    for ns in nsegs:
        per = -(-ns // NPART)
        iters = -(-per // 4)
        x = torch.zeros(NPART * iters * 4 * SEG, dtype=F32).view(NPART, iters * 4, SEG)
        gb = g[o * SEG:(o + ns) * SEG].view(ns, SEG)
        for w in range(NPART):
            s0, s1 = w * per, min(ns, (w + 1) * per)
            if s1 > s0:
                x[w, : s1 - s0] = gb[s0:s1]
        x = x.view(NPART, iters, 4, 64, 4)
        acc = torch.zeros(NPART, 4, 64, dtype=F32)
        for i in range(iters):
            v = x[:, i]
            acc = acc + ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + (v[..., 2] * v[..., 2] + v[..., 3] * v[..., 3]))
        red = _butterfly(acc)[..., 0]
        out.append((red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3]))
        o += ns
    return torch.cat(out)


def emulate_adam(pr, hp, fma=False):
    """amk_sumsq_partials + amk_adam_flat_step in f32 on the CPU in the kernels' order; fma: the moment updates, the
    AdamW decay and the parameter update as fused multiply-adds."""
    T = lambda x: torch.tensor(x, dtype=F32)  # noqa: E731
    partials = emulate_sumsq(pr["g"], pr["nsegs"])
    lanes = torch.zeros(-(-len(partials) // 256) * 256, dtype=F32)
    lanes[: len(partials)] = partials
    acc = torch.zeros(256, dtype=F32)
    for row in lanes.view(-1, 256):
        acc = acc + row
    red = _butterfly(acc.view(4, 64))[:, 0]
    norm = torch.sqrt((red[0] + red[1]) + (red[2] + red[3]))
    coef = T(1.0)
    if hp["max_norm"] > 0:
        coef = torch.minimum(T(1.0), T(hp["max_norm"]) / (norm + T(1e-6)))
    tab = adam_table(pr, hp)
    idx = pr["seg_param"].long().repeat_interleave(SEG)
    act, ss, bc2s = tab[idx, 0] != 0, tab[idx, 1], tab[idx, 2]
    if hp["table"]:
        wdf = tab[idx, 3]
    else:
        wdf = (T(hp["lr"]) * T(hp["wd"]) if hp["adamw"] else T(hp["wd"])).expand_as(ss)
    p, m, v = pr["p"], pr["m"], pr["v"]
    b2, eps = T(hp["beta2"]), T(hp["eps"])
    omb1, omb2 = T(1.0) - T(hp["beta1"]), T(1.0) - b2
    gg, pp = pr["g"] * coef, p
    if hp["wd"] != 0:
        if hp["adamw"]:
            pp = _fma(-wdf, p, p) if fma else p - wdf * p
        else:
            gg = _fma(wdf, p, gg)
    mm = _fma(omb1, gg - m, m) if fma else m + omb1 * (gg - m)
    vv = _fma(omb2 * gg, gg, b2 * v) if fma else b2 * v + omb2 * gg * gg
    den = torch.sqrt(vv) / bc2s + eps
    pn = _fma(-ss, mm / den, pp) if fma else pp - ss * (mm / den)
    return {"norm": norm.view(1), "p": torch.where(act, pn, p), "m": torch.where(act, mm, m), "v": torch.where(act, vv, v)}
