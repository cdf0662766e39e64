"""fp64 references and per-element error bounds for the bf16 GEMMs (csrc/gemm_bf16.hip) and the mixed-precision
element-wise kernels (csrc/mixed_bf16.hip).

Every reference is computed in fp64 on the values the kernel sees: bf16 operands as bf16 values, the f32 bias, gamma,
beta and residual as given.  u = 2^-8 (one bf16 round-to-nearest is off by up to 2^-8 of the value), u32 = 2^-24.
Products below are taken over absolute values (S = |A| @ |W| + |bias|).  Rules, as in tests/bf16_attention_ref.py:
every bf16 rounding contributes 2u |ref| (the factor 2 is the margin: roundings do add up coherently), an f32 chain of
n additions n u32 S, and errors pass through silu / silu' to first order.  No term is relative to a tensor's maximum.

* NT / NN, gemm_bf16_kernel<BTR, 0> (amk_gemm_bf16 op 0 / 1): bf16 x bf16 products are exact in f32 and summed by
  v_mfma_f32_32x32x16_bf16 into one f32 accumulator per element over nk = ceil(K / 32) rounded up to even steps of 32
  (the padding step adds exact zeros); the f32 bias is added to the accumulator, then one bf16 rounding:
      c:  2u |c| + n u32 S,   n = 32 ceil(K / 32) + 1.
* SwiGLU forward, EPI 1: a and b are f32 accumulators (bias included) with errors da = n u32 S_a, db = n u32 S_b, and
  g = (a rcp(1 + exp2(-a log2e))) b in f32.  The sigmoid s: the argument a log2e carries 2 u32 of |a| log2e (the f32
  constant and the product), which exp2 turns into 2 u32 |a| of its result, plus one ulp (2 u32) for v_exp_f32; 1 + e
  passes (1 - s) of that on and rounds (u32); v_rcp_f32 is one ulp:
      eps_s = (1 - s)(2 u32 |a| + 2 u32) + 3 u32.
  With silu'(a) = s (1 + a (1 - s)):
      g:  2u |g| + |silu'(a) b| da + |a s| db + |g| (eps_s + 2 u32) + under_g,     (a | b):  as NT.
* SwiGLU backward, EPI 2 (amk_gemm_bf16_swiglu_bwd): dG = dy w3 in f32 (n = 32 ceil(K / 32), no bias) is rounded to
  bf16 in the LDS tile (2u |dG|); a, b are the bf16 (a | b) of the forward.  silu' = s (1 + a (1 - s)) is formed in
  f32 and cancels near a = -1.28, so its error is absolute:
      E_sp = s (|1 + a - 2 a s| eps_s + 2 u32 |a| (1 - s) + u32 |1 + a (1 - s)|) + u32 |silu'|
      da = bf16((dG b) silu'):  4u |da| + |b silu'| n u32 S + |dG b| E_sp + 2 u32 |da| + under_da
      db = bf16(dG (a s)):      4u |db| + |a s| n u32 S + |dG a s| (eps_s + 2 u32) + under_db.
* TN, gemm_tn_bf16_kernel + tn_bf16_reduce_kernel (f32 outputs): each chunk of spc 64-row steps sums its products on
  the MFMA (64 additions per step), then the nchunk partial tiles are summed in chunk order; db is the column sums of
  the staged dY pieces (per thread, then a fold of up to 32 row groups, then the chunks).  spc and nchunk as
  chunks_for() in the source picks them for the device's CU count:
      dw: (64 spc + nchunk) u32 |Y|^T |X|,   db: (64 spc + nchunk + 32) u32 colsum|Y|.
* mixed_bf16.hip (built without fast-math: expf and IEEE division, each within one ulp / correctly rounded):
  swiglu_bf16_fwd / _bwd as EPI 1 / 2 with exact inputs (dG is a bf16 input, so neither its rounding nor S) and
      eps_s = (1 - s) 2 u32 + 2 u32.
  ln_mixed_fwd: h = x + res rounded once (dh = 2 u32 |h| with a residual, else h = x exactly); mean = (sum of the lane
  partials (4 NCH elements each, NCH as AMK_MX_DISPATCH picks it), 64-lane butterfly) times 1/D:
      nl = 4 NCH + 6,  dmean = (nl + 2) u32 mean|h| + mean(dh),
  v = h - mean with dv = dh + dmean + u32 |v|, the variance of the second pass with
      dvar = 2 mean(|v| dv) + (nl + 3) u32 mean(v^2) + u32 (var + eps),   eps_r = dvar / (2 (var + eps)) + 2 u32
  (rsqrtf: one ulp) the relative error of rstd, dxh = rstd dv + |xhat| (eps_r + u32) that of xhat, and
      y = bf16(xhat gamma + beta):  2u |y| + |gamma| dxh + 2 u32 (|xhat gamma| + |y|).
  The one-pass variance E[h^2] - mean^2 would lose everything on a residual stream at 1e3 with a spread of 1: the
  two-pass bound is what the `offset` family checks.
  ln_mixed_bwd reads the forward's f32 h, mean and rstd (errors as above), gy = dy gamma (u32), c1 = mean(gy) and
  c2 = mean(gy xhat) over the same chains, and dh = rstd (gy - c1 - xhat c2) (+ dh_in).  The bracket cancels, so its
  error is absolute:
      d_in = u32 |gy| + dc1 + |xhat| dc2 + |c2| dxh + 3 u32 (|gy| + |c1| + |xhat c2|)
      dh: rstd d_in + |rstd (gy - c1 - xhat c2)| (eps_r + u32) + 2 u32 |dh|   (the last: the f32 sum with dh_in)
      dh16 = bf16(dh): 2u |dh| + the bound of dh.
  dgamma and dbeta are per-workgroup f32 partials (rows per wave, a fold of 4 waves) summed over P <= 2048 partials:
      n = ceil(M / 4P) + P + 5;  dgamma: sum_m |dy| dxh + n u32 sum_m |dy xhat|,  dbeta: n u32 sum_m |dy|.
* under_x = 2 |x| where the fp64 sigmoid or |x| itself is below 2^-120: there the f32 sigmoid underflows (exp2 / expf
  of more than 126 overflows or leaves a subnormal), and the kernel returns anything between 0 and the value.  It
  vanishes wherever nothing underflows.

Input families (make_* below), shared by the CPU check of the bounds themselves and the GPU tests:
  unit: N(0, 1) data as the older tests draw it.  outlier_rows: rows M // 2 and 0 of the activations at 16x and 64x
  (the largest elements away from the last tile's rows).  binade: rows and columns scaled by powers of two over
  2^-12 .. 2^12.  cancel: exact results much smaller than S (the second half of the contraction repeats the first
  against nearly negated weights); for the SwiGLU backward also gate values near the zero of silu' (a in [-1.5, -1]).
  saturate: gate pre-activations over +-300, so that exp2 overflows.  LayerNorm: offset (a residual stream at
  1e3 +- 50 with a spread of about 1), constant (variance 0: y = beta up to rounding), spike (one element per row 1e4 x
  the rest).
"""
import torch

U = 2.0 ** -8
U32 = 2.0 ** -24
TINY = 2.0 ** -120
GEMM_FAMILIES = ("unit", "outlier_rows", "binade", "cancel", "saturate")
LN_FAMILIES = ("unit", "outlier_rows", "binade", "offset", "constant", "spike")
LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))   # the f32 eps the kernel adds


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _d(t):
    return None if t is None else t.detach().to("cpu", torch.float64)


def _row_scale(M, family, g):
    """(M, 1): the per-row factor of the activations of a family."""
    s = torch.ones(M, 1)
    if family == "outlier_rows":
        s[M // 2] = 16.0
        s[0] = 64.0
    elif family == "binade":
        s = torch.exp2(torch.randint(-12, 13, (M, 1), generator=g).float())
    return s


def _col_scale(N, family, g):
    if family != "binade":
        return torch.ones(N)
    return torch.exp2(torch.randint(-12, 13, (N,), generator=g).float())


def make_gemm(family, M, N, K, seed, nn=False):
    """a (M, K), w (N, K) [nn: (K, N)], bias (N,): f32 tensors; a and w hold bf16 values, the bias is f32."""
    g = _gen(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    a = n(M, K) * _row_scale(M, family, g)
    w = n(N, K) * K ** -0.5 * _col_scale(N, family, g).view(N, 1)
    bias = n(N) * _col_scale(N, family, g)
    if family == "cancel":
        h = K // 2                    # w[:, h:2h] = -w[:, :h] + small, a[:, h:2h] = a[:, :h]: the sums nearly cancel
        a[:, h:2 * h] = a[:, :h]
        w[:, h:2 * h] = bf16_round(-w[:, :h] + n(N, h) * K ** -0.5 / 64)
        bias = bias / 64
    elif family == "saturate":
        bias = torch.linspace(-300.0, 300.0, N)[torch.randperm(N, generator=g)]
    a, w = bf16_round(a), bf16_round(w)
    return a, (w.t().contiguous() if nn else w), bias


def make_swiglu(family, M, H, K, seed):
    """a (M, K), w12 (2H, K), b12 (2H,) for the SwiGLU forward; saturate puts the gate biases over +-300."""
    a, w12, b12 = make_gemm("unit" if family == "saturate" else family, M, 2 * H, K, seed)
    if family == "saturate":
        b12[:H] = torch.linspace(-300.0, 300.0, H)[torch.randperm(H, generator=_gen(seed + 1))]
    return a, w12, b12


def make_ab(family, M, H, seed):
    """(a | b) (M, 2H) bf16 values: the forward's pre-activations as the backward kernels read them."""
    g = _gen(seed + 3)
    ab = torch.randn(M, 2 * H, generator=g) * _row_scale(M, family, g)
    if family == "binade":
        ab = ab * _col_scale(2 * H, family, g)
    elif family == "cancel":
        ab[:, :H] = -1.0 - 0.5 * torch.rand(M, H, generator=g)      # around the zero of silu' (a = -1.278)
    elif family == "saturate":
        ab[:, :H] = torch.linspace(-300.0, 300.0, H)[torch.randperm(H, generator=g)] + torch.randn(M, H, generator=g)
    return bf16_round(ab)


def make_swiglu_bwd(family, M, H, K, seed):
    """dy (M, K), w3 (K, H), ab (M, 2H): the SwiGLU-backward GEMM's operands."""
    dy, w3, _ = make_gemm("unit" if family == "saturate" else family, M, H, K, seed, nn=True)
    return dy, w3, make_ab(family, M, H, seed)


def make_tn(family, M, N, K, seed):
    """y (M, N), x (M, K): dY and X of a weight gradient, bf16 values."""
    g = _gen(seed)
    r = _row_scale(M, family, g)
    y = torch.randn(M, N, generator=g) * r * _col_scale(N, family, g)
    x = torch.randn(M, K, generator=g) * r * _col_scale(K, family, g)
    if family == "cancel":
        h = M // 2
        x[h:2 * h] = x[:h]
        y[h:2 * h] = bf16_round(-y[:h] + torch.randn(h, N, generator=g) / 64)
    return bf16_round(y), bf16_round(x)


def make_ln(family, M, D, seed, x_bf16=True):
    """x (M, D) (bf16 values if x_bf16), res (M, D), gamma, beta (D,), cy (M, D) bf16 values (the cotangent of y),
    ch (M, D) (that of h, the dh_in of the backward): f32 tensors."""
    g = _gen(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    x, res = n(M, D), n(M, D)
    gamma, beta = n(D) * 0.5 + 1.0, n(D)
    if family in ("outlier_rows", "binade"):
        s = _row_scale(M, family, g)
        x, res = x * s, res * s
    elif family == "offset":
        res = 1000.0 + 50.0 * n(M, 1) + res
    elif family == "constant":
        x, res = n(M, 1).expand(M, D).clone(), (4.0 * n(M, 1)).expand(M, D).clone()
    elif family == "spike":
        j = torch.randint(0, D, (M,), generator=g)
        x[torch.arange(M), j] = 1e4 * torch.sign(n(M))
    if x_bf16:
        x = bf16_round(x)
    return x, res, gamma, beta, bf16_round(n(M, D)), n(M, D)


def make_ab_cot(family, M, H, seed):
    """(a | b) (M, 2H) and the cotangent of g (M, H), bf16 values: the element-wise SwiGLU's inputs."""
    cot = torch.randn(M, H, generator=_gen(seed + 5))
    return make_ab(family, M, H, seed), bf16_round(cot)


# ---------------------------------------------------------------------------------------------- references + bounds
def gemm_chain(K):
    """The longest f32 chain of gemm_bf16_kernel: 32 products per step of 32, over ceil(K / 32) steps."""
    return 32 * ((K + 31) // 32)


def _eps_sigmoid(a, s, hw):
    """Relative error of the f32 sigmoid: hardware exp2 of a rounded a log2e + v_rcp_f32 (hw), or expf + IEEE division."""
    if hw:
        return (1 - s) * (2 * U32 * a.abs() + 2 * U32) + 3 * U32
    return (1 - s) * 2 * U32 + 2 * U32


def _under(x, s):
    return torch.where((s < TINY) | (x.abs() < TINY), 2 * x.abs(), torch.zeros_like(x))


def _gemm64(a, w, bias, nn):
    """(C, S) in fp64: C = a w^T + bias [nn: a w], S = |a| |w|^T + |bias|."""
    A, W, B = _d(a), _d(w), _d(bias)
    if not nn:
        W = W.t()
    C, S = A @ W, A.abs() @ W.abs()
    if B is not None:
        C, S = C + B, S + B.abs()
    return C, S


def ref_gemm(a, w, bias=None, nn=False):
    """{"c", "bound_c"}: a (M, K), w (N, K) [nn: (K, N)], bias (N,) or None."""
    C, S = _gemm64(a, w, bias, nn)
    return {"c": C, "bound_c": 2 * U * C.abs() + (gemm_chain(a.shape[1]) + 1) * U32 * S}


def ref_swiglu_fwd(a, w12, b12):
    """{"g", "ab", "bound_g", "bound_ab"} of gemm_bf16_kernel<false, 1>."""
    AB, S = _gemm64(a, w12, b12, False)
    eAB = (gemm_chain(a.shape[1]) + 1) * U32 * S
    H = AB.shape[1] // 2
    x, y, ex, ey = AB[:, :H], AB[:, H:], eAB[:, :H], eAB[:, H:]
    s = torch.sigmoid(x)
    gref = x * s * y
    sp = s * (1 + x * (1 - s))
    bound = 2 * U * gref.abs() + (sp * y).abs() * ex + (x * s).abs() * ey + gref.abs() * (_eps_sigmoid(x, s, True) + 2 * U32)
    return {"g": gref, "ab": AB, "bound_g": bound + _under(gref, s), "bound_ab": 2 * U * AB.abs() + eAB}


def _swiglu_bwd(A, B, G, eG, rounded, hw):
    """da, db and their bounds for the cotangent G (fp64) with error eG (f32 chain; None when G is an exact input),
    rounded: G passes through one bf16 rounding on the way."""
    s = torch.sigmoid(A)
    eps_s = _eps_sigmoid(A, s, hw)
    sp = s * (1 + A * (1 - s))
    E_sp = s * ((1 + A - 2 * A * s).abs() * eps_s + 2 * U32 * A.abs() * (1 - s) + U32 * (1 + A * (1 - s)).abs()) + U32 * sp.abs()
    da, db = G * B * sp, G * A * s
    r = (4 if rounded else 2) * U
    bda = r * da.abs() + (G * B).abs() * E_sp + 2 * U32 * da.abs() + _under(da, s)
    bdb = r * db.abs() + (G * A * s).abs() * (eps_s + 2 * U32) + _under(db, s)
    if eG is not None:
        bda = bda + (B * sp).abs() * eG
        bdb = bdb + (A * s).abs() * eG
    return da, db, bda, bdb


def ref_swiglu_bwd(dy, w3, ab):
    """{"dab", "bound_dab"} of gemm_bf16_kernel<true, 2>: (dA | dB) for dG = dy w3 and the forward's (a | b)."""
    Y, W, AB = _d(dy), _d(w3), _d(ab)
    G = Y @ W
    eG = gemm_chain(Y.shape[1]) * U32 * (Y.abs() @ W.abs())
    H = G.shape[1]
    da, db, bda, bdb = _swiglu_bwd(AB[:, :H], AB[:, H:], G, eG, True, True)
    return {"dab": torch.cat([da, db], 1), "bound_dab": torch.cat([bda, bdb], 1)}


def ref_swiglu_mixed(ab, cot):
    """{"g", "dab", bounds} of swiglu_bf16_fwd / _bwd_kernel: g = silu(a) b, (dA | dB) for the bf16 cotangent cot."""
    AB, G = _d(ab), _d(cot)
    H = G.shape[1]
    A, B = AB[:, :H], AB[:, H:]
    s = torch.sigmoid(A)
    g = A * s * B
    bg = 2 * U * g.abs() + g.abs() * (_eps_sigmoid(A, s, False) + 2 * U32) + _under(g, s)
    da, db, bda, bdb = _swiglu_bwd(A, B, G, None, False, False)
    return {"g": g, "bound_g": bg, "dab": torch.cat([da, db], 1), "bound_dab": torch.cat([bda, bdb], 1)}


def tn_tile_k(N, K, tk=None):
    """The K width of the weight-gradient tile, as tile_k() in csrc/gemm_bf16.hip picks it (default settings).  tk: the
    width AMK_TN16_TK forces (128 or 256; anything else is ignored there and here)."""
    if tk in (128, 256):
        return tk
    return 256 if K >= 256 and ((N + 127) // 128) * ((K + 255) // 256) >= 12 else 128


def tn_chunks(M, N, K, cus=256, tk=None, wgs=1):
    """(steps per chunk, chunks) as chunks_for() in csrc/gemm_bf16.hip picks them (default settings).  tk, wgs: what
    AMK_TN16_TK and AMK_TN16_WGS force (workgroups per CU the grid aims at)."""
    TK = tn_tile_k(N, K, tk)
    tiles = ((N + 127) // 128) * ((K + TK - 1) // TK)
    steps = (M + 63) // 64
    chunks = max(1, wgs * cus // tiles)
    if chunks > steps // 8:
        chunks = max(1, steps // 8)
    s = (steps + chunks - 1) // chunks
    return s, (steps + s - 1) // s


def ref_tn(y, x, cus=256, tk=None, wgs=1):
    """{"dw", "db", "bound_dw", "bound_db"} of amk_gemm_tn_bf16: dW = y^T x, db = column sums of y."""
    Y, X = _d(y), _d(x)
    M, N = Y.shape
    spc, nch = tn_chunks(M, N, X.shape[1], cus, tk, wgs)
    n = 64 * spc + nch
    return {"dw": Y.t() @ X, "bound_dw": n * U32 * (Y.abs().t() @ X.abs()),
            "db": Y.sum(0), "bound_db": (n + 32) * U32 * Y.abs().sum(0)}


def ln_nch(D):
    return 1 if D <= 256 else 2 if D <= 512 else 4 if D <= 1024 else 8 if D <= 2048 else 16


def ln_parts(M):
    return min(2048, max(1, (M + 3) // 4))


def ref_ln(x, res, gamma, beta, dy=None, dh_in=None, eps=LN_EPS):
    """The mixed LayerNorm forward (h, y, mean, rstd) and, with dy, backward (dh, dh16, dgamma, dbeta), with bounds.
    res None: h = x.  dh_in None: no residual-stream gradient is added."""
    X, Rs, Gm, Bt = _d(x), _d(res), _d(gamma), _d(beta)
    M, D = X.shape
    H = X + Rs if Rs is not None else X
    eh = 2 * U32 * H.abs() if Rs is not None else torch.zeros_like(H)
    nl = 4 * ln_nch(D) + 6
    mean = H.mean(-1, keepdim=True)
    dmean = (nl + 2) * U32 * H.abs().mean(-1, keepdim=True) + eh.mean(-1, keepdim=True)
    v = H - mean
    dv = eh + dmean + U32 * v.abs()
    var = (v * v).mean(-1, keepdim=True)
    dvar = 2 * (v.abs() * dv).mean(-1, keepdim=True) + (nl + 3) * U32 * var + U32 * (var + eps)
    rstd = 1.0 / torch.sqrt(var + eps)
    eps_r = dvar / (2 * (var + eps)) + 2 * U32
    xh = v * rstd
    dxh = rstd * dv + xh.abs() * (eps_r + U32)
    y = xh * Gm + Bt
    R = {"h": H, "bound_h": eh, "mean": mean[:, 0], "bound_mean": dmean[:, 0], "rstd": rstd[:, 0],
         "bound_rstd": (rstd * eps_r)[:, 0], "y": y,
         "bound_y": 2 * U * y.abs() + Gm.abs() * dxh + 2 * U32 * ((xh * Gm).abs() + y.abs())}
    if dy is None:
        return R
    DY = _d(dy)
    gy = DY * Gm
    c1 = gy.mean(-1, keepdim=True)
    c2 = (gy * xh).mean(-1, keepdim=True)
    dc1 = (nl + 2) * U32 * gy.abs().mean(-1, keepdim=True)
    dc2 = (gy.abs() * dxh).mean(-1, keepdim=True) + (nl + 3) * U32 * (gy * xh).abs().mean(-1, keepdim=True)
    inner = gy - c1 - xh * c2
    d_in = U32 * gy.abs() + dc1 + xh.abs() * dc2 + c2.abs() * dxh + 3 * U32 * (gy.abs() + c1.abs() + (xh * c2).abs())
    dh = rstd * inner + (_d(dh_in) if dh_in is not None else 0.0)
    bdh = rstd * d_in + (rstd * inner).abs() * (eps_r + U32) + 2 * U32 * dh.abs()
    P = ln_parts(M)
    n = -(-M // (4 * P)) + P + 5
    R.update({"dh": dh, "bound_dh": bdh, "dh16": dh, "bound_dh16": 2 * U * dh.abs() + bdh,
              "dgamma": (DY * xh).sum(0), "bound_dgamma": (DY.abs() * dxh).sum(0) + n * U32 * (DY * xh).abs().sum(0),
              "dbeta": DY.sum(0), "bound_dbeta": n * U32 * DY.abs().sum(0)})
    return R


# ---------------------------------------------------------------------------------------------- checking
def ratios(got, R, names):
    """{name: (elements outside the bound, worst |got - ref| / bound)} for the tensors of `got` (any device / dtype)."""
    res = {}
    for n in names:
        a = got[n].detach().to("cpu", torch.float64)
        assert a.shape == R[n].shape, (n, tuple(a.shape), tuple(R[n].shape))
        err = (a - R[n]).abs()
        bad = ~(err <= R["bound_" + n])              # (a NaN is outside the bound too)
        r = torch.where(err == 0, torch.zeros_like(err), err / R["bound_" + n])   # (an exact zero: bound 0)
        res[n] = (int(bad.sum()), float(r.max()) if a.numel() else 0.0)
    return res


WORST = {}   # worst ratio per output over every assert_within of the process (reported by the GPU tests)


def assert_within(got, R, names, what="", key=None):
    """Every element of got[name] within the bound of R; records the worst ratio in WORST under key / name."""
    res = ratios(got, R, names)
    for n, (nbad, worst) in res.items():
        k = f"{key}.{n}" if key else n
        WORST[k] = max(WORST.get(k, 0.0), worst)
        assert nbad == 0, f"{what} {n}: {nbad} elements outside the bound (worst {worst:.3g}x the bound)"
    return res
