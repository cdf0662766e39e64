"""fp64 references, per-element error bounds, input families and a restatement of the host dispatch for the dense
exact-f32 GEMMs and the row statistics of csrc/gemm_f32.hip (amk_gemm_f32, amk_row_stats), as tests/moe_ref.py does it
for the MoE kernels.

Every reference is computed in fp64 on the f32 values the kernel reads (any device: the GPU tests keep them on the
device).  For the LayerNorm fold these are the mean and rstd tensors handed to the GEMM, not fp64 statistics; row_stats
has a reference and a bound of its own.  u32 = 2^-24.  No bound is relative to a tensor's maximum.

Hard tier (a theorem).  A result that is a sum of terms t_i, each formed by at most n rounded f32 operations on any path
from an input to the result -- in any order, fused or not -- satisfies
    |got - ref| <= gamma_n S + n 2^-126,   gamma_n = n u32 / (1 - n u32),   S = sum |t_i|.
n per output, read off the source:
* the MFMA chain over a contraction of length L (v_mfma_f32_32x32x2_f32, the rounding of an fmaf chain): a product
  rounding (absent when fused) and at most L additions on any path; the K tail and absent rows / columns are staged as
  exact zeros and add nothing:  chain(L) = L + 1.
* NT (gemm_nt_kernel, gemm_nt_dkernel): the chain over K, the bias add (1), the residual add (1):
      n = K + 3,   S = |A'| |W|^T + |bias| + |R|.
* LayerNorm fold (NT and TN operand staging): a' = fmaf((a - mu) rs, gamma, beta) has three roundings, a' =
  ((a - mu) rs gamma + beta)(1 + theta_3) with |A'| <= |(a - mu) rs gamma| + |beta|; they are carried through |W| by
  taking n + 3 and that |A'| in S.  (The flush-to-zero term grows by 3 2^-126 sum_k |w|.)
* NT with two projections: each segment is an NT of its own (same n); the dispatch, not the arithmetic, differs.
* SwiGLU forward: a = acc_a + b12[j], b = acc_b + b12[H + j] are NT results (n = K + 2; errors ea, eb);
  s = 1 / (1 + expf(-a)): expf is within one ulp (2 u32; csrc/Makefile builds this file without fast-math, so expf and
  the IEEE division are the accurate ones), which 1 + e passes on scaled by (1 - s); the sum and the division round
  once each: eps_s = (1 - s) 2 u32 + 2 u32.  g = (a s) b rounds twice more.  To first order through silu
  (silu' = s (1 + a (1 - s)), |silu''| <= 1/2 covers the second order):
      g:  |silu'(a) b| ea + |a s| eb + |g| (eps_s + 2 u32) + (ea^2 / 4) |b| + ea eb + under_g;   (a | b): as NT.
* NN (gemm_nn_kernel): n = chain(K1 + K2) = K1 + K2 + 1, S = |A1| |W1| + |A2| |W2|: the two contraction segments are
  one chain (each segment's tail is padded with exact zeros).
* SwiGLU backward (NN epilogue): dG = dy w3 with error eG = the NN bound; a, b are read from (a | b).
  silu' = s (1 + a (1 - s)) is formed in f32 and cancels near a = -1.278, so its error is absolute:
      E_sp = s (|1 + a - 2 a s| eps_s + 2 u32 |a| (1 - s) + u32 |1 + a (1 - s)|) + u32 |silu'|
      dA = (dG b) silu':  |b silu'| eG + |dG b| E_sp + 2 u32 |dA| + |b| eG E_sp + under
      dB = dG (a s):      |a s| eG + |dB| (eps_s + 2 u32) + under.
* TN (gemm_tn_kernel + tn_reduce_kernel): the chain of one chunk (BK steps_per_chunk rows) and nchunk additions of the
  partial tiles in chunk order:  n = BK steps_per_chunk + 1 + nchunk (+ 3 with the LayerNorm fold),  S = |Y|^T |X'|.
* dbias: every thread sums the rows r = cr (mod 8) of its chunk (BK steps_per_chunk / 8 additions), the 8-way fold
  through LDS (8), the chunks (nchunk):  n = BK steps_per_chunk / 8 + 8 + nchunk,  S = colsum |Y|.
* row_stats: a lane sums 4 NCH elements, the 64-lane butterfly adds 6 times, 1 / D is rounded and multiplied (2):
      nl = 4 NCH + 6,   mean: n = nl + 2,  S = mean |x|.
  v = x - mean (computed) is off by dv = dmean + u32 |v|; the two-pass variance sums v^2 over the same chain:
      dvar = 2 mean(|v| dv) + mean(dv^2) + gamma_(nl + 4) (var + mean(dv^2)) + u32 (var + eps)
  and rstd = rsqrtf(var + eps) (one ulp, 2 u32) has the relative error
      eps_r = 1 / sqrt(1 - dvar / (var + eps)) - 1 + 2 u32.
  mean(dv^2) matters for a constant row far from zero, where the computed v is all rounding error of the mean.
* under_x = 2 |x| where the fp64 sigmoid or |x| itself is below 2^-120 (as tests/bf16_dense_ref.py): there expf
  overflows or 1 / (1 + e) is subnormal, and the kernel returns anything between 0 and the value.  Only the saturate
  family needs it (tests/test_dense_f32_bounds.py asserts that, and that it covers under 5 % of its elements).

The non-linear outputs are given an S too, so that every output has one form of q: for g and (dA | dB) the part of
the bound that comes through the chain (|silu' b| S_a + |a s| S_b; |b silu'| S_G, |a s| S_G) plus the remaining terms --
a fixed number of roundings, whatever K is -- in units of u32; for rstd the bound without its absolute terms over
gamma_n.  The chain and the fixed part are kept apart because an earlier form, S = bound / gamma_n for all of it, makes
q = n x the hard ratio wherever the fixed terms dominate: the SwiGLU backward on the MI355X stood at 0.25-0.28 of its
hard bound at K = 40 and at K = 256 alike, which that form turned into q = 10 and q = 77 (1.6 x a limit taken from a
K = 40 emulation).  That was a finding about the checker, not the kernel: the error there is the four roundings of
silu', which do not grow with K.  The emulation now also runs K = 256 / 260 for both SwiGLU epilogues.

Tight tier.  q = (|got - ref| - the absolute terms) / (u32 S) is held to TIGHT_FACTOR x the worst q that the f32 CPU
emulation of tests/test_dense_f32_bounds.py (the kernel's chain: lane-half and step order, chunks, folds) reaches for
that kernel over every family and shape class: Q_EMU below, asserted there, measured from the emulation and never from
the kernel.  Where it carries weight: the limit is 4 Q_EMU u32 S against gamma_n S, so it is the tighter tier only for
n > 4 Q_EMU -- the GEMMs (n >= 100 on the walk; at K = 36 the two tiers nearly meet), the weight gradient (n > 128:
from two steps per chunk on), the bias gradient.  It adds nothing to the hard tier for the row_stats mean at NCH = 1 (n = 12
against 14.4; it does at NCH = 4 and 16, n = 24 and 72), for rstd (the limit is 57.6 / n of the hard bound, above it
for every NCH), for contractions shorter than about 20, and for
g and (dA | dB) wherever the fixed terms dominate (there q is the hard ratio, and 4 Q_EMU is above 1).

Measured on the MI355X (256 CUs), worst over tests/test_dense_f32_bounds_gpu.py and tests/test_dense_gpu.py -- hard
ratio, q / (4 Q_EMU):
    nt 0.199, 0.253          nt_walk 0.066, 0.500      nt_swiglu 0.067, 0.555
    nn 0.162, 0.268          nn_swiglu_bwd 0.382, 0.441
    tn dw 0.105, 0.120       tn db 0.153, 0.590
    row_stats mean 0.205, 0.342     row_stats rstd 0.648, 0.184
No fault was found in csrc/gemm_f32.hip: every guard stayed untouched, every bitwise invariant held, AMK_DENSE_WALK=0
and AMK_DENSE_STAGGER=3,2 gave the default's bits and AMK_DENSE_BK=16 and AMK_DENSE_TN_SLOTS=6 stayed inside both tiers.

Input families: unit, outlier_rows (rows 0 and M // 2 at 64x and 16x), binade (rows and columns by powers of two over
2^-12 .. 2^12), cancel (the second half of the contraction nearly negates the first; SwiGLU backward: gate values
around the zero of silu'); for the LayerNorm fold and row_stats also offset (a stream at 1e3 +- 50 with a spread of
about 1), constant (variance 0), spike (one element per row 1e4 x the rest); for SwiGLU also saturate (gate
pre-activations over +-100 up to +-300, where expf overflows or underflows).
"""
import torch

U32 = 2.0 ** -24
FTZ = 2.0 ** -126
TINY = 2.0 ** -120
TIGHT_FACTOR = 4.0
F64 = torch.float64
GEMM_FAMILIES = ("unit", "outlier_rows", "binade", "cancel")
LN_FAMILIES = ("unit", "outlier_rows", "binade", "offset", "constant", "spike")
SWIGLU_FAMILIES = GEMM_FAMILIES + ("saturate",)
LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))   # the f32 eps the kernel adds

# worst q of the f32 emulation per kernel (tests/test_dense_f32_bounds.py::test_emulation_defines_q)
Q_EMU = {"nt": 5.3, "nt_walk": 4.4, "nt_swiglu": 1.42, "nn": 5.0, "nn_swiglu_bwd": 1.78, "tn_dw": 32.0, "tn_db": 1.36,
         "row_stats_mean": 3.6, "row_stats_rstd": 14.4}


def gamma(n):
    n = torch.as_tensor(n, dtype=F64)
    return n * U32 / (1 - n * U32)


def hard_bound(n, S):
    return float(gamma(n)) * S + n * FTZ


def chain(L):
    return L + 1


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _d(t):
    return None if t is None else t.detach().to(F64)


def _out(R, name, ref, n, S, absolute=None, lin=None):
    """One output: reference, (n, S), the absolute allowance (flush-to-zero, under) and the hard bound gamma_n S (or
    `lin`, for the non-linear outputs) + the absolute allowance."""
    ab = torch.full_like(ref, n * FTZ) if absolute is None else absolute + n * FTZ
    R[name], R["n_" + name], R["S_" + name], R["abs_" + name] = ref, n, S, ab
    R["bound_" + name] = (float(gamma(n)) * S if lin is None else lin) + ab
    return R


def _mixed(n, chain_S, lin):
    """S of a non-linear output whose bound `lin` is gamma_n chain_S plus terms of a fixed number of roundings: the chain
    part as it is, the rest in units of u32, so that q does not grow with n where the fixed terms dominate."""
    return chain_S + (lin - float(gamma(n)) * chain_S).clamp_min(0) / U32


# ---------------------------------------------------------------------------------------------- references
def ln_apply(a, ln):
    """(a', |a'| bound, 3 if folded) in fp64 from the f32 (mean, rstd, gamma, beta) handed to the GEMM."""
    A = _d(a)
    if ln is None:
        return A, A.abs(), 0
    mean, rstd, gam, bet = (_d(t) for t in ln)
    t = (A - mean.view(-1, 1)) * rstd.view(-1, 1) * gam
    return t + bet, t.abs() + bet.abs(), 3


def _nt(a, w, bias, resid, ln, extra):
    A, Aa, nl = ln_apply(a, ln)
    W = _d(w)
    C, S = A @ W.t(), Aa @ W.abs().t()
    if bias is not None:
        C, S = C + _d(bias), S + _d(bias).abs()
    if resid is not None:
        C, S = C + _d(resid), S + _d(resid).abs()
    absolute = 3 * FTZ * W.abs().sum(1).expand_as(C) if nl else None
    return C, S, a.shape[1] + extra + nl, absolute


def ref_nt(a, w, bias=None, resid=None, ln=None, name="c", R=None):
    """dense.gemm_nt with one projection: {"c", "S_c", "n_c", "abs_c", "bound_c"}."""
    C, S, n, ab = _nt(a, w, bias, resid, ln, 3)
    return _out({} if R is None else R, name, C, n, S, ab)


def ref_nt2(a, w, bias, w2, bias2, ln=None):
    """dense.gemm_nt with w2: outputs "c" and "c2"."""
    return ref_nt(a, w2, bias2, None, ln, "c2", ref_nt(a, w, bias, None, ln))


def _eps_s(s):
    return (1 - s) * 2 * U32 + 2 * U32


def _under(x, s):
    return torch.where((s < TINY) | (x.abs() < TINY), 2 * x.abs(), torch.zeros_like(x))


def ref_nt_swiglu(a, w12, b12=None, ln=None):
    """dense.gemm_nt_swiglu: outputs "g" (M, H) and "ab" (M, 2H)."""
    AB, S, n, ab0 = _nt(a, w12, b12, None, ln, 2)
    R = _out({}, "ab", AB, n, S, ab0)
    H = AB.shape[1] // 2
    e = float(gamma(n)) * S + R["abs_ab"]
    x, y, ex, ey = AB[:, :H], AB[:, H:], e[:, :H], e[:, H:]
    s = torch.sigmoid(x)
    g = x * s * y
    sp = s * (1 + x * (1 - s))
    lin = (sp * y).abs() * ex + (x * s).abs() * ey + g.abs() * (_eps_s(s) + 2 * U32) + 0.25 * ex * ex * y.abs() + ex * ey
    R["under_g"] = _under(g, s)
    return _out(R, "g", g, n, _mixed(n, (sp * y).abs() * S[:, :H] + (x * s).abs() * S[:, H:], lin), R["under_g"], lin)


def ref_nn(a, w, a2=None, w2=None):
    """dense.gemm_nn: output "c"."""
    A, W = _d(a), _d(w)
    C, S, K = A @ W, A.abs() @ W.abs(), a.shape[1]
    if a2 is not None:
        A2, W2 = _d(a2), _d(w2)
        C, S, K = C + A2 @ W2, S + A2.abs() @ W2.abs(), K + a2.shape[1]
    return _out({}, "c", C, chain(K), S)


def ref_nn_swiglu_bwd(dy, w3, ab):
    """dense.gemm_nn(swiglu_ab=): output "dab" (M, 2H) = (dA | dB)."""
    G0 = ref_nn(dy, w3)
    G, eG, n = G0["c"], G0["bound_c"], G0["n_c"]
    AB = _d(ab)
    H = G.shape[1]
    A, B = AB[:, :H], AB[:, H:]
    s = torch.sigmoid(A)
    eps_s = _eps_s(s)
    sp = s * (1 + A * (1 - s))
    E_sp = s * ((1 + A - 2 * A * s).abs() * eps_s + 2 * U32 * A.abs() * (1 - s) + U32 * (1 + A * (1 - s)).abs()) + U32 * sp.abs()
    da, db = G * B * sp, G * A * s
    lda = (B * sp).abs() * eG + (G * B).abs() * E_sp + 2 * U32 * da.abs() + B.abs() * eG * E_sp
    ldb = (A * s).abs() * eG + db.abs() * (eps_s + 2 * U32) + (A * s).abs() * eG * (eps_s + 2 * U32)
    under = torch.cat([_under(da, s), _under(db, s)], 1)
    R = {"under_dab": under}
    lin = torch.cat([lda, ldb], 1)
    chain_S = torch.cat([(B * sp).abs(), (A * s).abs()], 1) * G0["S_c"].repeat(1, 2)
    return _out(R, "dab", torch.cat([da, db], 1), n, _mixed(n, chain_S, lin), under, lin)


def ref_tn(y, x, y2=None, ln=None, want_bias=True, spc=1, nchunk=1, bk=32):
    """dense.gemm_tn: outputs "dw", "dw2" (with y2) and "db" (N1 + N2) for the chunking (spc, nchunk) that
    expected_path gives for the launch."""
    X, Xa, nl = ln_apply(x, ln)
    n = bk * spc + 1 + nchunk + nl
    R = {}
    ys = [("dw", y)] + ([("dw2", y2)] if y2 is not None else [])
    for name, yy in ys:
        Y = _d(yy)
        _out(R, name, Y.t() @ X, n, Y.abs().t() @ Xa, 3 * FTZ * Y.abs().sum(0).view(-1, 1).expand(Y.shape[1], X.shape[1]) if nl else None)
    if want_bias:
        Y = torch.cat([_d(t) for _, t in ys], 1)
        _out(R, "db", Y.sum(0), bk * spc // 8 + 8 + nchunk, Y.abs().sum(0))
    return R


def stats_nch(D):
    """The NCH instance of row_stats_kernel that amk_row_stats launches."""
    return 1 if D <= 256 else (4 if D <= 1024 else 16)


def ref_row_stats(x, eps=LN_EPS):
    """dense.row_stats: outputs "mean" and "rstd" (M,)."""
    X = _d(x)
    D = X.shape[1]
    nl = 4 * stats_nch(D) + 6
    mean = X.mean(1)
    R = _out({}, "mean", mean, nl + 2, X.abs().mean(1))
    dmean = R["bound_mean"].view(-1, 1)
    v = X - mean.view(-1, 1)
    dv = dmean + U32 * (v.abs() + dmean)
    var = (v * v).mean(1)
    dv2 = (dv * dv).mean(1)
    dvar = 2 * (v.abs() * dv).mean(1) + dv2 + float(gamma(nl + 4)) * (var + dv2) + U32 * (var + eps)
    r = (dvar / (var + eps)).clamp(max=0.99)
    eps_r = 1 / torch.sqrt(1 - r) - 1 + 2 * U32
    rstd = 1 / torch.sqrt(var + eps)
    n = nl + 6
    return _out(R, "rstd", rstd, n, rstd * eps_r / float(gamma(n)))


# ---------------------------------------------------------------------------------------------- checking
WORST = {}   # kernel -> [worst hard ratio, worst q / (TIGHT_FACTOR Q_EMU)] over every check of the process


def measures(got, R, name):
    """(elements outside the hard bound, worst |err| / hard bound, worst q) over every element."""
    ref = R[name]
    a = got.detach().to(ref.device, F64).reshape(ref.shape)
    err = (a - ref).abs()
    hb, S, ab = R["bound_" + name], R["S_" + name], R["abs_" + name]
    bad = ~(err <= hb)                                           # (a NaN result is outside the bound too)
    zero = torch.zeros_like(err)
    ratio = torch.where(err > 0, err / hb, zero)
    q = torch.where((err > 0) & (S > 0), (err - ab).clamp_min(0) / (U32 * S), zero)
    q = torch.where((err > ab) & ~(S > 0), torch.full_like(q, float("inf")), q)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return int(bad.sum()), float(ratio.max()) if a.numel() else 0.0, float(q.max()) if a.numel() else 0.0


def violations(got, R, name, kernel=None):
    """Number of elements that miss the hard tier, plus 1 if the tight tier (kernel given) is missed."""
    nbad, _, q = measures(got, R, name)
    return nbad + (1 if kernel is not None and q > TIGHT_FACTOR * Q_EMU[kernel] else 0)


def assert_within(got, R, name, kernel, what=""):
    """Both tiers on every element; records the worst figures in WORST[kernel]."""
    nbad, ratio, q = measures(got, R, name)
    lim = TIGHT_FACTOR * Q_EMU[kernel]
    w = WORST.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], q / lim)
    print(f"{what} {name} [{kernel}]: hard ratio {ratio:.4g}, q {q:.4g} (limit {lim:.4g})")
    assert nbad == 0, f"{what} {name}: {nbad} elements outside the hard bound (worst {ratio:.3g}x)"
    assert q <= lim, f"{what} {name}: q = |err| / (u32 S) reaches {q:.3g}, limit {lim:.3g} ({TIGHT_FACTOR} x the emulation)"


# ---------------------------------------------------------------------------------------------- input families
def _row_scale(M, family, g):
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


def make_act(family, M, K, seed, with_scale=False):
    """Activations (M, K) of a family (every family of GEMM_FAMILIES and LN_FAMILIES); with_scale: and the (M, 1) row
    factors."""
    g = _gen(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    rs = _row_scale(M, family, g)
    a = n(M, K) * rs
    if family == "cancel":
        h = K // 2
        a[:, h:2 * h] = a[:, :h]
    elif family == "offset":
        a = 1000.0 + 50.0 * n(M, 1) + a
    elif family == "constant":
        a = (4.0 * n(M, 1)).expand(M, K).clone()
    elif family == "spike":
        a[torch.arange(M), torch.randint(0, K, (M,), generator=g)] = 1e4 * torch.sign(n(M))
    return (a.contiguous(), rs) if with_scale else a.contiguous()


def make_nt(family, M, N, K, seed):
    """a (M, K), w (N, K), bias (N,), resid (M, N), gamma, beta (K,): f32."""
    g = _gen(seed + 1)
    n = lambda *s: torch.randn(*s, generator=g)
    a, rs = make_act(family, M, K, seed, True)
    cs = _col_scale(N, family, g)
    w = n(N, K) * K ** -0.5 * cs.view(N, 1)
    bias = n(N) * cs
    resid = n(M, N) * rs * cs                     # (the residual of a row is of the row's scale)
    if family == "cancel":
        h = K // 2
        w[:, h:2 * h] = -w[:, :h] + n(N, h) * K ** -0.5 / 64
        bias, resid = bias / 64, resid / 64
    return {"a": a, "w": w.contiguous(), "bias": bias, "resid": resid.contiguous(), "gamma": n(K) * 0.5 + 1.0, "beta": n(K)}


def _saturated(H, g):
    """(H,) gate offsets of the saturate family: H // 32 columns (at least one) at -100 .. -300, where expf overflows and
    the sigmoid is below 2^-120, H // 4 at +100 .. +300, where expf underflows; zeros elsewhere."""
    nneg, npos = max(1, H // 32), H // 4
    off = torch.zeros(H)
    cols = torch.randperm(H, generator=g)
    off[cols[:nneg]] = -torch.linspace(100.0, 300.0, nneg)
    off[cols[nneg:nneg + npos]] = torch.linspace(100.0, 300.0, npos)
    return off


def make_swiglu(family, M, H, K, seed):
    """make_nt with w = w12 (2H, K) and bias = b12.  The gate pre-activations stay inside +-80 except on saturate (gate
    biases beyond +-100, see _saturated): outlier_rows divides the gate weights by 8, binade moves the row scales of a
    and the gate columns' scales to 2^-24 .. 1."""
    D = make_nt("unit" if family == "saturate" else family, M, 2 * H, K, seed)
    if family == "saturate":
        D["bias"][:H] += _saturated(H, _gen(seed + 2))
    elif family == "outlier_rows":
        D["w"][:H] /= 8
    elif family == "binade":
        D["a"] *= 2.0 ** -12
        D["w"][:H] *= 2.0 ** -12
        D["bias"][:H] *= 2.0 ** -12
    return D


def make_nn(family, M, N, K, seed, K2=0):
    """a (M, K), w (K, N) and with K2 a2 (M, K2), w2 (K2, N)."""
    D = make_nt(family, M, N, K + K2, seed)
    a, w = D["a"], D["w"].t().contiguous()
    out = {"a": a[:, :K].contiguous(), "w": w[:K].contiguous()}
    if K2:
        out["a2"], out["w2"] = a[:, K:].contiguous(), w[K:].contiguous()
    return out


def make_swiglu_bwd(family, M, H, K, seed):
    """dy (M, K), w3 (K, H), ab (M, 2H): cancel puts the gate around the zero of silu', saturate beyond +-100 (as
    make_swiglu; the other families keep it inside +-80)."""
    D = make_nn("unit" if family == "saturate" else family, M, H, K, seed)
    g = _gen(seed + 3)
    ab = torch.randn(M, 2 * H, generator=g) * _row_scale(M, family, g)
    if family == "binade":
        ab = ab * _col_scale(2 * H, family, g)
        ab[:, :H] *= 2.0 ** -24
    elif family == "outlier_rows":
        ab[:, :H] /= 8
    elif family == "cancel":
        ab[:, :H] = -1.0 - 0.5 * torch.rand(M, H, generator=g)
    elif family == "saturate":
        ab[:, :H] += _saturated(H, g)
    return {"dy": D["a"], "w3": D["w"], "ab": ab.contiguous()}


def make_tn(family, M, N, K, seed, N2=0):
    """y (M, N), x (M, K), gamma, beta (K,) and with N2 y2 (M, N2).  The LayerNorm families shape x."""
    g = _gen(seed + 4)
    n = lambda *s: torch.randn(*s, generator=g)
    r = _row_scale(M, family, g)
    y = n(M, N + N2) * r * _col_scale(N + N2, family, g)
    x = make_act(family, M, K, seed) * (_col_scale(K, family, g) if family == "binade" else 1.0)
    if family == "cancel":
        h = M // 2
        x = n(M, K)
        x[h:2 * h] = x[:h]
        y[h:2 * h] = -y[:h] + n(h, N + N2) / 64
    out = {"y": y[:, :N].contiguous(), "x": x.contiguous(), "gamma": n(K) * 0.5 + 1.0, "beta": n(K)}
    if N2:
        out["y2"] = y[:, N:].contiguous()
    return out


# ---------------------------------------------------------------------------------------------- dispatch restatement
def tn_chunks(M, N, K, cus=256, bk=32, tn_slots=0):
    """(nchunk, steps_per_chunk) as tn_chunks() of csrc/gemm_f32.hip picks them."""
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    steps = (M + bk - 1) // bk
    min_steps = 256 // bk
    wg = (3 if bk == 16 else 2) * cus
    slots = tn_slots if tn_slots else (wg // 2 if tiles <= 16 else wg)
    chunks = max(1, slots // tiles)
    if chunks > steps // min_steps:
        chunks = max(1, steps // min_steps)
    spc = (steps + chunks - 1) // chunks
    return (steps + spc - 1) // spc, spc


def expected_path(op, epilogue, M, N, K, split=0, ln=False, cus=256, bk=32, walk=True, tn_slots=0):
    """The kernel and launch geometry the host code of csrc/gemm_f32.hip picks.  op: "nt", "nn", "tn", "row_stats"
    (N = D); epilogue: "bias", "resid", "swiglu" (N = H), "swiglu_bwd".  Returns {"kernel", "instance", "tiles", "grid",
    "max_tiles", "min_tiles" (tiles per workgroup), "nchunk", "steps_per_chunk", "nch"}."""
    P = {"kernel": op, "tiles": 0, "grid": 0, "max_tiles": 1, "min_tiles": 1, "nchunk": 0, "steps_per_chunk": 0, "nch": 0}
    mt = (M + 127) // 128
    if op == "row_stats":
        P.update(nch=stats_nch(N), grid=min((M + 3) // 4, 16384), instance=f"row_stats<{stats_nch(N)}>")
        P["max_tiles"] = -(-((M + 3) // 4) // P["grid"])
        return P
    if op == "nt":
        sw = epilogue == "swiglu"
        ntn = (N + 63) // 64 if sw else (split // 128 + (N - split + 127) // 128 if split else (N + 127) // 128)
        tiles = mt * ntn
        slots = (3 if bk == 16 else 2) * cus
        use_walk = bool(walk) and bk != 16 and K > 96
        grid = min(tiles, slots) if use_walk else tiles
        P.update(kernel="nt_walk" if use_walk else "nt", tiles=tiles, grid=grid, max_tiles=-(-tiles // grid), min_tiles=tiles // grid)
        P["instance"] = (f"nt_walk<{epilogue},{int(ln)}>" if use_walk else f"nt<{bk},{epilogue},{int(ln)}>")
        return P
    if op == "nn":
        tiles = mt * ((N + 127) // 128)
        P.update(tiles=tiles, grid=tiles, instance=f"nn<{bk},{epilogue}>")
        return P
    assert op == "tn", op
    nchunk, spc = tn_chunks(M, N, K, cus, bk, tn_slots)
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    P.update(tiles=tiles, grid=tiles * nchunk, nchunk=nchunk, steps_per_chunk=spc, instance=f"tn<{bk},{int(ln)}>")
    return P
