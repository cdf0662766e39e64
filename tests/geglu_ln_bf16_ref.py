"""fp64 reference, per-element error bounds and a CPU emulation in the kernels' own order for the fused gate + LayerNorm
of the transformer FFN under bf16 autocast, csrc/geglu_ln_bf16.hip (amk_geglu_ln_bf16_fwd / _bwd, ops.geglu_ffn inside
torch.autocast("cuda", bfloat16)).

Semantics (include/amk.h).  ab (M, 2H) bf16 = (val | gate), gamma, beta (H) f32, dy (M, H) bf16:
    g = gelu(val) gate, gelu(v) = v Phi(v) = 0.5 v (1 + erf(v / sqrt 2));   mean = mean_j g,  var = mean_j (g - mean)^2,
    rstd = (var + eps)^-1/2,  xhat = (g - mean) rstd,  y = xhat gamma + beta                      (y rounded to bf16 once)
    dg = rstd (dy gamma - c1 - xhat c2),  c1 = mean_j(dy gamma),  c2 = mean_j(dy gamma xhat)
    d_ab = (dg gate gelu'(val) | dg gelu(val)),  gelu'(v) = Phi(v) + v phi(v)                  (d_ab rounded to bf16 once)
    dgamma = sum_rows dy xhat,  dbeta = sum_rows dy                                                              (f32)
The reference is fp64 on the bf16 values of ab and dy and the f32 gamma / beta; y's gradients are torch.autograd's.

Bounds.  u = 2^-8 (the project's bf16 unit: a rounding to bf16 is charged 2 u |ref|, tests/bf16_dense_ref.py), w = 2^-24
(f32), gamma_n = n w / (1 - n w).  Every E below is an absolute bound on |computed - exact| of the f32 quantity.

g.  erf's argument v c (c = f32(1 / sqrt 2)) carries 2 w relatively; |x erf'(x)| <= 0.49, so that moves erf by at most w.
erff itself is charged E_ERF = 16 ulp (the OpenCL full-profile limit the device math library is held to), 32 w absolutely
since |erf| <= 1.  fl(1 + e) = (1 + e)(1 + d) + D with |d| <= w and |D| <= 33 w.  D is ABSOLUTE: for negative val, 1 + erf
cancels, so no relative bound on gelu holds there.  Two more products (by 0.5 v, exact halving, and by gate):
    E_g = w (4 |g| + 17 |val gate|)                    c1 = 4 >= gamma_3 / w,  c2 = 17 >= 0.5 * 33 (1 + 3 w)
gelu(val) alone (the gate half of d_ab):   E_ge = w (3 |gelu| + 17 |val|).
gelu'.  Phi-part 0.5 fl(1 + e): 17 w + w Phi.  v phi(v) as v * k * expf(-0.5 v^2): the argument's rounding moves exp by
0.5 v^2 w relatively, expf is charged 4 ulp (8 w), k and two products 3 w:
    E_gp = w (18 + (0.5 v^2 + 11) |v| phi(v) + |gelu'|).

Row sums.  A thread adds its <= 16 elements in order, the wave reduces by a 6-level butterfly, four waves add in order, and
the sum is scaled by an f32 1 / H: no partial sum passes through more than N_SUM = 16 + 6 + 3 + 3 = 28 roundings, for
every H <= 4096.
    E_mean = mean_j E_g + gamma_28 (mean_j |g| + mean_j E_g)
    E_d    = E_g + E_mean + w |d|                                                d = g - mean, kept in registers
    E_var  = 2 mean_j(|d| E_d) + mean_j(E_d^2) + gamma_30 (var + the two terms before)    (the squares add two roundings)
    rho    = delta / (2 (1 - delta)) + 5 w,   delta = E_var / (var + eps)   (relative error of rstd: the add, v_rsq_f32
             at 1 ulp, eps as an f32; |(1 + t)^-1/2 - 1| <= |t| / (2 (1 - |t|)); no bound (inf) once delta >= 0.9)
    bound(mean) = E_mean,   bound(rstd) = rstd rho.

y = fl(fl(fl(d rstd) gamma) + beta):
    E_y32 = |gamma| rstd (1 + rho) E_d + |xhat gamma| (rho + 3 w) + w |y|
    bound(y) = 2 u |y| + (1 + 2 u) E_y32.

Backward (it reads the forward's f32 mean and rstd, so their errors are those above):
    E_xh    = rstd (1 + rho) E_d + |xhat| (rho + 2 w)
    gy = fl(dy gamma): w |gy|;   E_c1 = gamma_29 mean_j |gy|;   E_c2 = mean_j(|gy| E_xh) + gamma_30 mean_j |gy xhat|
    E_inner = w |gy| + E_c1 + |c2| E_xh + |xhat| E_c2 + 3 w (|gy| + |c1| + |xhat c2|)
    E_dg    = rstd (1 + rho) E_inner + |dg| (rho + w)
    val half:   A = gate gelu'(val),  E_A = |gate| E_gp + w |A|,   E32 = E_dg (|A| + E_A) + |dg| E_A + w |d_val|
    gate half:  B = gelu(val),        E_B = E_ge,                  E32 = E_dg (|B| + E_B) + |dg| E_B + w |d_gate|
    bound(d_ab) = 2 u |d_ab| + (1 + 2 u) E32
    bound(dgamma) = gamma_(M+2) sum_rows |dy xhat| + sum_rows |dy| E_xh        (any order of M products, f32 throughout)
    bound(dbeta)  = gamma_M sum_rows |dy|.
Every bound gets the floor 1e-5 max |ref| of its tensor, as elsewhere in the project.

The constants are derived, not fitted: tests/test_geglu_ln_bf16_bounds.py holds the CPU emulation below (f32 torch ops in
the kernels' order, bf16 roundings where the kernels round) under HALF of every bound on every family, and shows that
planted defects fall outside.

Measured on the MI355X, worst |got - ref| / bound over tests/test_geglu_ln_bf16_gpu.py:
    y 0.496    d_ab 0.494    mean 0.013    rstd 0.008    dgamma 0.013    dbeta 0.002
(y and d_ab sit just under 0.5: the bound charges a bf16 rounding 2 u = 2^-7, the rounding itself is at most 2^-8.)
"""
import math

import torch

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
U16 = 2.0 ** -8
U32 = 2.0 ** -24
EPS = 1e-5
FLOOR = 1e-5
N_SUM = 28
FAMILIES = ("diffuse", "wide", "flat_rows", "large")
TENSORS = ("y", "mean", "rstd", "d_ab", "dgamma", "dbeta")
MAX_PARTS = 512

# worst |got - ref| / bound per tensor over everything `ratios` has seen in this process
WORST = {}


def gamma_n(n):
    return n * U32 / (1.0 - n * U32)


# ---------------------------------------------------------------------------------------------- inputs
def make_inputs(family, M, H, seed=0):
    """(ab (M, 2H) bf16, dy (M, H) bf16, gamma (H) f32, beta (H) f32) on the CPU; beta is nonzero."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + H + 13 * FAMILIES.index(family))
    val = torch.randn(M, H, generator=gen)
    gate = torch.randn(M, H, generator=gen)
    if family == "wide":
        val = (torch.rand(M, H, generator=gen) * 2 - 1) * 12       # both tails of the GELU
    elif family == "flat_rows":
        cv = torch.randn(M, 1, generator=gen).expand(M, H)
        cg = torch.randn(M, 1, generator=gen).expand(M, H)
        r = torch.arange(M)[:, None]
        val = torch.where(r % 3 == 0, torch.zeros_like(val), torch.where(r % 3 == 1, cv, val))
        gate = torch.where(r % 3 == 0, torch.zeros_like(gate), torch.where(r % 3 == 1, cg, gate))
    elif family == "large":
        # g = gelu(4) * {256, 258} = 1023.97 or 1031.96: a mean of 10^3 with a deviation of a few units
        val = torch.full((M, H), 4.0)
        odd = torch.rand(M, H, generator=gen) < 0.05
        odd |= torch.arange(H)[None, :] == (torch.arange(M)[:, None] % H)
        gate = torch.where(odd, torch.full((M, H), 258.0), torch.full((M, H), 256.0))
    ab = torch.cat([val, gate], dim=1).to(BF16).contiguous()
    dy = torch.randn(M, H, generator=gen).to(BF16).contiguous()
    gamma = (0.5 + torch.rand(H, generator=gen)).to(F32)
    beta = (torch.rand(H, generator=gen) + 0.25).to(F32) * torch.where(torch.rand(H, generator=gen) < 0.5, -1.0, 1.0)
    return ab, dy, gamma, beta


def zero_rows(family, M):
    """Rows of `flat_rows` whose ab is all zero."""
    return [r for r in range(M) if r % 3 == 0] if family == "flat_rows" else []


# ---------------------------------------------------------------------------------------------- reference
def _phi(v):
    return torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)


def reference(ab, dy, gamma, beta, eps=EPS):
    """{name: fp64 reference, "bound_" + name: per-element bound} for name in TENSORS, on ab's device."""
    ab64 = ab.detach().to(F64).requires_grad_(True)
    gm = gamma.detach().to(F64).requires_grad_(True)
    bt = beta.detach().to(F64).requires_grad_(True)
    D = dy.detach().to(F64)
    M, H = D.shape
    v, t = ab64.chunk(2, dim=-1)
    y = torch.nn.functional.layer_norm(t * torch.nn.functional.gelu(v), (H,), gm, bt, eps)
    y.backward(D)
    R = {"y": y.detach(), "d_ab": ab64.grad, "dgamma": gm.grad, "dbeta": bt.grad}

    w = U32
    with torch.no_grad():
        v, t, gm, bt = v.detach(), t.detach(), gm.detach(), bt.detach()
        Phi = 0.5 * (1 + torch.erf(v / math.sqrt(2)))
        ge = v * Phi
        gp = Phi + v * _phi(v)
        g = ge * t
        mean = g.mean(1, keepdim=True)
        d = g - mean
        var = (d * d).mean(1, keepdim=True)
        rstd = (var + eps) ** -0.5
        xh = d * rstd
        R["mean"], R["rstd"] = mean[:, 0], rstd[:, 0]

        E_g = w * (4 * g.abs() + 17 * (v * t).abs())
        E_ge = w * (3 * ge.abs() + 17 * v.abs())
        E_gp = w * (18 + (0.5 * v * v + 11) * (v * _phi(v)).abs() + gp.abs())
        EGm = E_g.mean(1, keepdim=True)
        E_mean = EGm + gamma_n(N_SUM) * (g.abs().mean(1, keepdim=True) + EGm)
        E_d = E_g + E_mean + w * d.abs()
        E_var = 2 * (d.abs() * E_d).mean(1, keepdim=True) + (E_d * E_d).mean(1, keepdim=True)
        E_var = E_var + gamma_n(N_SUM + 2) * (var + E_var)
        delta = E_var / (var + eps)
        rho = torch.where(delta < 0.9, delta / (2 * (1 - delta.clamp(max=0.9))) + 5 * w, torch.full_like(delta, float("inf")))
        E_y32 = gm.abs() * rstd * (1 + rho) * E_d + (xh * gm).abs() * (rho + 3 * w) + w * R["y"].abs()
        B = {"mean": E_mean[:, 0], "rstd": (rstd * rho)[:, 0], "y": 2 * U16 * R["y"].abs() + (1 + 2 * U16) * E_y32}

        E_xh = rstd * (1 + rho) * E_d + xh.abs() * (rho + 2 * w)
        gy = D * gm
        c1 = gy.mean(1, keepdim=True)
        c2 = (gy * xh).mean(1, keepdim=True)
        E_c1 = gamma_n(N_SUM + 1) * gy.abs().mean(1, keepdim=True)
        E_c2 = (gy.abs() * E_xh).mean(1, keepdim=True) + gamma_n(N_SUM + 2) * (gy * xh).abs().mean(1, keepdim=True)
        E_in = w * gy.abs() + E_c1 + c2.abs() * E_xh + xh.abs() * E_c2 + 3 * w * (gy.abs() + c1.abs() + (xh * c2).abs())
        dg = rstd * (gy - c1 - xh * c2)
        E_dg = rstd * (1 + rho) * E_in + dg.abs() * (rho + w)
        A = t * gp
        E_A = t.abs() * E_gp + w * A.abs()
        dval, dgate = dg * A, dg * ge
        E_val = E_dg * (A.abs() + E_A) + dg.abs() * E_A + w * dval.abs()
        E_gate = E_dg * (ge.abs() + E_ge) + dg.abs() * E_ge + w * dgate.abs()
        B["d_ab"] = 2 * U16 * R["d_ab"].abs() + (1 + 2 * U16) * torch.cat([E_val, E_gate], dim=1)
        B["dgamma"] = gamma_n(M + 2) * (D * xh).abs().sum(0) + (D.abs() * E_xh).sum(0)
        B["dbeta"] = gamma_n(M) * D.abs().sum(0)
        for name in TENSORS:
            floor = FLOOR * float(R[name].abs().max()) if R[name].numel() else 0.0
            R["bound_" + name] = B[name] + floor
    return R


def ratios(got, R, names=TENSORS, record=True):
    """{name: worst |got - ref| / bound}; a non-finite value counts as inf."""
    out = {}
    for name in names:
        x = got[name].detach().to(F64).to(R[name].device).reshape(R[name].shape)
        q = (x - R[name]).abs() / R["bound_" + name]
        q = torch.where(torch.isfinite(x), q, torch.full_like(q, float("inf")))
        out[name] = float(q.max()) if q.numel() else 0.0
        if record:
            WORST[name] = max(WORST.get(name, 0.0), out[name])
    return out


# ---------------------------------------------------------------------------------------------- CPU emulation
def dispatch(H):
    """(chunks per thread, waves per row) as csrc/geglu_ln_bf16.hip dispatches the widths."""
    return (1, 1) if H <= 512 else (2, 1) if H <= 1024 else (1, 4) if H <= 2048 else (2, 4)


def num_partials(M, H):
    rpw = 4 // dispatch(H)[1]
    return min((M + rpw - 1) // rpw, MAX_PARTS)


def _row_sum(x, H):
    """Row sums of x (M, H) f32 in the kernel's order: thread t owns the 8-element chunks t, t + T, ...; it adds them in
    order, the wave butterflies (xor 32 ... 1), the waves add in order."""
    nchk, wpr = dispatch(H)
    T = 64 * wpr
    M = x.shape[0]
    pad = torch.zeros(M, nchk * T * 8, dtype=F32)
    pad[:, :H] = x
    pad = pad.view(M, nchk, T, 8)
    s = torch.zeros(M, T, dtype=F32)
    for j in range(nchk):
        for e in range(8):
            s = s + pad[:, j, :, e]
    s = s.view(M, wpr, 64)
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ o]
    tot = s[:, 0, 0]
    for k in range(1, wpr):
        tot = tot + s[:, k, 0]
    return tot[:, None]


def _gelu_parts(v):
    e = torch.erf(v * torch.tensor(0.70710678118654752, dtype=F32))
    return (0.5 * v) * (1 + e), e


def emulate(ab, dy, gamma, beta, eps=EPS, mut=None):
    """{y bf16, mean, rstd, d_ab bf16, dgamma, dbeta} on the CPU: f32 torch ops in the kernels' order, bf16 roundings where
    the kernels round.  mut plants a defect: "swapped_halves", "tanh_bf16_twice" (g by the tanh GELU, rounded to bf16
    after the GELU and after the gate), "uncentred_variance" (E[g^2] - mean^2), "gamma_after_means" (backward: gamma
    applied to dg instead of inside the two row means), "dgamma_drops_last_row"."""
    M, H = dy.shape
    v, t = ab[:, :H].to(F32), ab[:, H:].to(F32)
    if mut == "swapped_halves":
        v, t = t, v
    D, gm, bt = dy.to(F32), gamma.to(F32), beta.to(F32)
    inv_h = torch.tensor(1.0, dtype=F32) / torch.tensor(float(H), dtype=F32)
    eps32 = torch.tensor(eps, dtype=F32)
    ge, e = _gelu_parts(v)
    if mut == "tanh_bf16_twice":
        ge = torch.nn.functional.gelu(v, approximate="tanh").to(BF16).to(F32)
        g = (ge * t).to(BF16).to(F32)
    else:
        g = ge * t
    mean = _row_sum(g, H) * inv_h
    d = g - mean
    if mut == "uncentred_variance":
        var = _row_sum(g * g, H) * inv_h - mean * mean
    else:
        var = _row_sum(d * d, H) * inv_h
    rstd = torch.rsqrt(var + eps32)
    y = ((d * rstd) * gm + bt).to(BF16)

    gp = 0.5 * (1 + e) + (v * torch.tensor(0.39894228040143268, dtype=F32)) * torch.exp(-0.5 * v * v)
    xh = (g - mean) * rstd
    if mut == "gamma_after_means":
        c1 = _row_sum(D, H) * inv_h
        c2 = _row_sum(D * xh, H) * inv_h
        dg = rstd * (D - c1 - xh * c2) * gm
    else:
        gy = D * gm
        c1 = _row_sum(gy, H) * inv_h
        c2 = _row_sum(gy * xh, H) * inv_h
        dg = rstd * (gy - c1 - xh * c2)
    d_ab = torch.cat([dg * (t * gp), dg * ge], dim=1).to(BF16)

    # dgamma / dbeta: a workgroup's wave takes the rows b * rpw + wave + k * grid * rpw in order; the waves add in order
    # (one wave when the workgroup shares a row); the partials are summed by torch.sum
    rpw = 4 // dispatch(H)[1]
    grid = num_partials(M, H)
    acc = torch.zeros(grid, rpw, 2, H, dtype=F32)
    last = M - 1 if mut == "dgamma_drops_last_row" else M
    for r in range(M):
        b, wv = (r // rpw) % grid, r % rpw
        if r < last:
            acc[b, wv, 0] = acc[b, wv, 0] + D[r] * xh[r]
        acc[b, wv, 1] = acc[b, wv, 1] + D[r]
    part = torch.zeros(grid, 2, H, dtype=F32)
    for wv in range(rpw):
        part = part + acc[:, wv]
    dgb = part.sum(0)
    return {"y": y, "mean": mean[:, 0], "rstd": rstd[:, 0], "d_ab": d_ab, "dgamma": dgb[0], "dbeta": dgb[1]}
