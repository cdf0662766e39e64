"""fp64 references, per-element error bounds and input families for SwitchHeadAttention's experts under bf16 autocast:
the narrow grouped GEMMs and the bf16 per-expert sums of csrc/moe_bf16.hip (amk_grouped_gemm_nt64 / nn64 / wgrad64_bf16,
amk_moe_expert_sums_bf16) and ops._SharedRowExpertsBF16 / _SummedExpertsBF16 built on them.

House rules of tests/moe_bf16_ref.py: every reference is computed in fp64 ON THE VALUES THE KERNEL READS, bounds are per
element and derived from the kernel's own operation chain, no term is relative to a tensor's maximum, no element is
left out.  u32 = 2^-24, U = 2^-8 (one bf16 rounding), gamma_n = n u32 / (1 - n u32), flush term n 2^-126.

* nt64 / nn64 / wgrad64: the chains of the wide kernels -- the narrow tile only decides which wave and which
  accumulator register hold an element -- so moe_bf16_ref.ref_nt / ref_nn / ref_wgrad hold unchanged:
      nt  n = Kd + 1,  nn  n = N + 1:  gamma_n S + n 2^-126;   wgrad  n = cnt_e + 2:  (U with a scale) S + gamma_n S + n 2^-126.
  Tight tier of nt64 / nn64: q = (|err| - n 2^-126) / (u32 S) held to TIGHT_FACTOR x the worst q of the CPU emulation over
  every family and every case of THIS list (Q_EMU below, asserted in tests/test_switchhead_bf16_bounds.py).
* expert sums (expert_sums_bf16_kernel): per (row, expert, column) an f32 sum of at most `fan` terms scale x a in
  ascending pair order -- one rounded product (or one fused multiply-add) and one rounded add per term -- then ONE
  rounding to bf16 (within U / (1 + U) of the f32 sum, which is within (1 + gamma_fan) of S):
      |got - ref| <= (gamma_fan + U) S + fan 2^-126,   S = sum |scale a|.   No pair: S = 0, exactly zero.

Op level (x16 = bf16(x), W16 = bf16(W) or the optimizer's shadow, the f32 gate and the ids as amk_moe_topk returns them,
the lists of amk_moe_route_distinct: virtual pairs g E + e).  z, B_z: reference and bound of the bf16 sums Z16.
  The library's bf16 GEMM (Z16 @ W16): exact products, an f32 sum of K = E d terms in an order we do not know -- any order
  is within gamma_{K - 1} of sum |z| |w|, charged as n = K + 1 -- and ONE rounding of the result to bf16:
      lib(z, B_z, w) = B_z |w| + gamma_{K+1} S + U (|ref| + B_z |w| + gamma_{K+1} S) + (K + 1) 2^-126,  S = (|z| + B_z) |w|.
  _SharedRowExpertsBF16 (V experts; W (E, d, dim)):
      V    = nt64(x16, W16) per distinct (token, expert):  B_v
      out  = sum_j g_j V_j (combine_rows, 2 operations per slot): sum_j g_j B_v_j + gamma_2k sum_j g_j (|V_j| + B_v_j) + 2k 2^-126
      dlogits = g (1 - g) <dOut, V>:  hard_bound(d + 7, g (1 - g) sum |dOut| (|V| + B_v)) + g (1 - g) sum |dOut| B_v
      Z16  = sums of g dOut:  B_z;     dx = lib(z, B_z, W16 as (E d, dim))
      dW   = wgrad64(Z16, x16), no scale:  B_z^T |x16| + hard_bound(cnt_e + 2, (|z| + B_z)^T |x16|)
  _SummedExpertsBF16 (output experts; W (E, dim, d)):
      Z16  = sums of the rows a:  B_z;  out = lib(z, B_z, W16 as (E d, dim))
      D    = nn64(d16, W16), d16 = bf16(dOut):  B_D;   da = sum_j D_j (1 operation per slot):
             sum_j B_D_j + gamma_k sum_j (|D_j| + B_D_j) + k 2^-126
      dW   = wgrad64(d16, Z16), no scale:  |d16|^T B_z + hard_bound(cnt_e + 2, |d16|^T (|z| + B_z))
  A dx or dlogits handed back in bf16 where it was formed in f32 adds U (|ref| + bound).
  The model (SwitchHeadAttention): q and k are the bf16 values the stacked projection hands the f32 attention core; v and
  the core's d_o are the references above with their bounds; attention_backward() gives dq, dk with the core's bound,
  rounded to bf16 on the way to the projection (+ U (|ref| + bound)); the projection's weight gradients (q, k, W_s) are
  lib_wgrad() of those and of dlogits; d x = dx of the V experts + lib_gemm of (dq | dk | dlogits) through the stacked
  weight, one f32 addition.

Measured on the MI355X (256 CUs), worst over tests/test_switchhead_bf16_gpu.py -- hard ratio, q / (4 Q_EMU):
    nt64 0.154, 0.121    nn64 0.131, 0.079    dw64 0.984    sums 0.995   (dw64: an expert of one pair with s G next to a
    rounding midpoint attains the U S term; sums: a sum next to a bf16 midpoint attains the U term -- the CPU emulation
    reaches the same 0.987 / 0.995)
    op level, |err| / composed bound, V experts: out 0.004, dx 0.203, dlogits 0.0007 (0.890 handed back in bf16), dw 0.260;
    output experts: out 0.208, da 0.003, dw 0.247;
    in the model, composed through the attention core and the projection's library GEMM: W_s' gradient 0.281, q's 0.040,
    k's 0.036, the input's 0.032.  (The wide entry points on the same inputs, recorded apart: 0.154 / 0.131 / 0.984.)
No fault was found in the kernels: the first run on the GPU passed every kernel-level check.

Input families: moe_ref.make_data rounded to bf16 values; routing families: moe_ref.make_lists, skewed_counts, and the
distinct lists of moe_ref.ref_route_distinct on random ids.
"""
import torch

import moe_bf16_ref as bref
import moe_ref as mref
from moe_bf16_ref import BF16, U, assert_bounded, make_data, ref_nn, ref_nt, ref_wgrad  # noqa: F401
from moe_ref import DATA_FAMILIES, F64, FTZ, TIGHT_FACTOR, U32, gamma, hard_bound, make_lists, skewed_counts  # noqa: F401

# worst q = |err| / (u32 S) of the f32 emulation (tests/test_switchhead_bf16_bounds.py::test_emulation_defines_q)
Q_EMU = {"nt64": 8.0, "nn64": 10.7}

# tile constants of the narrow forms in csrc/moe_bf16.hip
NARROW = 64                                   # widest narrow side
PAIR_TILE, WAVE_PAIRS, K_STEP = 256, 64, 32   # nt64 / nn64: pairs per unit, pairs per wave, contraction step
WG_PAIR_STEP, WG_WIDE_TILE = 32, 128          # wgrad64: pairs per step, tile along the other side
NARROW_WIDTHS = (8, 56, 64)


# ---------------------------------------------------------------------------------------------- expert sums
def ref_expert_sums(A, lda, a_div, ids, scale, G, fan, E, d):
    """amk_moe_expert_sums_bf16 on the values of A (f32 or bf16): {"z" (G, E d), "S_z", "n_z", "bound_z"}."""
    R = mref.ref_expert_sums(A, lda, a_div, ids, scale, G, fan, E, d)
    R["n_z"] = fan
    R["bound_z"] = (gamma(fan) + U) * R["S_z"] + fan * FTZ
    return R


def lib_gemm(z, Bz, w):
    """(ref, bound) of bf16(Z16 @ w) by the library's bf16 GEMM, Z16 within Bz of z (fp64), w (K, N) the bf16 values."""
    w = w.to(F64)
    K = w.shape[0]
    ref = z @ w
    prop = Bz @ w.abs()
    acc = gamma(K + 1) * ((z.abs() + Bz) @ w.abs())
    return ref, prop + acc + U * (ref.abs() + prop + acc) + (K + 1) * FTZ


def lib_wgrad(g, Bg, x16):
    """(ref, bound) of an autocast nn.Linear's weight gradient bf16(G16^T @ x16) by the library's bf16 GEMM: G16 (M, N)
    within Bg of g (fp64), x16 (M, K) the bf16 values; a sum of M terms in any order (n = M + 1), one bf16 rounding."""
    x = x16.to(F64)
    M = x.shape[0]
    ref = g.t() @ x
    prop = Bg.t() @ x.abs()
    acc = gamma(M + 1) * ((g.abs() + Bg).t() @ x.abs())
    return ref, prop + acc + U * (ref.abs() + prop + acc) + (M + 1) * FTZ


def attention_backward(q, k, v, Bv, do, Bdo, scale):
    """fp64 dq, dk of softmax attention o = softmax(scale q k^T) v (no masks) and per-element bounds of the f32 core's
    (csrc/attn_*.hip) results when it reads q, k exactly (B, h, T, D), v within Bv of `v` and d_o within Bdo of `do`.
    First-order chain, every constant generous (the core's errors are u32-sized; what the callers compose on top is
    U-sized), u = u32:
      s = scale q.k, A = scale sum |q||k|:  Es = gamma_{D+4} A  (a chain of D products on the exact-f32 MFMA, the scale
          and log2 e factors; the split-bf16 forward, taken from 128 keys on, is not covered: J < 128 is asserted)
      p = exp(s - m) / l:  relative rho_ij = eta_ij + max_j eta_ij + gamma_{J+8},  eta = Es + max_j Es + 8u (1 + |s| + |m|)
          (the exponent's absolute error, exp2 and the statistics m, log l kept for the backward), taken as expm1(rho)
      o = p v:            Eo = sum_j p (rho + gamma_{J+2}) (|v| + Bv) + sum_j p Bv
      dp = do.v:          Edp = gamma_{D+1} sum (|do| + Bdo)(|v| + Bv) + sum (Bdo |v| + |do| Bv + Bdo Bv)
      delta = do.o (or sum_j p dp: |o| is taken as sum_j p |v|, which covers both):
                          Edl = gamma_{D+J+2} sum (|do| + Bdo)(|o| + Eo) + sum (Bdo |o| + |do| Eo + Bdo Eo)
      ds = p (dp - delta):  Eds = p [rho (|dp| + |delta|) + (1 + rho)(Edp + Edl) + 3u (|dp| + |delta|)]
      dq = scale ds k (a sum over J keys in any order, atomics included):  scale [Eds |k| + gamma_{J+3} (|ds| + Eds) |k|]
      dk = scale ds^T q likewise over the I queries;  plus 1024 2^-126."""
    q, k, v, do, Bv, Bdo = (t.to(F64) for t in (q, k, v, do, Bv, Bdo))
    I, J, D = q.shape[2], k.shape[2], q.shape[3]
    u = U32
    s = scale * (q @ k.transpose(-1, -2))
    A = scale * (q.abs() @ k.abs().transpose(-1, -2))
    assert J < 128, "the split-bf16 forward (ops.ATTENTION_X6_MIN_KEYS) has another score chain"
    Es = gamma(D + 4) * A
    m = s.max(-1, keepdim=True)[0]
    p = torch.softmax(s, -1)
    eta = Es + Es.max(-1, keepdim=True)[0] + 8 * u * (1 + s.abs() + m.abs())
    rho = torch.expm1(eta + eta.max(-1, keepdim=True)[0] + gamma(J + 8))
    va = v.abs() + Bv
    oabs = p @ v.abs()
    Eo = (p * (rho + gamma(J + 2))) @ va + p @ Bv
    doa = do.abs() + Bdo
    dp = do @ v.transpose(-1, -2)
    Edp = gamma(D + 1) * (doa @ va.transpose(-1, -2)) + Bdo @ v.abs().transpose(-1, -2) + do.abs() @ Bv.transpose(-1, -2) \
        + Bdo @ Bv.transpose(-1, -2)
    o = p @ v
    delta = (do * o).sum(-1, keepdim=True)
    Edl = gamma(D + J + 2) * (doa * (oabs + Eo)).sum(-1, keepdim=True) + (Bdo * oabs + do.abs() * Eo + Bdo * Eo).sum(-1, keepdim=True)
    mag = dp.abs() + (do.abs() * oabs).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    Eds = p * (rho * mag + (1 + rho) * (Edp + Edl) + 3 * u * mag)
    dq = scale * (ds @ k)
    Edq = scale * (Eds @ k.abs() + gamma(J + 3) * ((ds.abs() + Eds) @ k.abs())) + 1024 * FTZ
    dk = scale * (ds.transpose(-1, -2) @ q)
    Edk = scale * (Eds.transpose(-1, -2) @ q.abs() + gamma(I + 3) * ((ds.abs() + Eds).transpose(-1, -2) @ q.abs())) + 1024 * FTZ
    return {"dq": dq, "bound_dq": Edq, "dk": dk, "bound_dk": Edk}


def _wgrad_through_z(G_, ldg, g_div, X_, ldx, x_div, Bz_as, off, perm, P, E, N, Kd):
    """dW of wgrad64 without a scale where one operand is the bf16 sums Z16, known as z (fp64) within B_z.  Bz_as: ("G", B)
    or ("X", B), B shaped as that operand."""
    R1 = mref.ref_wgrad(G_, ldg, g_div, X_, ldx, x_div, None, off, perm, P, E, N, Kd)
    which, B = Bz_as
    R2 = (mref.ref_wgrad(B, ldg, g_div, X_, ldx, x_div, None, off, perm, P, E, N, Kd) if which == "G"
          else mref.ref_wgrad(G_, ldg, g_div, B, ldx, x_div, None, off, perm, P, E, N, Kd))
    _, _, cnt = mref.named_pairs(off, perm, E)
    n = (cnt.to(F64) + 2).view(E, 1, 1)
    return R1["dw"], R2["S_dw"] + hard_bound(n, R1["S_dw"] + R2["S_dw"])


def _rows_of(ids, H, E):
    """Row of V / D (G E, .) that pair (u, j) reads: (u // H) E + ids[u, j]."""
    U_, k = ids.shape
    return ((torch.arange(U_, device=ids.device) // H) * E).view(-1, 1) + ids


def ref_shared_row(x, logits, W16, d_out, ids, gate, k, H):
    """ops.shared_row_experts under bf16 autocast and its backward on d_out (U, d): out, dx, dlogits, dw."""
    U_, E = logits.shape
    G = U_ // H
    fan = H * k
    N, Kd = W16.shape[1], W16.shape[2]
    x16, w16 = x.to(BF16).contiguous(), W16.to(BF16).contiguous()
    off, perm = mref.ref_route_distinct(ids, G, fan, E)
    Rv = ref_nt(x16, Kd, E, w16, None, off, perm, G * E, E, N, Kd)
    rows = _rows_of(ids, H, E)                                     # (U, k)
    V, Bv = Rv["y"][rows], Rv["bound_y"][rows]                     # (U, k, N); every row read is a named one
    g = gate.to(F64).view(U_, k, 1)
    Va = V.abs() + Bv
    out = (g * V).sum(1)
    b_out = (g * Bv).sum(1) + gamma(2 * k) * (g * Va).sum(1) + 2 * k * FTZ
    d64 = d_out.to(F64).reshape(U_, 1, N)
    f = (g * (1 - g)).view(U_, k)
    dl = torch.zeros(U_, E, dtype=F64, device=x.device)
    b_dl = torch.zeros_like(dl)
    ur = torch.arange(U_, device=x.device).view(-1, 1).expand(U_, k)
    dl[ur, ids] = f * (d64 * V).sum(2)
    b_dl[ur, ids] = hard_bound(N + 7, f * (d64.abs() * Va).sum(2)) + f * (d64.abs() * Bv).sum(2)
    d_in = d_out if d_out.dtype == BF16 else d_out.float()
    Rz = ref_expert_sums(d_in.reshape(U_, N), N, k, ids, gate.reshape(-1), G, fan, E, N)
    z, Bz = Rz["z"], Rz["bound_z"]
    dx, b_dx = lib_gemm(z, Bz, w16.reshape(E * N, Kd))
    dw, b_dw = _wgrad_through_z(z.reshape(G * E, N), N, 1, x16, Kd, E, ("G", Bz.reshape(G * E, N)), off, perm, G * E, E, N, Kd)
    R = {"out": out, "bound_out": b_out, "dx": dx, "bound_dx": b_dx, "dlogits": dl, "bound_dlogits": b_dl, "dw": dw, "bound_dw": b_dw}
    if logits.dtype == BF16:
        R["bound_dlogits"] = b_dl + U * (dl.abs() + b_dl)
    return R


def ref_summed(a, logits, W16, d_out, ids, k, H):
    """ops.summed_experts under bf16 autocast and its backward on d_out (G, dim): out, da, dw."""
    U_, E = logits.shape
    G = U_ // H
    fan = H * k
    N, Kd = W16.shape[1], W16.shape[2]
    w16 = W16.to(BF16).contiguous()
    Rz = ref_expert_sums(a, Kd, k, ids, None, G, fan, E, Kd)
    z, Bz = Rz["z"], Rz["bound_z"]
    out, b_out = lib_gemm(z, Bz, w16.permute(0, 2, 1).reshape(E * Kd, N))
    d16 = d_out.to(BF16).contiguous()
    off, perm = mref.ref_route_distinct(ids, G, fan, E)
    Rd = ref_nn(d16, N, E, w16, None, off, perm, G * E, E, N, Kd)
    rows = _rows_of(ids, H, E)
    D, Bd = Rd["y"][rows], Rd["bound_y"][rows]
    da = D.sum(1)
    b_da = Bd.sum(1) + gamma(k) * (D.abs() + Bd).sum(1) + k * FTZ
    dw, b_dw = _wgrad_through_z(d16, N, E, z.reshape(G * E, Kd), Kd, 1, ("X", Bz.reshape(G * E, Kd)), off, perm, G * E, E, N, Kd)
    return {"out": out, "bound_out": b_out, "da": da, "bound_da": b_da, "dw": dw, "bound_dw": b_dw}


# ---------------------------------------------------------------------------------------------- checking
WORST = bref.WORST   # kernel -> [worst hard ratio, worst q / (TIGHT_FACTOR Q_EMU) or None]; op level under 'op_' + name


def measures(got, R, name):
    return mref.measures(got, R, name)


def violations(got, R, name, kernel=None):
    nbad, _, q = measures(got, R, name)
    return nbad + (1 if kernel in Q_EMU and q > TIGHT_FACTOR * Q_EMU[kernel] else 0)


def assert_within(got, R, name, kernel, what="", key=None):
    """The hard tier on every element, the tight tier where the kernel has one; records the worst figures under `key`
    (default: the kernel's name)."""
    nbad, ratio, q = measures(got, R, name)
    w = WORST.setdefault(key or kernel, [0.0, None])
    w[0] = max(w[0], ratio)
    msg = f"{what} {name}: hard ratio {ratio:.4g}"
    if kernel in Q_EMU:
        lim = TIGHT_FACTOR * Q_EMU[kernel]
        w[1] = max(w[1] or 0.0, q / lim)
        msg += f", q {q:.4g} (limit {lim:.4g})"
    print(msg)
    assert nbad == 0, f"{what} {name}: {nbad} elements outside the hard bound (worst {ratio:.3g}x)"
    if kernel in Q_EMU:
        assert q <= lim, f"{what} {name}: q = |err| / (u32 S) reaches {q:.3g}, limit {lim:.3g} ({TIGHT_FACTOR} x the emulation)"


# ---------------------------------------------------------------------------------------------- the GPU case list
EDGE = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 0]          # per-expert counts at the tile edges, empty first and last
HOLES = [0, 1, 31, 0, 33, 65, 0, 0, 257, 129, 0]


def C(id, family, route, d, w, a_div=1, x_div=1, pad=False, nulls=False):
    """d: the narrow side (nt64: N, nn64: Kd, wgrad64: either), w: the other side.  route: ("counts", counts) |
    ("sparse", counts, P) | ("distinct", G, fan, E): amk_moe_route_distinct's virtual pairs (P = G E)."""
    E = route[3] if route[0] == "distinct" else len(route[1])
    return dict(id=id, family=family, route=route, E=E, d=d, w=w, a_div=a_div, x_div=x_div, pad=pad, nulls=nulls)


CASES = [
    C("edge_d64_w128", "unit", ("counts", EDGE), 64, 128, 2, 2),
    C("holes_d8_w136", "expert_scale", ("counts", HOLES), 8, 136, 16, 2),
    C("skew_d56_w264", "cancel", ("counts", skewed_counts(900, 6)), 56, 264, 1, 1),
    C("distinct_d64_w256", "binade", ("distinct", 70, 8, 8), 64, 256, 8, 1),
    C("sparse_d64_w120", "gate_tiny", ("sparse", [40, 0, 256, 33, 127], 700), 64, 120, 3, 3, pad=True),
    C("one_takes_all_d56_w32", "outlier_rows", ("counts", [0, 0, 600, 0]), 56, 32, 2, 16, nulls=True),
    C("holes_d8_w8", "unit", ("counts", HOLES), 8, 8, 1, 1, nulls=True),
    C("edge_d64_w24", "binade", ("counts", EDGE), 64, 24, 2, 2, pad=True),
    C("holes_d56_w40", "cancel", ("counts", HOLES), 56, 40, 3, 1, pad=True),
    C("e70_d64_w72", "expert_scale", ("counts", bref._rand_counts(194, 70, 2)), 64, 72, 2, 2),
]

# expert sums: (id, G, fan, E, d, a_div, scaled, A in bf16, padded row stride)
SUM_CASES = [
    dict(id="switchhead_32", G=37, fan=16, E=32, d=64, a_div=2, scaled=False, a16=False, pad=False),
    dict(id="gated_bf16_rows", G=37, fan=16, E=32, d=64, a_div=2, scaled=True, a16=True, pad=True),
    dict(id="gated_f32_rows", G=65, fan=6, E=5, d=8, a_div=3, scaled=True, a16=False, pad=True),
    dict(id="one_expert", G=9, fan=12, E=1, d=56, a_div=1, scaled=False, a16=True, pad=False),
    dict(id="many_experts", G=5, fan=300, E=270, d=32, a_div=4, scaled=True, a16=False, pad=False),
]


# op level: (G tokens, H heads, k, E, dim, d); each passes ops.distinct_experts_ok (asserted on the CPU)
OP_SHAPES = [(130, 4, 2, 4, 256, 64), (97, 8, 2, 8, 256, 32), (65, 4, 3, 5, 264, 64)]


def case_lists(c, seed=7):
    """(ids (P) with -1 for a pair no list names, offsets, perm, P) of a case."""
    r = c["route"]
    if r[0] == "distinct":
        _, G, fan, E = r
        g = torch.Generator().manual_seed(seed)
        sel = torch.stack([torch.randperm(E, generator=g)[:2] for _ in range(G * fan // 2)]).reshape(G * fan // 2 * 2)
        off, perm = mref.ref_route_distinct(sel.view(-1, 2), G, fan, E)
        ids = torch.full((G * E,), -1, dtype=torch.int64)
        ids[perm.long()] = perm.long() % E
        return ids, off, perm, G * E
    counts = r[1]
    P = r[2] if r[0] == "sparse" else sum(counts)
    ids, off, perm = make_lists(counts, P=P, seed=seed)
    return ids, off, perm, P


def case_counts(c):
    _, off, _, P = case_lists(c)
    return (off[1:] - off[:-1]).tolist(), P


def sum_inputs(c, seed=11):
    """(A (rows, lda) f32 or bf16 with NaN padding, ids (G fan), scale or None) of an expert-sums case."""
    g = torch.Generator().manual_seed(seed)
    G, fan, E, d, a_div = c["G"], c["fan"], c["E"], c["d"], c["a_div"]
    rows = (G * fan - 1) // a_div + 1
    lda = d + 8 if c["pad"] else d
    A = torch.full((rows, lda), float("nan"))
    A[:, :d] = torch.randn(rows, d, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, 1), generator=g).float())
    ids = torch.randint(0, E, (G * fan,), generator=g)
    ids[:fan] = 0                                   # a row whose pairs all chose one expert: the full sum of fan terms
    scale = torch.sigmoid(torch.randn(G * fan, generator=g)) if c["scaled"] else None
    return (A.to(BF16) if c["a16"] else A), ids, scale


def _edge(v, t, step=1):
    return {"-": v == t - step, "0": v == t, "+": v == t + step}


def case_features(c):
    counts, P = case_counts(c)
    d, w, out = c["d"], c["w"], set()
    out.add(f"narrow {d}")
    for s, hit in _edge(w, WG_WIDE_TILE, 8).items():
        if hit:
            out.add(f"wgrad wide tile {s}")
    for s, hit in _edge(w, K_STEP, 8).items():
        if hit:
            out.add(f"k step {s}")
    if w > WG_WIDE_TILE:
        out.add("wgrad wide tiles > 1")
    if w % K_STEP:
        out.add("k tail")
    for t, name in ((PAIR_TILE, "pair tile"), (WAVE_PAIRS, "wave pairs"), (WG_PAIR_STEP, "wgrad step")):
        for s in "-0+":
            if t + "-0+".index(s) - 1 in counts:
                out.add(f"{name} {s}")
    if max(counts) > 2 * PAIR_TILE:
        out.add("pair tiles > 2")
    out |= {f"count {n}" for n in (0, 1) if n in counts}
    out.add("nulls" if c["nulls"] else "bias and scale")
    if c["E"] > 64:
        out.add("E > 64")
    if c["route"][0] != "counts":
        out.add(c["route"][0])
    if c["pad"]:
        out.add("pad")
    out |= {f"a_div {c['a_div']}", f"x_div {c['x_div']}", f"family {c['family']}"}
    return out


def required_features():
    req = {f"narrow {d}" for d in NARROW_WIDTHS}
    req |= {f"{name} {s}" for name in ("wgrad wide tile", "k step", "pair tile", "wave pairs", "wgrad step") for s in "-0+"}
    req |= {"wgrad wide tiles > 1", "k tail", "pair tiles > 2", "count 0", "count 1", "nulls", "bias and scale", "E > 64",
            "sparse", "distinct", "pad"}
    req |= {f"a_div {d}" for d in (1, 2, 3, 16)} | {f"x_div {d}" for d in (1, 2, 3, 16)} | {f"family {f}" for f in DATA_FAMILIES}
    return req


def missing_coverage():
    seen = set()
    for c in CASES:
        seen |= case_features(c)
    missing = required_features() - seen
    sums = {(c["scaled"], c["a16"]) for c in SUM_CASES}
    missing |= {f"expert sums scaled={s} bf16={b}" for s in (False, True) for b in (False, True) if (s, b) not in sums}
    if not any(c["pad"] for c in SUM_CASES):
        missing.add("expert sums pad")
    return missing
