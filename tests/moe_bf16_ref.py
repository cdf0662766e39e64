"""fp64 references, per-element error bounds and input families for the bf16 grouped expert GEMMs (csrc/moe_bf16.hip)
and for ops._RoutedLinearBF16 built on them.

House rules of tests/moe_ref.py and tests/bf16_dense_ref.py: every reference is computed in fp64 ON THE VALUES THE
KERNEL READS -- the bf16 operands as bf16 values, the f32 bias and scale as given -- with the addressing arguments of
the C ABI; bounds are per element, derived from the kernel's own operation chain; no term is relative to a tensor's
maximum; no element is left out.  u32 = 2^-24, U = 2^-8 (one bf16 rounding: bf16 keeps 8 significant bits, so
round-to-nearest is off by at most U / (1 + U) of the value -- U itself is the margin), gamma_n = n u32 / (1 - n u32),
flush term n 2^-126.

* nt (grouped_bf16_kernel<false>; Y = A W_e^T + b_e): bf16 x bf16 products are exact in f32; v_mfma_f32_32x32x16_bf16
  sums them into ONE f32 accumulator per element over ceil(Kd / 32) steps of 32 (the tail of the contraction, absent
  pairs and rows past N are staged as exact zeros: they add nothing), no fold, then the f32 bias is added:
      n = Kd + 1,   |got - ref| <= gamma_n S + n 2^-126,   S = |A| |W_e|^T + |b_e|.
* nn (grouped_bf16_kernel<true>; Y = s (G W_e)): the same chain over N, then one f32 product with the scale:
      n = N + 1,    S = |s| |G| |W_e|.
* wgrad (grouped_wgrad_bf16_kernel; dW_e = sum_p s G^T (x) X): s G is formed in f32 and ROUNDED ONCE TO BF16 where it is
  staged (together within U of the term: U / (1 + U) for the rounding, and the U^2 left over covers the u32 of the f32
  product -- an expert of one pair with s G near a rounding midpoint comes close to it), then one exact product and one add per pair
  of the expert (steps of 32 pairs, absent pairs zeros), one workgroup per output tile -- no split, no partial sums:
      n = cnt_e + 2,   |got - ref| <= U S + gamma_n S + n 2^-126,   S = sum_p |s| |G|^T |X|   (no U term without a scale).
  dbias: the staged (rounded) values summed in f32 per thread over its two rows of every step, then the 16 row groups
  in order -- cnt_e - 1 additions of non-zero terms in a fixed tree:  the same form with S = sum_p |s| |G|.
  An expert without pairs has S = 0: exactly zero.  (The data families keep s G far above the subnormals -- the
  smallest is 2^-20 x 2^-12 x the unit scale -- so the rounding of s G is relative throughout.)

Tight tier (nt, nn), as moe_ref.py has it: q = (|err| - n 2^-126) / (u32 S) is held to TIGHT_FACTOR (4, of moe_ref.py) x
the worst q that the f32 CPU emulation of tests/test_moe_bf16_bounds.py (one product and one add per contraction
step on the bf16-valued inputs, bias / scale after the chain) reaches over every family and every shape of the GPU case
list: the constants Q_EMU below, asserted there.  A Y rounded to bf16 somewhere has q near 2^15 and misses it.

Op level (ops._RoutedLinearBF16 as MoELayer calls it; x16 = bf16(x), W16 = bf16(W), d16 = bf16(d_out), the f32 gate g as
amk_moe_route returns it -- the values the kernels read).  The rules of moe_ref.py for the two f32 kernels it goes
through: combine_kernel rounds w y and every sum separately (2 operations per slot, 1 when un-weighted), gate_grad has
n = N + 7 on S = g (1 - g) sum |dOut| |Y|.  With B_y the nt bound of a pair's row and Ya = |Y_ref| + B_y:
      out     = sum_j g_j Y_j:        sum_j g_j B_y_j + gamma_2k sum_j g_j Ya_j + 2k 2^-126
      dxp     = nn on d16 with s = g:  B_nn;   dx = sum over the k pairs of the row (un-weighted combine):
                                       sum_j B_nn_j + gamma_k sum_j (|dxp_ref_j| + B_nn_j) + k 2^-126
      dlogits = g (1 - g) <dOut, Y>:   hard_bound(N + 7, g (1 - g) sum |dOut| Ya) + g (1 - g) sum |dOut| B_y
      dW, db  = wgrad on (d16, x16, g): the kernel bound.
A dx or dlogits handed back in bf16 (the caller passed bf16) adds U (|ref| + bound).

Measured on the MI355X (256 CUs), worst over tests/test_moe_bf16_gpu.py -- hard ratio, q / (4 Q_EMU):
    nt 0.128, 0.074    nn 0.169, 0.092    dw 0.971    db 0.970   (an expert of one pair with s G next to a rounding
    midpoint attains the U S term: 0.97 is the bound being exact, not the kernel being close to wrong)
    op level, |err| / composed bound: out 0.016, dx 0.005 (0.971 handed back in bf16), dlogits 0.001 (0.904 in bf16),
    dw 0.547, db 0.371.
No fault was found in the kernels: the first run on the GPU passed every check.

Input families: moe_ref.make_data rounded to bf16 values (A, W, Gm, X; bias and scale stay f32); routing families:
moe_ref.make_lists, skewed_counts.
"""
import torch

import moe_ref as mref
from moe_ref import (DATA_FAMILIES, F64, FTZ, TIGHT_FACTOR, U32, hard_bound, make_lists, named_pairs,  # noqa: F401
                     skewed_counts, take_rows)

U = 2.0 ** -8
BF16 = torch.bfloat16

# worst q = |err| / (u32 S) of the f32 emulation (tests/test_moe_bf16_bounds.py::test_emulation_defines_q)
Q_EMU = {"nt": 9.0, "nn": 13.5}

# tile constants of csrc/moe_bf16.hip (the case lists put counts and widths one below, at and one above each)
PAIR_TILE, COL_TILE, K_STEP = 64, 256, 32          # nt / nn
WG_PAIR_STEP, WG_TILE = 32, 128                    # wgrad


def make_data(family, P, E, N, Kd, a_div, x_div, seed, lda=None, ldn=None, ldx=None):
    """moe_ref.make_data with A, W, Gm, X as bf16 tensors (padding columns NaN), bias and scale f32."""
    D = mref.make_data(family, P, E, N, Kd, a_div, x_div, seed, lda, ldn, ldx)
    for key in ("A", "W", "Gm", "X"):
        D[key] = D[key].to(BF16)
    return D


def ref_nt(A, lda, a_div, W, bias, offsets, perm, P, E, N, Kd):
    R = mref.ref_nt(A, lda, a_div, W, bias, offsets, perm, P, E, N, Kd)
    R["n_y"] = Kd + 1
    R["bound_y"] = hard_bound(Kd + 1, R["S_y"])
    return R


def ref_nn(G, ldg, a_div, W, scale, offsets, perm, P, E, N, Kd):
    R = mref.ref_nn(G, ldg, a_div, W, scale, offsets, perm, P, E, N, Kd)
    R["n_y"] = N + 1
    R["bound_y"] = hard_bound(N + 1, R["S_y"])
    return R


def ref_wgrad(G, ldg, g_div, X, ldx, x_div, scale, offsets, perm, P, E, N, Kd):
    R = mref.ref_wgrad(G, ldg, g_div, X, ldx, x_div, scale, offsets, perm, P, E, N, Kd)
    _, _, cnt = named_pairs(offsets, perm, E)
    n = cnt.to(F64) + 2
    u = U if scale is not None else 0.0
    for name, shape in (("dw", (E, 1, 1)), ("db", (E, 1))):
        R["n_" + name] = n.view(shape)
        R["bound_" + name] = u * R["S_" + name] + hard_bound(n.view(shape), R["S_" + name])
    return R


# ---------------------------------------------------------------------------------------------- op level
def ref_op(x, logits, W, bias, d_out, route, k):
    """ops.routed_linear(x, logits, W, bias, k, x_div=k) under bf16 autocast and its backward on d_out: references and
    bounds of out, dx, dlogits, dw, db.  route: ops.moe_route(logits.float(), k) (ids, gate, offsets, perm)."""
    dev = x.device
    U_, E = logits.shape
    N, Kd = W.shape[1], W.shape[2]
    P = U_ * k
    x16, w16, d16 = x.to(BF16).contiguous(), W.to(BF16).contiguous(), d_out.float().to(BF16).contiguous()
    ids, gate, off, perm = route["ids"], route["gate"], route["offsets"], route["perm"]
    g = gate.reshape(-1).to(F64)
    Ry = ref_nt(x16, Kd, k, w16, bias, off, perm, P, E, N, Kd)
    Y, By = Ry["y"], Ry["bound_y"]
    Ya = Y.abs() + By
    out = (g.view(-1, 1) * Y).view(U_, k, N).sum(1)
    b_out = (g.view(-1, 1) * By).view(U_, k, N).sum(1) + mref.gamma(2 * k) * (g.view(-1, 1) * Ya).view(U_, k, N).sum(1) + 2 * k * FTZ
    Rn = ref_nn(d16, N, k, w16, gate.reshape(-1), off, perm, P, E, N, Kd)
    dxp, Bn = Rn["y"], Rn["bound_y"]
    dx = dxp.view(U_, k, Kd).sum(1)
    b_dx = Bn.view(U_, k, Kd).sum(1) + mref.gamma(k) * (dxp.abs() + Bn).view(U_, k, Kd).sum(1) + k * FTZ
    d64 = d_out.to(F64).reshape(U_, N)
    f = (g * (1 - g))
    pr = torch.arange(P, device=dev) // k
    dl = torch.zeros(U_, E, dtype=F64, device=dev)
    S_dl, extra = torch.zeros_like(dl), torch.zeros_like(dl)
    idx = (pr, ids.reshape(-1))
    dl[idx] = f * (d64[pr] * Y).sum(1)
    S_dl[idx] = f * (d64[pr].abs() * Ya).sum(1)
    extra[idx] = f * (d64[pr].abs() * By).sum(1)
    b_dl = hard_bound(N + 7, S_dl) + extra
    Rw = ref_wgrad(d16, N, k, x16, Kd, k, gate.reshape(-1), off, perm, P, E, N, Kd)
    R = {"out": out, "bound_out": b_out, "dx": dx, "bound_dx": b_dx, "dlogits": dl, "bound_dlogits": b_dl,
         "dw": Rw["dw"], "bound_dw": Rw["bound_dw"], "db": Rw["db"], "bound_db": Rw["bound_db"]}
    if x.dtype == BF16:
        R["bound_dx"] = R["bound_dx"] + U * (dx.abs() + R["bound_dx"])
    if logits.dtype == BF16:
        R["bound_dlogits"] = R["bound_dlogits"] + U * (dl.abs() + R["bound_dlogits"])
    return R


# ---------------------------------------------------------------------------------------------- checking
WORST = {}   # kernel -> [worst hard ratio, worst q / (TIGHT_FACTOR Q_EMU) or None]


def measures(got, R, name):
    """moe_ref.measures: (elements outside the hard bound, worst |err| / bound, worst q)."""
    return mref.measures(got, R, name)


def violations(got, R, name, kernel=None):
    nbad, _, q = measures(got, R, name)
    return nbad + (1 if kernel in Q_EMU and q > TIGHT_FACTOR * Q_EMU[kernel] else 0)


def assert_within(got, R, name, kernel, what=""):
    """The hard tier on every element, the tight tier where the kernel has one; records the worst figures."""
    nbad, ratio, q = measures(got, R, name)
    w = WORST.setdefault(kernel, [0.0, None])
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


def assert_bounded(got, R, name, what=""):
    """Op level: |got - ref| <= bound on every element (a NaN is outside); records the worst ratio under 'op_' + name."""
    ref, b = R[name], R["bound_" + name]
    a = got.detach().to(ref.device, F64).reshape(ref.shape)
    err = (a - ref).abs()
    bad = ~(err <= b)
    ratio = torch.where(err > 0, err / b, torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    r = float(ratio.max()) if a.numel() else 0.0
    w = WORST.setdefault("op_" + name, [0.0, None])
    w[0] = max(w[0], r)
    print(f"{what} {name}: worst |err| / bound {r:.4g}")
    assert int(bad.sum()) == 0, f"{what} {name}: {int(bad.sum())} elements outside the composed bound (worst {r:.3g}x)"


# ---------------------------------------------------------------------------------------------- the GPU case list
EDGE = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 257]          # per-expert counts at the tile edges
HOLES = [0, 1, 31, 0, 33, 65, 0, 0, 97, 129, 164, 0]                         # empty experts first, in the middle, last


def _rand_counts(P, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.bincount(torch.randint(0, E, (P,), generator=g), minlength=E).tolist()


def C(id, family, route, N, Kd, a_div=1, x_div=1, pad=False, nulls=False):
    counts = route[1]
    return dict(id=id, family=family, route=route, E=len(counts), N=N, Kd=Kd, a_div=a_div, x_div=x_div, pad=pad, nulls=nulls)


# route: ("counts", counts) | ("sparse", counts, P)
CASES = [
    C("edge_136x128", "unit", ("counts", EDGE), 136, 128, 2, 2),
    C("holes_64x72", "expert_scale", ("counts", HOLES), 64, 72, 16, 2),
    C("skew_128x264", "cancel", ("counts", skewed_counts(1500, 8)), 128, 264, 1, 1),
    C("sparse_256x64", "binade", ("sparse", [40, 0, 100, 33, 127], 520), 256, 64, 2, 2),
    C("one_takes_all_264x136", "gate_tiny", ("counts", [0, 0, 777, 0]), 264, 136, 3, 3),
    C("holes_8x8", "unit", ("counts", HOLES), 8, 8, 1, 1),
    C("strides_1024", "outlier_rows", ("counts", _rand_counts(300, 6, 4)), 1024, 1024, 16, 2, pad=True),
    C("edge_248x256", "expert_scale", ("counts", EDGE), 248, 256, 2, 2, pad=True, nulls=True),
    C("holes_120x248", "binade", ("counts", HOLES), 120, 248, 3, 1, pad=True),
    C("edge_24x40", "cancel", ("counts", EDGE), 24, 40, 2, 16),
    C("holes_32x32", "gate_tiny", ("counts", HOLES), 32, 32, 1, 1, nulls=True),
    C("holes_40x24", "outlier_rows", ("counts", HOLES), 40, 24, 2, 2),
    C("e70_128x120", "expert_scale", ("counts", _rand_counts(194, 70, 2)), 128, 120, 2, 2),
]


def case_counts(c):
    r = c["route"]
    return r[1], (r[2] if r[0] == "sparse" else sum(r[1]))


def case_features(c):
    """What of the kernels' control flow a case reaches (csrc/moe_bf16.hip has one kernel per entry point and no
    dispatch on the device's size; these are the branches and edges inside them)."""
    counts, P = case_counts(c)
    N, Kd, out = c["N"], c["Kd"], set()
    for kind, wout, win in (("nt", N, Kd), ("nn", Kd, N)):
        for name, v, t in (("out", wout, COL_TILE), ("k", win, K_STEP)):
            for d in (-8, 0, 8):
                if v == t + d:
                    out.add(f"{kind} {name} tile {'-0+'[d // 8 + 1]}")
        if wout > COL_TILE:
            out.add(f"{kind} column tiles > 1")
        if win % K_STEP:
            out.add(f"{kind} k tail")
    for name, v in (("n", N), ("k", Kd)):
        for d in (-8, 0, 8):
            if v == WG_TILE + d:
                out.add(f"wgrad {name} tile {'-0+'[d // 8 + 1]}")
    for t, name in ((PAIR_TILE, "pair tile"), (WG_PAIR_STEP, "wgrad step")):
        for d in (-1, 0, 1):
            if t + d in counts:
                out.add(f"{name} {'-0+'[d + 1]}")
    out.add("wgrad scale" if not c["nulls"] else "nulls")
    out.add("wgrad noscale")
    if 0 in counts:
        out.add("empty expert")
    if c["E"] > 64:
        out.add("E > 64")
    if c["route"][0] == "sparse":
        out.add("sparse")
    if c["pad"]:
        out.add("pad")
    out |= {f"a_div {c['a_div']}", f"x_div {c['x_div']}", f"family {c['family']}"}
    return out


def required_features():
    req = {f"{kind} {name} tile {s}" for kind in ("nt", "nn") for name in ("out", "k") for s in "-0+"}
    req |= {f"wgrad {name} tile {s}" for name in ("n", "k") for s in "-0+"}
    req |= {f"{name} {s}" for name in ("pair tile", "wgrad step") for s in "-0+"}
    req |= {"nt column tiles > 1", "nn column tiles > 1", "nt k tail", "nn k tail", "wgrad scale", "wgrad noscale", "nulls",
            "empty expert", "E > 64", "sparse", "pad"}
    req |= {f"a_div {d}" for d in (1, 2, 3, 16)} | {f"x_div {d}" for d in (1, 2, 3, 16)} | {f"family {f}" for f in DATA_FAMILIES}
    return req


def missing_coverage():
    seen = set()
    for c in CASES:
        seen |= case_features(c)
    return required_features() - seen
