"""CPU checks of the bf16 GEMM / mixed-precision checker (tests/bf16_dense_ref.py), no GPU needed.

Not too tight: an f32 emulation of the rounding points of each kernel (csrc/gemm_bf16.hip, csrc/mixed_bf16.hip: exact
bf16 products summed in f32 per 32-deep step, the f32 bias, the f32 SwiGLU epilogues with dG rounded to bf16 in
between, the TN chunks summed in order, the two-pass LayerNorm statistics, every bf16 output rounded once) stays within
half of every element's bound on every input family.
Sensitive enough: results that are wrong the way these kernels go wrong -- a row of a partial tile unwritten, the K
tail dropped, a bias group missing, the padding step not zero, gate / value columns mispaired, silu or silu' cut off,
exp2 without log2e, da / db swapped, a 64-row step or the db tile rule wrong, rstd of the neighbouring row, the
one-pass variance, dh16 rounded too early, a bf16 sigmoid -- are flagged on at least the listed families.
test_old_criteria_report prints which of these the suite's older global criteria (max |got - ref| / max |ref|) pass
(AMK_BF16_DENSE_OLD_REPORT=<file>: also as JSON)."""
import json
import math
import os

import pytest
import torch

import bf16_dense_ref as ref

F32 = torch.float32
bf = ref.bf16_round
LOG2E32 = torch.tensor(math.log2(math.e), dtype=F32)


# ---------------------------------------------------------------------------------------------- emulations
def _acc(a, W, mutation=None):
    """f32 accumulators of a (M, K) @ W (K, N) step by step over 32-deep K steps, as gemm_bf16_kernel forms them."""
    M, K = a.shape
    steps = (K + 31) // 32
    acc = torch.zeros(M, W.shape[1], dtype=F32)
    last_tile = 128 * ((M - 1) // 128)
    for t in range(steps):
        part = a[:, 32 * t:32 * t + 32] @ W[32 * t:32 * t + 32]
        if mutation == "k_tail_dropped" and t == steps - 1:
            part[last_tile:] = 0.0
        acc = acc + part
    if mutation == "pad_step_repeats" and steps % 2:   # the zero step of an odd step count reads the last real step again
        acc = acc + a[:, 32 * (steps - 1):] @ W[32 * (steps - 1):]
    return acc


def emu_gemm(a, w, bias=None, nn=False, mutation=None):
    a, W = a.to(F32), (w if nn else w.t()).to(F32)
    acc = _acc(a, W, mutation)
    if bias is not None:
        b = bias.to(F32).clone()
        if mutation == "bias_missing_last_group":
            b[-8:] = 0.0
        acc = acc + b
    c = bf(acc)
    if mutation == "last_row_unwritten":
        c[-1] = 0.0
    return {"c": c}


def _sigmoid_hw(x, mutation=None):
    t = -x if mutation == "exp2_no_log2e" else -x * LOG2E32
    return torch.reciprocal(1.0 + torch.exp2(t))


def emu_swiglu_fwd(a, w12, b12, mutation=None):
    acc = _acc(a.to(F32), w12.t().to(F32)) + b12.to(F32)
    H = acc.shape[1] // 2
    x, y = acc[:, :H], acc[:, H:].clone()
    if mutation == "pair_off_by_32":               # the last (partial) 64-column gate tile pairs j with value j +- 32
        j0 = 64 * ((H - 1) // 64)
        lo, hi = torch.arange(j0, min(j0 + 32, H - 32)), torch.arange(j0, min(j0 + 32, H - 32)) + 32
        y[:, lo], y[:, hi] = acc[:, H + hi], acc[:, H + lo]
    s = _sigmoid_hw(x, mutation)
    if mutation == "silu_zero_below_-3":
        s = torch.where(x < -3, torch.zeros_like(s), s)
    return {"g": bf(x * s * y), "ab": bf(acc)}


def emu_swiglu_bwd(dy, w3, ab, mutation=None):
    G = bf(_acc(dy.to(F32), w3.to(F32)))
    H = G.shape[1]
    A, B = ab[:, :H].to(F32), ab[:, H:].to(F32)
    s = _sigmoid_hw(A)
    inner = 1.0 + A * (1.0 - s)
    if mutation == "silu_prime_no_a_term":
        inner = torch.where(A < -1, torch.ones_like(inner), inner)
    da, db = bf(G * B * (s * inner)), bf(G * (A * s))
    if mutation == "swap_last8":
        da[:, -8:], db[:, -8:] = db[:, -8:].clone(), da[:, -8:].clone()
    return {"dab": torch.cat([da, db], 1)}


def emu_tn(y, x, mutation=None, cus=256):
    y, x = y.to(F32), x.to(F32)
    M, N = y.shape
    K = x.shape[1]
    spc, nch = ref.tn_chunks(M, N, K, cus)
    dw, db = torch.zeros(N, K, dtype=F32), torch.zeros(N, dtype=F32)
    for c in range(nch):
        acc, bs = torch.zeros(N, K, dtype=F32), torch.zeros(N, dtype=F32)
        for s in range(spc):
            r0 = 64 * (c * spc + s)
            if r0 >= M or (mutation == "drop_step" and c == nch - 1 and s == 1):
                continue
            acc = acc + y[r0:r0 + 64].t() @ x[r0:r0 + 64]
            bs = bs + y[r0:r0 + 64].sum(0)
        dw, db = dw + acc, db + bs
    if mutation == "db_every_k_tile":
        db = db * ((K + ref.tn_tile_k(N, K) - 1) // ref.tn_tile_k(N, K))
    return {"dw": dw, "db": db}


def emu_ln(x, res, gamma, beta, dy, dh_in, mutation=None):
    x = x.to(F32)
    h = x + res.to(F32) if res is not None else x
    D = h.shape[1]
    inv_d = torch.tensor(1.0 / D, dtype=F32)
    mean = h.sum(-1, keepdim=True) * inv_d
    v = h - mean
    if mutation == "one_pass_var":
        var = (h * h).sum(-1, keepdim=True) * inv_d - mean * mean
    else:
        var = (v * v).sum(-1, keepdim=True) * inv_d
    rstd = torch.rsqrt(var + ref.LN_EPS)
    if mutation == "rstd_neighbour_row":
        rstd = torch.roll(rstd, 1, 0)
    y = bf(v * rstd * gamma + beta)
    out = {"h": h, "y": y, "mean": mean[:, 0], "rstd": rstd[:, 0]}
    if dy is None:
        return out
    dy = dy.to(F32)
    xh = v * rstd
    gy = dy * gamma
    c1 = gy.sum(-1, keepdim=True) * inv_d
    c2 = (gy * xh).sum(-1, keepdim=True) * inv_d
    dh0 = rstd * (gy - c1 - xh * c2)
    dh = dh0 + dh_in if dh_in is not None else dh0
    dh16 = bf(bf(dh0) + dh_in) if mutation == "dh16_before_dh_in" and dh_in is not None else bf(dh)
    out.update({"dh": dh, "dh16": dh16, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0)})
    return out


def emu_swiglu_mixed(ab, cot, mutation=None):
    H = cot.shape[1]
    A, B, G = ab[:, :H].to(F32), ab[:, H:].to(F32), cot.to(F32)
    if mutation == "sigmoid_bf16":
        s = bf(1.0 / bf(1.0 + bf(torch.exp(-A))))
    else:
        s = 1.0 / (1.0 + torch.exp(-A))
    g = bf(A * s * B)
    da, db = bf(G * B * (s * (1.0 + A * (1.0 - s)))), bf(G * (A * s))
    return {"g": g, "dab": torch.cat([da, db], 1)}


# ---------------------------------------------------------------------------------------------- cases
NT_SHAPE, SW_SHAPE, TN_SHAPE, LN_SHAPE, MX_SHAPE = (300, 136, 72), (300, 104, 40), (1000, 136, 264), (64, 260), (64, 104)
LN_OUT = ("h", "y", "mean", "rstd", "dh", "dh16", "dgamma", "dbeta")


def case(kernel, family, mutation=None, seed=11, variant=(True, True)):
    """(emulated outputs, reference dict, names of the outputs) of one kernel on one input family."""
    if kernel in ("nt", "nn"):
        nn = kernel == "nn"
        M, N, K = NT_SHAPE
        a, w, b = ref.make_gemm(family, M, N, K, seed, nn=nn)
        b = None if nn else b
        return emu_gemm(a, w, b, nn, mutation), ref.ref_gemm(a, w, b, nn), ("c",)
    if kernel == "swiglu_fwd":
        a, w12, b12 = ref.make_swiglu(family, *SW_SHAPE, seed)
        return emu_swiglu_fwd(a, w12, b12, mutation), ref.ref_swiglu_fwd(a, w12, b12), ("g", "ab")
    if kernel == "swiglu_bwd":
        dy, w3, ab = ref.make_swiglu_bwd(family, *SW_SHAPE, seed)
        return emu_swiglu_bwd(dy, w3, ab, mutation), ref.ref_swiglu_bwd(dy, w3, ab), ("dab",)
    if kernel == "tn":
        y, x = ref.make_tn(family, *TN_SHAPE, seed)
        return emu_tn(y, x, mutation), ref.ref_tn(y, x), ("dw", "db")
    if kernel == "ln":
        x_bf16, residual = variant
        x, res, gm, bt, cy, ch = ref.make_ln(family, *LN_SHAPE, seed, x_bf16=x_bf16)
        res = res if residual else None
        return emu_ln(x, res, gm, bt, cy, ch, mutation), ref.ref_ln(x, res, gm, bt, cy, ch), LN_OUT
    if kernel == "swiglu_mixed":
        ab, cot = ref.make_ab_cot(family, *MX_SHAPE, seed)
        return emu_swiglu_mixed(ab, cot, mutation), ref.ref_swiglu_mixed(ab, cot), ("g", "dab")
    raise ValueError(kernel)


FAMILIES = {"nt": ref.GEMM_FAMILIES, "nn": ref.GEMM_FAMILIES, "swiglu_fwd": ref.GEMM_FAMILIES,
            "swiglu_bwd": ref.GEMM_FAMILIES, "tn": ref.GEMM_FAMILIES[:4], "ln": ref.LN_FAMILIES,
            "swiglu_mixed": ref.GEMM_FAMILIES}


@pytest.mark.parametrize("kernel,family", [(k, f) for k, fams in FAMILIES.items() for f in fams])
def test_bound_not_too_tight(kernel, family):
    got, R, names = case(kernel, family)
    for n, (nbad, worst) in ref.ratios(got, R, names).items():
        assert worst <= 0.5, f"{kernel}/{family} {n}: the emulated kernel reaches {worst:.3f} of the bound"


@pytest.mark.parametrize("variant", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("family", ref.LN_FAMILIES)
def test_ln_bound_not_too_tight_variants(family, variant):
    """x f32 and / or no residual (h = x exactly)."""
    got, R, names = case("ln", family, variant=variant)
    for n, (nbad, worst) in ref.ratios(got, R, names).items():
        assert worst <= 0.5, f"{family}/{variant} {n}: {worst:.3f}"


def test_saturate_has_overflowing_gates():
    """The family reaches the exp2 overflow (a log2e < -128) and the emulation returns +-0 there, never NaN."""
    got, R, _ = case("swiglu_fwd", "saturate")
    H = SW_SHAPE[1]
    a = R["ab"][:, :H]
    assert (a < -89).any() and (a > 89).any()
    assert torch.isfinite(got["g"]).all() and (got["g"][a < -100] == 0).all()
    got, R, _ = case("swiglu_bwd", "saturate")
    assert torch.isfinite(got["dab"]).all()


# mutation -> (kernel, families it must be flagged on)
MUTATIONS = {
    "last_row_unwritten": ("nt", ref.GEMM_FAMILIES),
    "k_tail_dropped": ("nt", ref.GEMM_FAMILIES),
    "bias_missing_last_group": ("nt", ref.GEMM_FAMILIES),
    "pad_step_repeats": ("nt", ref.GEMM_FAMILIES),
    "nn:last_row_unwritten": ("nn", ref.GEMM_FAMILIES),
    "nn:k_tail_dropped": ("nn", ref.GEMM_FAMILIES),
    "nn:pad_step_repeats": ("nn", ref.GEMM_FAMILIES),
    "pair_off_by_32": ("swiglu_fwd", ref.GEMM_FAMILIES),
    "silu_zero_below_-3": ("swiglu_fwd", ("unit", "outlier_rows", "binade", "saturate")),   # (cancel: |a| stays small)
    "exp2_no_log2e": ("swiglu_fwd", ref.GEMM_FAMILIES),
    "silu_prime_no_a_term": ("swiglu_bwd", ref.GEMM_FAMILIES),
    "swap_last8": ("swiglu_bwd", ref.GEMM_FAMILIES),
    "drop_step": ("tn", ref.GEMM_FAMILIES[:4]),
    "db_every_k_tile": ("tn", ref.GEMM_FAMILIES[:4]),
    "rstd_neighbour_row": ("ln", tuple(f for f in ref.LN_FAMILIES if f != "constant")),   # (constant: equal rstd)
    "one_pass_var": ("ln", ("offset", "constant")),      # (the other families: the f32 cancellation stays small)
    "dh16_before_dh_in": ("ln", ref.LN_FAMILIES),
    "sigmoid_bf16": ("swiglu_mixed", ref.GEMM_FAMILIES),
}


def _mut(m):
    return m.split(":", 1)[1] if ":" in m else m


@pytest.mark.parametrize("mutation,family", [(m, f) for m, (_, fams) in MUTATIONS.items() for f in fams])
def test_bound_flags_wrong_results(mutation, family):
    kernel = MUTATIONS[mutation][0]
    got, R, names = case(kernel, family)
    assert all(nbad == 0 for nbad, _ in ref.ratios(got, R, names).values())
    bad = ref.ratios(case(kernel, family, _mut(mutation))[0], R, names)
    assert any(nbad > 0 for nbad, _ in bad.values()), f"{mutation} on {family} inputs passes the bound: {bad}"


# ---------------------------------------------------------------------------------------------- the older criteria
def _rel(a, b):
    a, b = a.to(torch.float64), b.to(torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def old_criteria_pass(kernel, got, R):
    """The global checks of test_dense_bf16_gpu.py / test_mixed_gpu.py before the per-element bounds."""
    if kernel in ("nt", "nn"):
        exact = (got["c"] == R["c"].float().bfloat16().float()).float().mean().item()
        return _rel(got["c"], R["c"]) < 2 ** -8 and exact > 0.99
    if kernel == "swiglu_fwd":
        return _rel(got["g"], R["g"]) < 2 ** -8 and _rel(got["ab"], R["ab"]) < 2 ** -8
    if kernel == "swiglu_bwd":
        return _rel(got["dab"], R["dab"]) < 2e-2
    if kernel == "tn":
        return _rel(got["dw"], R["dw"]) < 2e-5 and _rel(got["db"], R["db"]) < 2e-5
    if kernel == "ln":
        return (_rel(got["y"], R["y"]) < 4e-3 and _rel(got["h"], R["h"]) < 2e-5 and _rel(got["dh"], R["dh"]) < 2e-5
                and _rel(got["dh16"], R["dh"]) < 8e-3 and _rel(got["dgamma"], R["dgamma"]) < 2e-5
                and _rel(got["dbeta"], R["dbeta"]) < 2e-5)
    if kernel == "swiglu_mixed":
        return _rel(got["g"], R["g"]) < 4e-3 and _rel(got["dab"], R["dab"]) < 8e-3
    raise ValueError(kernel)


def test_old_criteria_report(capsys):
    """Reports, without asserting, on which families the older global criteria pass each planted fault."""
    report = {}
    for m, (kernel, _) in MUTATIONS.items():
        passed, flagged = [], []
        for fam in FAMILIES[kernel]:
            got, R, names = case(kernel, fam, _mut(m))
            if old_criteria_pass(kernel, got, R):
                passed.append(fam)
            if any(nbad > 0 for nbad, _ in ref.ratios(got, R, names).values()):
                flagged.append(fam)
        report[m] = {"kernel": kernel, "old_criteria_pass_on": passed, "bound_flags_on": flagged}
    with capsys.disabled():
        print("\nplanted fault                  kernel         old global criteria pass on / per-element bound flags on")
        for m, r in report.items():
            print(f"{m:30s} {r['kernel']:14s} {','.join(r['old_criteria_pass_on']) or '-'} / {','.join(r['bound_flags_on'])}")
    path = os.environ.get("AMK_BF16_DENSE_OLD_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(report, f, indent=1)
