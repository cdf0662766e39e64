"""fp64 references, per-element bounds and an f32 CPU emulation with planted defects for the guided logits head of the
parallel decode under bf16 autocast: amk_cfg_layernorm_bf16 (csrc/mixed_bf16.hip) and amk_gemm_bf16_f32out
(csrc/gemm_bf16.hip).  The LayerNorm's error terms, the GEMM reference and the input families are those of
tests/bf16_dense_ref.py; u = 2^-8, u32 = 2^-24 as there.

* Guided LayerNorm.  Rows c and n are normalised as ln_mixed_fwd_kernel does it (two passes over the registers), so
  the f32 values yc = xhat_c gamma + beta and yn carry ref_ln's bound_y without its bf16 term 2u |y|: b_c, b_n.  The
  combine u = yn + s (yc - yn) is three f32 operations (a subtraction, a product, a sum; fewer where they contract):
      b = |s| b_c + |1 - s| b_n + 3 u32 (|n| + |s| |c - n| + |u|),
  and the one bf16 rounding is held in interval form: the stored element lies in [RNE(ref - b), RNE(ref + b)].
  Without the second row (or with s = 1, which the entry point maps to it) u = yc and b = b_c.
* GEMM with f32 output: the accumulators of gemm_bf16_kernel<false, 0> stored as they are,
      |c - ref| <= n u32 S,   n = 32 ceil(K / 32) + 1,   S = |A| |W|^T + |bias|;   no bf16 term.

emulate_cfg_ln / emulate_gemm redo the arithmetic in f32 on the CPU; `defect` plants one mistake a kernel of this kind
could make, and every one of them must leave the bound (tests/test_guided_head_bounds.py).
"""
import torch

import bf16_dense_ref as dref
from bf16_dense_ref import GEMM_FAMILIES, LN_EPS, LN_FAMILIES, U, U32, make_gemm, make_ln, ref_gemm, ref_ln  # noqa: F401
from gn_act_bf16_ref import bf16_rne

F32, F64 = torch.float32, torch.float64
LN_DEFECTS = ("swap_scale", "round_rows", "shared_stats", "beta_twice", "drop_tail")
GEMM_DEFECTS = ("round_acc", "drop_k", "bias_twice")


def make_cfg_ln(family, M, D, seed, bf16=False):
    """hc, hn (M, D), gamma, beta (D,): two rows of hidden states of one family (bf16 values if bf16), f32 tensors."""
    hc, _, gamma, beta, _, _ = make_ln(family, M, D, seed, x_bf16=bf16)
    hn, res, _, _, _, _ = make_ln(family, M, D, seed + 1000, x_bf16=bf16)
    if family == "offset":          # make_ln puts the offset into its residual: these rows carry it themselves
        hc, hn = hc + res, hn + res
        if bf16:
            hc, hn = dref.bf16_round(hc), dref.bf16_round(hn)
    return hc, hn, gamma, beta


def _ln_f32_part(x, gamma, beta):
    R = ref_ln(x, None, gamma, beta)
    return R["y"], R["bound_y"] - 2 * U * R["y"].abs()


def ref_cfg_ln(hc, hn, gamma, beta, s):
    """{"y": fp64 reference, "bound_y": b (the f32 value before the rounding), "lo_y", "hi_y": the bf16 interval}."""
    c, bc = _ln_f32_part(hc, gamma, beta)
    if hn is None:
        u, b = c, bc
    else:
        n, bn = _ln_f32_part(hn, gamma, beta)
        u = n + s * (c - n)
        b = abs(s) * bc + abs(1 - s) * bn + 3 * U32 * (n.abs() + abs(s) * (c - n).abs() + u.abs())
    return {"y": u, "bound_y": b, "lo_y": bf16_rne(u - b), "hi_y": bf16_rne(u + b)}


def inside(v, R):
    """lo <= v <= hi per element; v: the stored bf16 tensor (any device)."""
    v = v.detach().to("cpu", F64)
    return (R["lo_y"] <= v) & (v <= R["hi_y"]) & torch.isfinite(v)


def ref_gemm_f32(a, w, bias=None):
    """{"c", "bound_c"}: ref_gemm's reference with its chain term alone (no rounding to bf16 happens)."""
    R = ref_gemm(a, w, bias)
    return {"c": R["c"], "bound_c": R["bound_c"] - 2 * U * R["c"].abs()}


def outside_gemm(c, R):
    """The number of elements of c (f32, any device) outside the bound."""
    err = (c.detach().to("cpu", F64) - R["c"]).abs()
    return int((~(err <= R["bound_c"])).sum())


# ---------------------------------------------------------------------------------------------- f32 emulation
def _stats(x, drop_tail):
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / D
    v = x - mean
    q = v * v
    if drop_tail:
        q = q[..., :D - D % 64]
    rstd = 1.0 / torch.sqrt(q.sum(-1, keepdim=True) / D + torch.tensor(LN_EPS, dtype=F32))
    return v, rstd


def emulate_cfg_ln(hc, hn, gamma, beta, s, defect=None):
    """The stored bf16 tensor as the kernel's arithmetic gives it, in f32 on the CPU."""
    assert defect is None or defect in LN_DEFECTS
    g, b = gamma.to(F32), beta.to(F32)
    s = torch.tensor(s, dtype=F32)
    drop = defect == "drop_tail"
    vc, rc = _stats(hc.to(F32), drop)
    if hn is None:
        return (vc * rc * g + b).to(torch.bfloat16)
    vn, rn = _stats(hn.to(F32), drop)
    if defect == "shared_stats":
        vn, rn = hn.to(F32) - (hc.to(F32) - vc), rc
    if defect == "beta_twice":
        return ((1 - s) * (vn * rn * g) + s * (vc * rc * g) + (s.abs() + (1 - s).abs()) * b).to(torch.bfloat16)
    c, n = vc * rc * g + b, vn * rn * g + b
    if defect == "round_rows":
        c, n = dref.bf16_round(c), dref.bf16_round(n)
    u = c + s * (n - c) if defect == "swap_scale" else n + s * (c - n)
    return u.to(torch.bfloat16)


def emulate_gemm(a, w, bias=None, defect=None):
    """The f32 result as the kernel's arithmetic gives it, in f32 on the CPU (a, w hold bf16 values)."""
    assert defect is None or defect in GEMM_DEFECTS
    A, W = a.to(F32), w.to(F32)
    if defect == "drop_k":
        k = A.shape[1] // 32 * 32
        A, W = A[:, :k], W[:, :k]
    c = A @ W.t()
    if bias is not None:
        c = c + bias.to(F32) * (2 if defect == "bias_twice" else 1)
    if defect == "round_acc":
        c = dref.bf16_round(c)
    return c


# ---------------------------------------------------------------------------------------------- the algebra
def guided_form64(hc, hn, gamma, beta, w, s, eps=1e-5):
    """(guided, reference's order) in fp64: W (LN(hn) + s (LN(hc) - LN(hn))) and null + s (l - null), l = W LN(hc)."""
    ln = lambda x: torch.nn.functional.layer_norm(x.to(F64), x.shape[-1:], gamma.to(F64), beta.to(F64), eps)  # noqa: E731
    W = w.to(F64)
    yc, yn = ln(hc), ln(hn)
    l, null = yc @ W.t(), yn @ W.t()
    return (yn + s * (yc - yn)) @ W.t(), null + s * (l - null)
