"""fp64 reference, per-element bound and a CPU emulation for the few-row bf16 GEMM (csrc/gemm_rows_bf16.hip,
amk_gemm_rows_bf16):  Y (M, N) = X (M, K) . W (N, K)^T + bias, bf16 operands, f32 bias, f32 accumulation, Y f32 or bf16.

Reference: fp64 on the values the kernel sees (bf16 operands exactly, the f32 bias as given).  S = |X| |W|^T + |bias|,
u32 = 2^-24.

Bound, derived as tests/bf16_dense_ref.py derives its NT rule (bf16 x bf16 products are exact in f32; an MFMA step adds
its 32 products into the accumulator, charged as 32 f32 additions; a padded product is an exact zero).  The kernel's
longest addition path of one output element, read off the source:
  * a workgroup's four waves split the ceil(K / 32) steps of 32: wave w takes steps w, w + 4, ..., at most
    T = ceil(ceil(K / 32) / 4) of them, summed into ONE accumulator by v_mfma_f32_16x16x32_bf16: 32 T additions;
  * the four partial tiles are added in wave order, ((t0 + t1) + t2) + t3: 3 additions;
  * the f32 bias: 1 addition.
      f32 output:   |got - ref| <= b32 = n u32 S,    n = 32 T + 4.
  * bf16 output: the kernel stores RNE(v) of that f32 value v and rounds nothing else; RNE is monotone, so
      RNE(ref - b32) <= got <= RNE(ref + b32),
    evaluated exactly in fp64 (gn_act_bf16_ref.bf16_rne).  Not a 2 u |ref| allowance: a truncated store lands outside.
No term is relative to a tensor's maximum.  (K = 264: 9 steps, T = 3, n = 100; K = 8 .. 128: T = 1, n = 36.)

Families: unit, cancel and binade of bf16_dense_ref.make_gemm.  Shapes: M in {1, 2, 8, 16, 17} (one row, a batch, a full
row block, a second block of one row), N in {1, 16, 48, 130} (a column tail of 1 and of 2 behind full tiles), K in
{8, 40, 170, 264} (less than a step; a step and a piece; the FFN width at dim 64, whose last 16-byte piece straddles K;
more than two rounds of the four waves).  The operands of a smaller M or N are the leading rows of the (17, 130) draw, so
that one reference serves them all and row m can be compared bitwise across M.
"""
import functools

import torch

import bf16_dense_ref as dense
from bf16_dense_ref import bf16_round
from gn_act_bf16_ref import bf16_rne

U32 = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
FAMILIES = ("unit", "cancel", "binade")
MS = (1, 2, 8, 16, 17)
NS = (1, 16, 48, 130)
KS = (8, 40, 170, 264)
M_MAX, N_MAX = max(MS), max(NS)


def chain(K):
    """n of the docstring: the longest addition path of one output element."""
    steps = (K + 31) // 32
    return 32 * ((steps + 3) // 4) + 4


@functools.lru_cache(maxsize=None)
def make(family, K):
    """x (17, K), w (130, K) bf16 values as f32, bias (130) f32: the draw every (M, N) of a (family, K) slices."""
    return dense.make_gemm(family, M_MAX, N_MAX, K, seed=7000 + K)


@functools.lru_cache(maxsize=None)
def reference(family, K, with_bias=True):
    """{"y", "b32", "lo", "hi"} at (17, 130): slice [:M, :N] for a smaller shape (rows and columns are independent)."""
    x, w, bias = make(family, K)
    X, W = x.to(F64), w.to(F64)
    y, S = X @ W.t(), X.abs() @ W.abs().t()
    if with_bias:
        y, S = y + bias.to(F64), S + bias.to(F64).abs()
    b32 = chain(K) * U32 * S
    return {"y": y, "b32": b32, "lo": bf16_rne(y - b32), "hi": bf16_rne(y + b32)}


def outside_f32(got, R, M, N):
    """(elements outside the f32 bound, worst |err| / b32) of a (M, N) f32 result."""
    err = (got.to("cpu", F64) - R["y"][:M, :N]).abs()
    b = R["b32"][:M, :N]
    bad = ~(err <= b)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    return int(bad.sum()), float(ratio.max())


def outside_bf16(got, R, M, N):
    """Elements of a (M, N) bf16 result outside [RNE(ref - b32), RNE(ref + b32)]."""
    g = got.to("cpu", F64)
    ok = (R["lo"][:M, :N] <= g) & (g <= R["hi"][:M, :N]) & torch.isfinite(g)
    return int((~ok).sum())


def bf16_truncate(x):
    return (x.to(F32).contiguous().view(torch.int32) & -65536).view(F32)


def emulate_f32(x, w, bias, drop_k_tail=False, bias_bf16=False, acc_bf16=False):
    """The kernel's chain in f32 on the CPU: each wave's steps into one accumulator (a product at a time: no fewer
    roundings than the MFMA's), the four partial tiles in wave order, the bias.  Faults: drop_k_tail leaves out the
    last, partial step of 32; bias_bf16 rounds the bias to bf16; acc_bf16 rounds the accumulator to bf16 after every add."""
    M, K = x.shape
    N = w.shape[0]
    x, w = x.to(F32), w.to(F32)
    rnd = bf16_round if acc_bf16 else (lambda t: t)
    steps = (K + 31) // 32
    parts = []
    for wave in range(4):
        acc = torch.zeros(M, N, dtype=F32)
        for s in range(wave, steps, 4):
            k1 = min(32 * s + 32, K)
            if drop_k_tail and k1 - 32 * s < 32:
                continue
            for k in range(32 * s, k1):
                acc = rnd(acc + x[:, k:k + 1] * w[:, k][None, :])
        parts.append(acc)
    y = rnd(rnd(rnd(parts[0] + parts[1]) + parts[2]) + parts[3])
    if bias is not None:
        y = rnd(y + (bf16_round(bias) if bias_bf16 else bias).to(F32)[None, :])
    return y


def emulate(x, w, bias, out_bf16, truncate=False, swap_rows=False, **faults):
    """What the kernel stores.  truncate: the bf16 store cuts instead of rounding; swap_rows: rows 15 and 16 exchanged."""
    y = emulate_f32(x, w, bias, **faults)
    if swap_rows:
        y = y.clone()
        y[[15, 16]] = y[[16, 15]]
    if out_bf16:
        return bf16_truncate(y) if truncate else bf16_round(y)
    return y
