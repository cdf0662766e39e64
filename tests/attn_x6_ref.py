"""fp64 reference, per-element error bound, input families and an f32 emulation for the raw scores of the split-bf16
attention forward (csrc/attn_fwd_x6.hip), in the manner of tests/dense_f32_ref.py.

What the kernel computes.  q' = f32(q * qscale), qscale = f32(scale * log2 e): the f32 values the MFMAs are fed from.
Every f32 operand x is split  h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)  (round to nearest; both differences are
exact in f32), and the score of (query i, key j) is, per 16-deep block of the head dim (four blocks for D = 64), six MFMAs
v_mfma_f32_32x32x16_bf16 added into one f32 accumulator in the order  m m, l h, h l, m h, h m, h h  (K part first):
    S[i, j] = sum_d  (k_m q_m + k_l q_h + k_h q_l + k_m q_h + k_h q_m + k_h q_h)[d].

The bound (hard tier of tests/dense_f32_ref.py: |got - ref| <= gamma_n sum|t_i| + n 2^-126 for a sum of terms t_i with at
most n rounded f32 operations on any path).  With A = sum_d |q'_d| |k_d|:
* terms: the partial products.  A bf16 x bf16 product has 16 significant bits: exact in f32, no product rounding.
  bf16 keeps 8 significant bits, so rounding to it moves a value by at most 2^-8 of it:  |m| <= |x - h| <= 2^-8 |x|,
  |l| <= |x - h - m| <= 2^-16 |x|, and  |h| + |m| + |l| <= |x| (1 + 2^-8 + 2^-8 + 2^-16) <= |x| (1 + 2^-7), so
  sum|t_i| <= A (1 + 2^-7)^2.
* n, read off the source: six MFMAs per 16-deep block, four blocks, and each MFMA's own 16-product sum counted as at
  most 16 additions (its internal order and rounding points are not specified):  n = 6 * 4 * 16 = 384.
* truncation: what the six products leave out of q'_d k_d.
      split residual rho = x - h - m - l:  x - h - m is a multiple of ulp(x) = 2^(e-23) of magnitude <= 2^(e-16)
          (2^e <= |x|), that is at most 2^7 units: 8 significant bits, so l takes it exactly and rho = 0
          (three signed 8-bit parts hold the 24 bits of an f32; tests/test_attention_x6_bounds.py asserts it);
      dropped m l and l m:   2 * 2^-8 2^-16 = 2^-23
      dropped l l:           2^-32
  together  T = 2^-23 (1 + 2^-9) A.
  (bf16 has the exponent range of f32; the families below hold no non-zero value under 2^-60, so no part of a split
  underflows.)
      bound = gamma_384 (1 + 2^-7)^2 A + 2^-23 (1 + 2^-9) A + 384 * 2^-126.
No term is relative to a tensor's maximum.  The fp64 reference rounded to f32 differs from it by at most 2^-24 |ref| <=
2^-24 A, 1/400 of the bound: tests/test_attention_x6_bounds.py asserts that for every input used.
"""
import torch

U32 = 2.0 ** -24
FTZ = 2.0 ** -126
LOG2E32 = 1.4426950408889634   # AMK_LOG2E, rounded to f32 where it is used
N_CHAIN = 6 * 4 * 16
FAMILIES = ("unit", "outlier_rows", "binade", "cancel")
F64 = torch.float64


def gamma(n):
    return n * U32 / (1 - n * U32)


def make_qk(family, B, H, I, J, seed, D=64):
    """q (B, H, I, D), k (B, H, J, D), f32, on the CPU."""
    g = torch.Generator().manual_seed(int(seed))
    q = torch.randn(B, H, I, D, generator=g)
    k = torch.randn(B, H, J, D, generator=g)
    if family == "outlier_rows":   # a few rows a thousand times the rest
        q[:, :, ::7] *= 1000.0
        k[:, :, 3::11] *= 1000.0
    elif family == "binade":       # magnitudes spread over 2^-20 .. 2^20 along the head dim
        e = torch.randint(-20, 21, (D,), generator=g).float()
        q = q * torch.exp2(e)
        k = k * torch.exp2(-e + torch.randint(-3, 4, (D,), generator=g).float())
    elif family == "cancel":       # large terms that cancel: the sum is far below sum |t|
        k[..., 1::2] = k[..., 0::2]
        q[..., 1::2] = -q[..., 0::2] * (1.0 + 2.0 ** -12 * torch.randn(B, H, I, D // 2, generator=g))
        q, k = q * 64.0, k * 64.0
    elif family != "unit":
        raise ValueError(family)
    return q.contiguous(), k.contiguous()


def scaled_q(q, scale):
    """The f32 values the kernel splits: q * (scale * log2 e), both products rounded to f32 as the kernel rounds them."""
    qscale = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32)
    return q.float() * qscale.to(q.device)


def reference(q, k, scale):
    """(S in fp64 (B, H, I, J), per-element bound) from the f32 q' and k; any device."""
    qs = scaled_q(q, scale).to(F64)
    kd = k.to(F64)
    ref = torch.einsum("bhid,bhjd->bhij", qs, kd)
    A = torch.einsum("bhid,bhjd->bhij", qs.abs(), kd.abs())
    bound = gamma(N_CHAIN) * (1 + 2.0 ** -7) ** 2 * A + 2.0 ** -23 * (1 + 2.0 ** -9) * A + N_CHAIN * FTZ
    return ref, bound


def worst_ratio(got, ref, bound):
    """(elements outside the bound, worst |got - ref| / bound)."""
    err = (got.to(F64) - ref).abs()
    return int((err > bound).sum()), float((err / bound).max())


def split3(x):
    """The three bf16 parts of an f32 tensor, as f32 tensors (csrc/attn_fwd_x6.hip split1)."""
    h = x.to(torch.bfloat16).float()
    r1 = x - h
    m = r1.to(torch.bfloat16).float()
    l = (r1 - m).to(torch.bfloat16).float()
    return h, m, l


def emulate(q, k, scale, c0=None):
    """The kernel's chain in f32 on the CPU: per 16-deep block the six products in the kernel's order, each MFMA taken
    as sixteen sequential f32 additions of exact products into the accumulator (the most roundings the bound allows it).
    c0 (B, H, I, 1): the chain opens with it instead of zero (the variant with -mref as the C operand) and the result is
    S + c0."""
    qp = split3(scaled_q(q, scale))   # index 0, 1, 2 = h, m, l
    kp = split3(k.float())
    B, H, I, D = q.shape
    acc = torch.zeros(B, H, I, k.shape[2], dtype=torch.float32)
    if c0 is not None:
        acc = acc + c0.float()
    order = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))   # (K plane, Q plane): mfma6 of the kernel
    for c in range(D // 16):
        for ka, qa in order:
            for d in range(16 * c, 16 * c + 16):
                # bf16 x bf16: exact in f32, so this multiply rounds nothing
                acc = acc + qp[qa][..., :, None, d] * kp[ka][..., None, :, d]
    return acc


def unpack_scores(scores, B, H, I, J):
    """ScoreTiles -> (B, H, I, J): 32x32 tiles [b][h][key block][query block][key][query], both lengths padded to the
    forward's workgroups (128 queries, 64 keys)."""
    nqt, nkb = 4 * ((I + 127) // 128), 2 * ((J + 63) // 64)
    t = scores.view(B, H, nkb, nqt, 32, 32).permute(0, 1, 3, 5, 2, 4).reshape(B, H, nqt * 32, nkb * 32)
    return t[:, :, :I, :J]
