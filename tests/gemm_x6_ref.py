"""fp64 references, per-element error bounds and an f32 emulation for the split-bf16 dense GEMM and its fused forms
(csrc/gemm_x6.hip), in the manner of tests/attn_x6_ref.py (the bound of the product) and tests/dense_f32_ref.py (the
bound carried through the SwiGLU epilogues, and the input families, which are that file's).

What the kernel computes.  Every f32 operand x is split  h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)  (round to
nearest; both differences are exact in f32); the weight's parts come from the planes, the activation's are made between
its global load and its LDS store.  Per 16-deep block of the contraction (two per 32-step; K is padded to 32 with exact
zeros) six MFMAs v_mfma_f32_32x32x16_bf16 are added into one f32 accumulator in the order (A part, W part) =
m m, l h, h l, m h, h m, h h; a second contraction segment (amk_gemm_x6_nt2) continues the same chain.

The bound, with S = sum_k |a_k| |w_k| (+ |bias|):
* chain: gamma_n S (1 + 2^-7)^2.  The terms are the partial products (bf16 x bf16: exact in f32), whose magnitudes sum to
  at most S (1 + 2^-7)^2 (tests/attn_x6_ref.py).  n, read off gemm_x6_nt_kernel: six MFMAs per 16-deep block, each MFMA's
  own 16-product sum counted as at most 16 additions, so six roundings per element of the PADDED contraction (both
  segments padded on their own), plus the epilogue's bias addition:  n = 6 (Kp + Kp2) + 1.
* dropped partial products m l, l m, l l:  2^-23 (1 + 2^-9) S  (the split itself is exact: tests/attn_x6_ref.py).
* n 2^-126 for flushes, as tests/dense_f32_ref.py adds it.
The families (dense_f32_ref's unit, outlier_rows, binade, cancel) hold no non-zero value below 2^-60, so no part of a split
underflows; `saturate` is left out, so no element needs that file's underflow allowance and nothing is excluded.

Through the gate, exactly as dense_f32_ref.ref_nt_swiglu / ref_nn_swiglu_bwd do it, with e = the bound above in the place
of their ea, eb, eG (the epilogues are the same f32 arithmetic: accurate expf, IEEE division).
"""
import torch

import dense_f32_ref as R32

U32, FTZ, F64 = R32.U32, R32.FTZ, torch.float64
FAMILIES = ("unit", "outlier_rows", "binade", "cancel")
ORDER = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))   # (A plane, W plane) of the six MFMAs: PA / PB of the kernel


def pad32(k):
    return -(-k // 32) * 32


def n_chain(K, K2=0):
    return 6 * (pad32(K) + (pad32(K2) if K2 else 0)) + 1


def product_bound(n, S):
    return float(R32.gamma(n)) * (1 + 2.0 ** -7) ** 2 * S + 2.0 ** -23 * (1 + 2.0 ** -9) * S + n * FTZ


def _d(t):
    return None if t is None else t.detach().to(F64)


def ref_nt(a, w, bias=None, a2=None, w2=None):
    """a w^T (+ bias) (+ a2 w2^T): (ref fp64, bound)."""
    A, W = _d(a), _d(w)
    C, S = A @ W.t(), A.abs() @ W.abs().t()
    if a2 is not None:
        C, S = C + _d(a2) @ _d(w2).t(), S + _d(a2).abs() @ _d(w2).abs().t()
    if bias is not None:
        C, S = C + _d(bias), S + _d(bias).abs()
    return C, product_bound(n_chain(a.shape[1], a2.shape[1] if a2 is not None else 0), S)


def ref_nt_swiglu(a, w12, b12=None):
    """(g ref, g bound, (a | b) ref, (a | b) bound) of amk_gemm_x6_nt_swiglu."""
    AB, e = ref_nt(a, w12, b12)
    H = AB.shape[1] // 2
    x, y, ex, ey = AB[:, :H], AB[:, H:], e[:, :H], e[:, H:]
    s = torch.sigmoid(x)
    g = x * s * y
    sp = s * (1 + x * (1 - s))
    lin = (sp * y).abs() * ex + (x * s).abs() * ey + g.abs() * (R32._eps_s(s) + 2 * U32) + 0.25 * ex * ex * y.abs() + ex * ey
    return g, lin + n_chain(a.shape[1]) * FTZ, AB, e


def ref_nt_swiglu_bwd(dy, w3t, ab):
    """((dA | dB) ref, bound) of amk_gemm_x6_nt_swiglu_bwd; w3t = W3^T (H, K), the matrix whose planes the kernel reads."""
    G, eG = ref_nt(dy, w3t)
    AB = _d(ab)
    H = G.shape[1]
    A, B = AB[:, :H], AB[:, H:]
    s = torch.sigmoid(A)
    eps_s = R32._eps_s(s)
    sp = s * (1 + A * (1 - s))
    E_sp = s * ((1 + A - 2 * A * s).abs() * eps_s + 2 * U32 * A.abs() * (1 - s) + U32 * (1 + A * (1 - s)).abs()) + U32 * sp.abs()
    da, db = G * B * sp, G * A * s
    lda = (B * sp).abs() * eG + (G * B).abs() * E_sp + 2 * U32 * da.abs() + B.abs() * eG * E_sp
    ldb = (A * s).abs() * eG + db.abs() * (eps_s + 2 * U32) + (A * s).abs() * eG * (eps_s + 2 * U32)
    return torch.cat([da, db], 1), torch.cat([lda, ldb], 1) + n_chain(dy.shape[1]) * FTZ


def worst_ratio(got, ref, bound):
    """(elements outside the bound, worst |got - ref| / bound)."""
    err = (got.to(F64) - ref).abs()
    return int((err > bound).sum()), float((err / bound).max())


def split3(x):
    """The three bf16 parts of an f32 tensor, as f32 tensors (split1 of the kernel)."""
    h = x.to(torch.bfloat16).float()
    r1 = x - h
    m = r1.to(torch.bfloat16).float()
    return h, m, (r1 - m).to(torch.bfloat16).float()


def emulate_nt(a, w, bias=None, a2=None, w2=None):
    """The kernel's chain in f32 on the CPU: per 16-deep block the six products in the kernel's order, every MFMA taken as
    sixteen sequential f32 additions of exact products (the most roundings the bound allows it); the padding adds exact
    zeros and is skipped; the bias last."""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for x, y in ((a, w),) + (((a2, w2),) if a2 is not None else ()):
        xp, yp = split3(x.float()), split3(y.float())
        K = x.shape[1]
        for c in range(0, K, 16):
            for pa, pb in ORDER:
                for k in range(c, min(c + 16, K)):
                    acc = acc + xp[pa][:, None, k] * yp[pb][None, :, k]   # bf16 x bf16: exact in f32
    return acc + bias.float() if bias is not None else acc


def emulate_gate(ab32):
    """silu(a) b in the epilogue's f32 arithmetic."""
    H = ab32.shape[1] // 2
    a, b = ab32[:, :H], ab32[:, H:]
    return a * (1.0 / (1.0 + torch.exp(-a))) * b


def emulate_gate_bwd(dg32, ab32):
    H = ab32.shape[1] // 2
    a, b = ab32[:, :H], ab32[:, H:]
    sg = 1.0 / (1.0 + torch.exp(-a))
    return torch.cat([dg32 * b * (sg * (1.0 + a * (1.0 - sg))), dg32 * (a * sg)], 1)


def gate_order(w12):
    """w12 (2H, K) -> its rows in the gate order of amk_gemm_x6_nt_swiglu (128 ceil(H / 64) rows, zero rows as padding),
    and the index tensor (plane row of every row of w12) that undoes it."""
    H = w12.shape[0] // 2
    j = torch.arange(H)
    rows = torch.cat([128 * (j // 64) + j % 64, 128 * (j // 64) + 64 + j % 64])
    out = torch.zeros(128 * -(-H // 64), w12.shape[1], dtype=w12.dtype, device=w12.device)
    out[rows.to(w12.device)] = w12
    return out, rows


def split_planes_gpu(w):
    """[3][R][K padded] bf16 planes of a device matrix by amk_gemm_x6_split (the per-call split the table-driven one must
    reproduce bit for bit)."""
    from amk import lib, ops

    L = lib.load()
    R, K = w.shape
    out = torch.empty(L.amk_gemm_x6_planes_bytes(R, K) // 2, device=w.device, dtype=torch.bfloat16)
    lib.check(L.amk_gemm_x6_split(ops._ptr(w), w.stride(0), R, K, ops._ptr(out), ops._stream()), "amk_gemm_x6_split")
    return out.view(3, R, pad32(K))
