"""fp64 reference, per-element error bounds and an f32 emulation for the split-bf16 weight gradient
(csrc/gemm_x6_tn.hip, dense.gemm_x6_tn), built from tests/gemm_x6_ref.py (the bound of a split-bf16 product) and
tests/dense_f32_ref.py (the bias gradient's bound, the input families, the checking).

What the kernel computes.  C[n, k] = sum_m Y[m, n] X[m, k].  Both operands are split h, m, l as gemm_x6_ref describes,
between the global load and the LDS store.  The M rows are cut into `nchunk` chunks of `spc` steps of BKM rows; a chunk's
step count is rounded up to even and rows past the chunk (and past M) are exact zeros.  Per 16 rows six MFMAs
v_mfma_f32_32x32x16_bf16 are added into one f32 accumulator in the order (Y part, X part) = m m, l h, h l, m h, h m, h h
(gemm_x6_ref.ORDER).  The chunks' partial tiles are then added in chunk order, starting from zero.

The bound of dW, with S = sum_m |y| |x|:  gemm_x6_ref.product_bound(n, S) with n read off gemm_x6_tn_kernel and
x6_tn_reduce_kernel: six MFMAs per 16 rows, each counted as at most 16 additions, so six roundings per row of the PADDED
chunk (BKM * the even step count), plus one addition per chunk in the ordered sum:  n = 6 BKM steps_even + nchunk.
(With one chunk the tile is stored directly; the one addition counted for it only loosens the bound by u.)

The bound of db is the one dense_f32_ref.ref_tn gives (the column sums are exact-f32 arithmetic on the pieces BEFORE
the split): a thread adds its BKM / YRP rows of every step in order, the YRP row groups of a column are folded in order,
then the chunks: BKM steps / YRP + YRP + nchunk additions.  ref_tn counts bk spc / 8 + 8 + nchunk, so it is called with
(bk, spc) that make the two counts equal -- (32, steps) for the four-wave kernel (YRP = 8), (8, steps + 8) for the eight-wave
one (YRP = 16, BKM = 16).

The families are gemm_x6_ref.FAMILIES (no non-zero value below 2^-60: no part of a split underflows); nothing is excluded.
"""
import torch

import dense_f32_ref as R32
import gemm_x6_ref as X6

F64 = torch.float64
FAMILIES = X6.FAMILIES


# ------------------------------------------------------------------------------------ the host code's choices, restated
def tile_k(N, K):
    """x6tn_tile_k(): 256 (eight waves, 16 rows per step) or 128 (four waves, 32 rows per step)."""
    return 256 if K >= 256 and ((N + 127) // 128) * ((K + 255) // 256) >= 12 else 128


def geometry(M, N, K, cus=256, tk=None):
    """(nchunk, steps per chunk, BKM, YRP) as x6tn_chunks() picks them; N = all rows of the launch (both segments)."""
    tk = tk or tile_k(N, K)
    bkm, yrp = (16, 16) if tk == 256 else (32, 8)
    tiles = ((N + 127) // 128) * ((K + tk - 1) // tk)
    steps, min_steps = (M + bkm - 1) // bkm, 256 // bkm
    chunks = max(1, cus // tiles)
    if chunks > steps // min_steps:
        chunks = max(1, steps // min_steps)
    spc = (steps + chunks - 1) // chunks
    return (steps + spc - 1) // spc, spc, bkm, yrp


def first_chunked_m(N, K, cus=256):
    """The smallest M that gives more than one chunk for an (N, K) gradient."""
    M = 1
    while geometry(M, N, K, cus)[0] < 2:
        M += 1
    return M


def n_chain(spc, nchunk, bkm):
    steps_even = (spc + 1) // 2 * 2
    return 6 * bkm * steps_even + nchunk


# ------------------------------------------------------------------------------------------------------- reference
def ref_tn(y, x, y2=None, want_bias=True, geo=None):
    """dense.gemm_x6_tn: outputs "dw", "dw2" (with y2) and "db" in the dictionary form of dense_f32_ref (so its
    measures / assert helpers apply); geo = geometry(M, N1 + N2, K) of the launch."""
    M, K = x.shape
    N = y.shape[1] + (y2.shape[1] if y2 is not None else 0)
    nchunk, spc, bkm, yrp = geo or geometry(M, N, K)
    n = n_chain(spc, nchunk, bkm)
    X = x.detach().to(F64)
    R = {}
    for name, yy in [("dw", y)] + ([("dw2", y2)] if y2 is not None else []):
        Y = yy.detach().to(F64)
        S = Y.abs().t() @ X.abs()
        ref = Y.t() @ X
        R[name], R["n_" + name], R["S_" + name] = ref, n, S
        R["abs_" + name] = torch.full_like(ref, n * R32.FTZ)
        R["bound_" + name] = X6.product_bound(n, S)
    if want_bias:
        bk, s = (32, spc) if yrp == 8 else (8, spc + 8)
        assert bk * s // 8 + 8 == bkm * spc // yrp + yrp
        B = R32.ref_tn(y, x, y2=y2, want_bias=True, spc=s, nchunk=nchunk, bk=bk)
        for k in ("db", "n_db", "S_db", "abs_db", "bound_db"):
            R[k] = B[k]
    return R


def outside(got, R, name):
    """(elements outside the bound, worst |got - ref| / bound) over every element."""
    err = (got.detach().to("cpu", F64).reshape(R[name].shape) - R[name]).abs()
    b = R["bound_" + name]
    bad = ~(err <= b)
    ratio = torch.where(err > 0, err / b, torch.zeros_like(err))
    return int(bad.sum()), float(ratio.max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------------------- emulation
def emulate_tn(y, x, geo):
    """The kernel's chain in f32 on the CPU: (dw, db).  Per chunk and 16 rows the six products in the kernel's order, every
    MFMA taken as sixteen sequential f32 additions of exact products (the most roundings the bound allows it); rows of
    padding add exact zeros and are skipped; the chunk partials are added in order from zero.  db: per thread row group
    (rows r, r + YRP, .. of every step), then the groups, then the chunks."""
    nchunk, spc, bkm, yrp = geo
    M, N = y.shape
    K = x.shape[1]
    yp, xp = X6.split3(y.float()), X6.split3(x.float())
    dw, db = torch.zeros(N, K), torch.zeros(N)
    for c in range(nchunk):
        m0, m1 = c * spc * bkm, min((c + 1) * spc * bkm, M)
        acc = torch.zeros(N, K)
        for b in range(m0, m1, 16):
            for pa, pb in X6.ORDER:
                for m in range(b, min(b + 16, m1)):
                    acc = acc + yp[pa][m][:, None] * xp[pb][m][None, :]   # bf16 x bf16: exact in f32
        dw = dw + acc
        groups = torch.zeros(yrp, N)
        for m in range(m0, m1):
            g = (m - m0) % bkm % yrp
            groups[g] = groups[g] + y[m].float()
        part = torch.zeros(N)
        for g in range(yrp):
            part = part + groups[g]
        db = db + part
    return dw, db
