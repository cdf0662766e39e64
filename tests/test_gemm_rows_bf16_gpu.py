"""amk_gemm_rows_bf16 on the GPU (csrc/gemm_rows_bf16.hip) against the fp64 reference and bounds of
tests/gemm_rows_bf16_ref.py: every (M, N, K) of its lists in three input families, f32 and bf16 output, with and without
the bias, poisoned padding behind every row's K elements, bitwise independence of a row from M, and the refusals."""
import ctypes

import pytest
import torch

import gemm_rows_bf16_ref as G

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
POISON = float("nan")   # behind a row's K elements: one read of it and the row's results are NaN


def _padded(t, device):
    """The bf16 matrix on the device, rows at a stride that is a multiple of 8 plus 8 more, the padding poisoned."""
    r, k = t.shape
    buf = torch.full((r, (k + 7) // 8 * 8 + 8), POISON, device=device, dtype=BF16)
    buf[:, :k] = t.to(device, BF16)
    return buf[:, :k]


@pytest.mark.parametrize("K", G.KS)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_every_shape_is_inside_the_bound(device, family, K):
    from amk import ops

    x, w, bias = G.make(family, K)
    xd, wd, bd = _padded(x, device), _padded(w, device), bias.to(device)
    worst = 0.0
    for with_bias in (True, False):
        R = G.reference(family, K, with_bias)
        for M in G.MS:
            for N in G.NS:
                b = bd[:N].contiguous() if with_bias else None
                y32 = ops.linear_rows_bf16(xd[:M], wd[:N], b, out_dtype=torch.float32)
                assert y32.dtype == torch.float32 and tuple(y32.shape) == (M, N)
                n_bad, ratio = G.outside_f32(y32, R, M, N)
                worst = max(worst, ratio)
                assert n_bad == 0, f"{family} M {M} N {N} K {K} bias {with_bias}: {n_bad} outside (worst {ratio:.2f}x)"
                y16 = ops.linear_rows_bf16(xd[:M], wd[:N], b, out_dtype=BF16)
                assert y16.dtype == BF16 and tuple(y16.shape) == (M, N)
                assert G.outside_bf16(y16.float(), R, M, N) == 0, f"{family} M {M} N {N} K {K} bias {with_bias}: bf16 output"
                # the bf16 output is the f32 output rounded once
                assert torch.equal(y16.view(torch.int16), y32.to(BF16).view(torch.int16))
    print(f"{family} K {K}: worst |err| / b32 {worst:.3f}")


@pytest.mark.parametrize("K", [170, 264])
def test_a_row_is_bitwise_independent_of_the_batch(device, K):
    from amk import ops

    x, w, bias = G.make("unit", K)
    xd, wd, bd = _padded(x, device), _padded(w, device), bias.to(device)
    full = ops.linear_rows_bf16(xd, wd, bd, out_dtype=torch.float32)          # M = 17
    again = ops.linear_rows_bf16(xd, wd, bd, out_dtype=torch.float32)
    assert torch.equal(full, again)
    for m in range(G.M_MAX):                                                    # M = 1, every row
        one = ops.linear_rows_bf16(xd[m:m + 1], wd, bd, out_dtype=torch.float32)
        assert torch.equal(one[0], full[m]), m
    eight = ops.linear_rows_bf16(xd[:8], wd, bd, out_dtype=BF16)
    assert torch.equal(eight.view(torch.int16), full[:8].to(BF16).view(torch.int16))


def test_unpadded_operands_and_refusals(device):
    from amk import lib, ops

    x, w, bias = G.make("unit", 170)
    R = G.reference("unit", 170)
    xd, wd, bd = x.to(device, BF16), w.to(device, BF16), bias.to(device)      # row stride 170: the op pads a copy
    y = ops.linear_rows_bf16(xd, wd, bd, out_dtype=torch.float32)
    assert G.outside_f32(y, R, G.M_MAX, G.N_MAX)[0] == 0
    assert torch.equal(y, ops.linear_rows_bf16(_padded(x, device), _padded(w, device), bd, out_dtype=torch.float32))
    with pytest.raises(RuntimeError, match="bf16 matrices"):
        ops.linear_rows_bf16(xd.float(), wd)
    with pytest.raises(RuntimeError, match="do not fit"):
        ops.linear_rows_bf16(xd, wd[:, :160])
    with pytest.raises(RuntimeError, match="float32 or bfloat16"):
        ops.linear_rows_bf16(xd, wd, out_dtype=torch.float16)
    L = lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    null = ctypes.c_void_p(0)
    xp, wp = _padded(x, device), _padded(w, device)
    out = torch.full((17, 132), 7.0, device=device)
    assert L.amk_gemm_rows_bf16(null, 184, p(wp), 184, null, p(out), 132, 17, 130, 170, 0, null) == -1
    assert L.amk_gemm_rows_bf16(p(xp), 184, p(wp), 184, null, p(out), 132, 0, 130, 170, 0, null) == -1
    assert L.amk_gemm_rows_bf16(p(xp), 170, p(wp), 184, null, p(out), 132, 17, 130, 170, 0, null) == -1    # ldx % 8
    assert L.amk_gemm_rows_bf16(p(xp), 184, p(wp), 184, null, p(out), 130, 17, 130, 170, 0, null) == -1    # ldy % 4
    assert L.amk_gemm_rows_bf16(p(xp), 184, p(wp), 184, null, p(out), 128, 17, 130, 170, 0, null) == -1    # ldy < N
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
