"""The bound of tests/gemm_x6_tn_ref.py against an f32 emulation of the split-bf16 weight gradient's chain (no GPU): the
emulation takes the most roundings the bound allows the kernel, and must stay inside it on every family."""
import pytest
import torch

import dense_f32_ref as R32
import gemm_x6_tn_ref as T

SHAPES = [(5, 8, 36), (70, 12, 52), (3, 4, 4)]
# the launch's own geometry (one chunk at these M), and chunked ones the kernel would pick for longer M: both step depths
GEOS = ["launch", (3, 1, 32, 8), (5, 1, 16, 16)]


def _geo(g, M, N, K):
    if g == "launch":
        return T.geometry(M, N, K)
    _, spc, bkm, yrp = g
    steps = -(-M // bkm)
    return -(-steps // spc), spc, bkm, yrp


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("geo", GEOS, ids=lambda g: g if isinstance(g, str) else "x".join(map(str, g)))
def test_emulation_inside_the_bound(family, shape, geo):
    M, N, K = shape
    D = R32.make_tn(family, M, N, K, seed=11 * M + N)
    g = _geo(geo, M, N, K)
    R = T.ref_tn(D["y"], D["x"], geo=g)
    dw, db = T.emulate_tn(D["y"], D["x"], g)
    for name, got in (("dw", dw), ("db", db)):
        nbad, ratio = T.outside(got, R, name)
        print(f"{family} {shape} {g} {name}: worst ratio {ratio:.3g}")
        assert nbad == 0, f"{name}: {nbad} elements outside the bound (worst {ratio:.3g}x)"


def test_bound_is_of_f32_size():
    """The bound stays an f32-level one: at the train step's longest chunk (dWo: 32 chunks of 1024 rows) it is below
    2^-10 S, three orders under one bf16 rounding (2^-9 per operand)."""
    nchunk, spc, bkm, _ = T.geometry(32768, 256, 512)
    n = T.n_chain(spc, nchunk, bkm)
    assert (nchunk, spc * bkm) == (32, 1024)
    assert T.X6.product_bound(n, 1.0) < 2.0 ** -10


def test_geometry_restates_the_step_shapes():
    """(tile width, chunks) at the five gradients of the ViT-VQGAN step, M = 32768, 256 CUs."""
    for (N, K), (tk, chunks) in {(1536, 256): (256, 21), (256, 512): (128, 32), (2736, 256): (256, 11), (256, 1368): (256, 21)}.items():
        assert T.tile_k(N, K) == tk
        assert T.geometry(32768, N, K)[0] == chunks
    assert T.first_chunked_m(4, 4) == 481   # 16 steps of 32 rows: two chunks of at least 256 rows' worth of steps


def test_two_segments_and_no_bias():
    D = R32.make_tn("unit", 37, 128, 20, seed=3, N2=68)
    R = T.ref_tn(D["y"], D["x"], y2=D["y2"], want_bias=False)
    assert R["dw"].shape == (128, 20) and R["dw2"].shape == (68, 20) and "db" not in R
    assert torch.equal(R["dw2"], D["y2"].double().t() @ D["x"].double())
