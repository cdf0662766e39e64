"""The few-row bf16 GEMM's bound (tests/gemm_rows_bf16_ref.py) on the CPU: an emulation of the kernel's chain lies inside
it for every family, K and output type, and each planted fault lands outside it."""
import pytest
import torch

import gemm_rows_bf16_ref as G


@pytest.mark.parametrize("K", G.KS)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_emulation_is_inside(family, K):
    x, w, bias = G.make(family, K)
    for with_bias in (True, False):
        R = G.reference(family, K, with_bias)
        b = bias if with_bias else None
        y32 = G.emulate(x, w, b, out_bf16=False)
        n_bad, worst = G.outside_f32(y32, R, G.M_MAX, G.N_MAX)
        print(f"{family} K {K} bias {with_bias}: worst |err| / b32 {worst:.3f}")
        assert n_bad == 0, (n_bad, worst)
        assert G.outside_bf16(G.emulate(x, w, b, out_bf16=True), R, G.M_MAX, G.N_MAX) == 0
        assert G.outside_bf16(G.bf16_rne(R["y"]), R, G.M_MAX, G.N_MAX) == 0


def test_a_row_does_not_depend_on_the_others():
    x, w, bias = G.make("unit", 170)
    full = G.emulate(x, w, bias, out_bf16=False)
    for m in (0, 15, 16):
        assert torch.equal(G.emulate(x[m:m + 1], w, bias, out_bf16=False)[0], full[m])


@pytest.mark.parametrize("K", G.KS)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_planted_faults_are_outside(family, K):
    x, w, bias = G.make(family, K)
    R = G.reference(family, K)
    M, N = G.M_MAX, G.N_MAX

    def bad32(**faults):
        return G.outside_f32(G.emulate(x, w, bias, out_bf16=False, **faults), R, M, N)[0]

    assert bad32() == 0
    assert bad32(drop_k_tail=True) > 0, "the K tail dropped"
    assert bad32(bias_bf16=True) > 0, "the bias rounded to bf16"
    assert bad32(acc_bf16=True) > 0, "bf16 accumulation"
    assert bad32(swap_rows=True) > 0, "rows 15 and 16 swapped"
    assert G.outside_bf16(G.emulate(x, w, bias, out_bf16=True), R, M, N) == 0
    assert G.outside_bf16(G.emulate(x, w, bias, out_bf16=True, truncate=True), R, M, N) > 0, "a truncated store"
    assert G.outside_bf16(G.emulate(x, w, bias, out_bf16=True, swap_rows=True), R, M, N) > 0
