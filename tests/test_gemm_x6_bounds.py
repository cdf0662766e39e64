"""The per-element bounds of tests/gemm_x6_ref.py for the split-bf16 GEMM and its fused forms, without a GPU: an f32
emulation of the kernel's chain (split, six products per 16-deep block in the kernel's order, every MFMA as sixteen
sequential additions, the epilogue's f32 arithmetic) must stay inside them on every family.  The bound comes from the
source and the number formats; this test only shows that it is not violated by the arithmetic it describes."""
import pytest
import torch

import dense_f32_ref as R32
import gemm_x6_ref as ref

SHAPES = [(5, 8, 36), (9, 12, 52), (3, 4, 4)]   # (M, N or H, K): a 32-step tail, two steps, a single short step


def _check(got, want, bound, what):
    nbad, ratio = ref.worst_ratio(got, want, bound)
    print(f"{what}: worst |err| / bound = {ratio:.3f}")
    assert nbad == 0, f"{what}: {nbad} elements outside the bound, worst ratio {ratio:.3f}"


def test_split_is_exact():
    x = R32.make_act("binade", 64, 64, 0)
    h, m, l = ref.split3(x)
    assert torch.equal((h.double() + m.double() + l.double()).float(), x)


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_nt_emulation_within_bound(family, M, N, K):
    D = R32.make_nt(family, M, N, K, 11)
    for bias in (None, D["bias"]):
        want, bound = ref.ref_nt(D["a"], D["w"], bias)
        _check(ref.emulate_nt(D["a"], D["w"], bias), want, bound, f"nt {family} {(M, N, K)} bias={bias is not None}")


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_two_segment_emulation_within_bound(family):
    D = R32.make_nn(family, 7, 12, 32, 12, K2=36)
    wt, w2t = D["w"].t().contiguous(), D["w2"].t().contiguous()
    want, bound = ref.ref_nt(D["a"], wt, None, D["a2"], w2t)
    _check(ref.emulate_nt(D["a"], wt, None, D["a2"], w2t), want, bound, f"nt2 {family}")


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("M,H,K", SHAPES)
def test_swiglu_emulation_within_bound(family, M, H, K):
    D = R32.make_swiglu(family, M, H, K, 13)
    g, gb, ab, abb = ref.ref_nt_swiglu(D["a"], D["w"], D["bias"])
    ab32 = ref.emulate_nt(D["a"], D["w"], D["bias"])
    _check(ab32, ab, abb, f"(a | b) {family} {(M, H, K)}")
    _check(ref.emulate_gate(ab32), g, gb, f"gate {family} {(M, H, K)}")


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("M,H,K", SHAPES)
def test_swiglu_bwd_emulation_within_bound(family, M, H, K):
    D = R32.make_swiglu_bwd(family, M, H, K, 14)
    w3t = D["w3"].t().contiguous()
    want, bound = ref.ref_nt_swiglu_bwd(D["dy"], w3t, D["ab"])
    dg32 = ref.emulate_nt(D["dy"], w3t)
    _check(ref.emulate_gate_bwd(dg32, D["ab"]), want, bound, f"(dA | dB) {family} {(M, H, K)}")


def test_gate_order_round_trip():
    w12 = torch.arange(2 * 68 * 4, dtype=torch.float32).view(136, 4)
    out, rows = ref.gate_order(w12)
    assert out.shape == (256, 4) and torch.equal(out[rows], w12)
    assert torch.equal(out[64 + 3], w12[68 + 3]) and torch.equal(out[128 + 64 + 3], w12[68 + 67])
    assert not out[128 + 4:128 + 64].any() and not out[128 + 64 + 4:].any()
