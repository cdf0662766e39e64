"""The bounds of tests/guided_head_ref.py checked on the CPU: the f32 emulation of amk_cfg_layernorm_bf16 and
amk_gemm_bf16_f32out stays inside them on every input family, every planted defect leaves them, and the guided form
W (LN(h_null) + s (LN(h_cond) - LN(h_null))) is the reference's null + s (logits - null) in exact arithmetic."""
import pytest
import torch

import guided_head_ref as ref

LN_SHAPES = [(1, 4), (5, 252), (33, 260), (8, 1024)]
GEMM_SHAPES = [(1, 136, 1368), (127, 8, 24), (129, 120, 40), (65, 264, 96)]


@pytest.mark.parametrize("family", ref.LN_FAMILIES)
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_ln_emulation_inside(family, bf16):
    for i, (M, D) in enumerate(LN_SHAPES):
        hc, hn, gamma, beta = ref.make_cfg_ln(family, M, D, 10 + i, bf16=bf16)
        for s in (3.0, 1.0, 0.0):
            R = ref.ref_cfg_ln(hc, hn, gamma, beta, s)
            ok = ref.inside(ref.emulate_cfg_ln(hc, hn, gamma, beta, s), R)
            assert ok.all(), f"{family} M{M} D{D} s={s}: {int((~ok).sum())} elements outside"
        R = ref.ref_cfg_ln(hc, None, gamma, beta, 3.0)
        assert ref.inside(ref.emulate_cfg_ln(hc, None, gamma, beta, 3.0), R).all(), f"{family} M{M} D{D} one input"


@pytest.mark.parametrize("defect", ref.LN_DEFECTS)
def test_ln_defects_outside(defect):
    M, D = 33, 260          # D % 64 = 4: drop_tail leaves four elements out of the variance
    hc, hn, gamma, beta = ref.make_cfg_ln("unit", M, D, 21)
    R = ref.ref_cfg_ln(hc, hn, gamma, beta, 3.0)
    assert ref.inside(ref.emulate_cfg_ln(hc, hn, gamma, beta, 3.0), R).all()
    bad = ~ref.inside(ref.emulate_cfg_ln(hc, hn, gamma, beta, 3.0, defect=defect), R)
    assert bad.any(), f"{defect} stays inside the bound"


@pytest.mark.parametrize("family", ref.GEMM_FAMILIES)
def test_gemm_emulation_inside(family):
    for i, (M, N, K) in enumerate(GEMM_SHAPES):
        a, w, b = ref.make_gemm(family, M, N, K, 30 + i)
        for bias in (None, b):
            R = ref.ref_gemm_f32(a, w, bias)
            assert ref.outside_gemm(ref.emulate_gemm(a, w, bias), R) == 0, f"{family} {M}x{N}x{K} bias={bias is not None}"


@pytest.mark.parametrize("defect", ref.GEMM_DEFECTS)
def test_gemm_defects_outside(defect):
    M, N, K = 129, 120, 40   # K % 32 = 8: drop_k leaves the last partial step out
    a, w, b = ref.make_gemm("unit", M, N, K, 41)
    R = ref.ref_gemm_f32(a, w, b)
    assert ref.outside_gemm(ref.emulate_gemm(a, w, b), R) == 0
    assert ref.outside_gemm(ref.emulate_gemm(a, w, b, defect=defect), R) > 0, f"{defect} stays inside the bound"


def test_cpu_tensors_are_refused_and_the_gate_is_closed():
    from amk import ops

    h, w = torch.randn(3, 64), torch.randn(256, 64)
    assert not ops.guided_logits_ok(h, w)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not ops.guided_logits_ok(h, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.guided_logits(h, torch.ones(64), torch.zeros(64), w)


def test_argument_errors_come_back_as_codes():
    """No device is touched: every call below fails its argument checks first."""
    import ctypes

    from amk import lib

    L = lib.load()
    null, p = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    assert L.amk_cfg_layernorm_bf16(null, 0, null, 0, p, p, 3.0, 4, 64, 1e-5, p, null) == -1
    assert L.amk_cfg_layernorm_bf16(p, 0, null, 0, p, p, 3.0, 0, 64, 1e-5, p, null) == -1
    assert L.amk_cfg_layernorm_bf16(p, 0, null, 0, p, p, 3.0, 4, 62, 1e-5, p, null) == -2
    assert L.amk_cfg_layernorm_bf16(p, 0, null, 0, p, p, 3.0, 4, 4100, 1e-5, p, null) == -2
    assert L.amk_cfg_layernorm_bf16(p, 0, ctypes.c_void_p(4104), 0, p, p, 3.0, 4, 64, 1e-5, p, null) == -1
    assert L.amk_gemm_bf16_f32out(p, 64, p, 64, null, null, 256, 8, 256, 64, null) == -1
    assert L.amk_gemm_bf16_f32out(p, 64, p, 64, null, p, 256, 8, 256, 60, null) == -2
    assert L.amk_gemm_bf16_f32out(p, 64, p, 64, null, p, 254, 8, 256, 64, null) == -2
    assert L.amk_gemm_bf16_f32out(p, 64, p, 64, null, p, 128, 8, 256, 64, null) == -1           # ldc < N
    assert L.amk_gemm_bf16_f32out(p, 64, p, 64, null, ctypes.c_void_p(4100), 256, 8, 256, 64, null) == -1
    assert L.amk_gemm_bf16_f32out(p, 1 << 23, p, 64, null, p, 256, 8, 256, 64, null) == -2       # a 128-row panel of a past 1 GiB


@pytest.mark.parametrize("family", ["unit", "outlier_rows", "spike"])
def test_guided_form_is_the_reference_order(family):
    M, D, V = 24, 64, 256
    hc, hn, gamma, beta = ref.make_cfg_ln(family, M, D, 50)
    w = torch.randn(V, D, generator=torch.Generator().manual_seed(51)) * 0.02
    guided, reference = ref.guided_form64(hc, hn, gamma, beta, w, 3.0)
    assert float((guided - reference).abs().max()) <= 1e-12 * float(reference.abs().max())
