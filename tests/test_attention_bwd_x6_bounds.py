"""The tolerance of tests/attn_bwd_x6_ref.py for the split-bf16 dV / dK products of the attention backward, without a GPU:
the f32 emulation of the six-product accumulation stays within FACTOR of the emulated f32 MFMA chain's figure on the same
operands, and planted defects of the kind the kernel could have land outside it -- for every input family and mask the
GPU test (tests/test_attention_bwd_x6_gpu.py) uses."""
import os
import subprocess
import sys

import pytest
import torch

import attn_bwd_x6_ref as ref

SCALE = 64 ** -0.5
SHAPES = [(2, 2, 40, 77), (1, 1, 95, 130)]   # (B, H, I, J): ragged query tiles, more than one, keys past a 32-key wave


def _cases():
    for si, shape in enumerate(SHAPES):
        for fi, family in enumerate(ref.FAMILIES):
            for mi, mode in enumerate(ref.MASKS):
                yield family, mode, shape, 1000 * si + 100 * fi + 10 * mi


@pytest.fixture(scope="module")
def products():
    """Per case and product: (x, y, fp64 sum of the f32 operands, its scale A, the f32 chain's figure)."""
    out = {}
    for family, mode, shape, seed in _cases():
        q, k, v, d_o = ref.make_inputs(family, *shape, seed)
        km, cm = ref.make_masks(mode, shape[0], shape[2], shape[3])
        r = ref.reference(q, k, v, d_o, SCALE, km, cm)
        for name, (x, y) in zip(("dv", "dk"), ref.kernel_operands(q, d_o, r, SCALE)):
            want = torch.einsum("bhid,bhij->bhjd", x.double(), y.double())
            A = torch.einsum("bhid,bhij->bhjd", x.double().abs(), y.double().abs())
            out[(family, mode, shape, name)] = (x, y, want, A, ref.figure(ref.emulate_f32(x, y), want, A))
    return out


def test_slot_rows_are_the_accumulator_rows_of_registers_8t_to_8t_plus_7():
    acc_row = lambda r, hf: (r & 3) + 8 * (r >> 2) + 4 * hf   # csrc/amk_common.h
    for t in (0, 1):
        assert ref.slot_rows(t) == [acc_row(8 * t + j, hf) for hf in (0, 1) for j in range(8)]
        assert sorted(ref.slot_rows(t)) == ref.slot_rows(t, packed=False)


def test_emulation_is_within_the_factor_of_the_f32_chain(products):
    """With one rounding per MFMA.  The per-product model (96 roundings per 16 queries against the f32 chain's 16) is
    printed: it sits at about the factor itself, which is why the hardware's measured 1.5e-6 against 2.6e-6
    (tools/ubench_bf16x6.hip) and not that model stands behind the factor."""
    for key, (x, y, want, A, fig32) in products.items():
        fig = ref.figure(ref.emulate_x6(x, y), want, A)
        worst = ref.figure(ref.emulate_x6(x, y, per_product=True), want, A)
        print(f"{key}: six products {fig[0]:.3e} (rounding after every product: {worst[0]:.3e}), f32 chain {fig32[0]:.3e}")
        assert ref.within_factor(fig, fig32), (key, fig, fig32)


DEFECTS = {
    "smallest partial product dropped": dict(order=ref.ORDER[1:]),
    "m x h dropped": dict(order=ref.ORDER[:3] + ref.ORDER[4:]),
    "planes in the wrong pairing (l x m for l x h)": dict(order=((1, 1), (2, 1), (0, 2), (1, 0), (0, 1), (0, 0))),
    "k-slot 1 read in natural order": dict(natural_slot=1),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects_land_outside(products, defect):
    for key, (x, y, want, A, fig32) in products.items():
        fig = ref.figure(ref.emulate_x6(x, y, **DEFECTS[defect]), want, A)
        print(f"{key}: {defect}: {fig[0]:.3e} against {ref.FACTOR} x {fig32[0]:.3e}")
        assert not ref.within_factor(fig, fig32), (key, defect, fig, fig32)


@pytest.mark.parametrize("env,want", [(None, "auto"), ("0", "0"), ("1", "1")])
def test_environment_selects_the_backward(env, want):
    """AMK_ATTN_BWD_X6 is read once, at import: auto unless set; 0 is the switch back to the f32 products."""
    e = {k: v for k, v in os.environ.items() if k != "AMK_ATTN_BWD_X6"}
    if env is not None:
        e["AMK_ATTN_BWD_X6"] = env
    e["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    out = subprocess.run([sys.executable, "-c", "from amk import ops; print(ops.ATTENTION_BACKWARD_X6)"],
                         env=e, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == want
