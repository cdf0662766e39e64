"""The per-element bound of tests/attn_x6_ref.py for the split-bf16 attention scores, without a GPU: a torch CPU
emulation of the split and of the six-product chain in f32, in the kernel's order, against the fp64 reference."""
import os
import subprocess
import sys

import pytest
import torch

import attn_x6_ref as ref

SCALE = 64 ** -0.5
SHAPES = [(1, 1, 32, 32), (2, 2, 40, 77), (1, 2, 200, 130)]   # (B, H, I, J) of tests/test_attention_x6_keep_gpu.py
# worst |emulation - fp64| / bound over FAMILIES x SHAPES, measured with this file (the emulation rounds after every
# one of the 384 additions, in one fixed order: errors add like a random walk, far inside the worst case gamma_384)
EMU_WORST = 0.02178


def _cases():
    for si, shape in enumerate(SHAPES):
        for fi, family in enumerate(ref.FAMILIES):
            yield family, shape, 100 * si + fi


@pytest.fixture(scope="module")
def measured():
    out = {}
    for family, shape, seed in _cases():
        q, k = ref.make_qk(family, *shape, seed)
        want, bound = ref.reference(q, k, SCALE)
        out[(family, shape)] = (ref.worst_ratio(ref.emulate(q, k, SCALE), want, bound),
                                ref.worst_ratio(want.float(), want, bound))
    return out


def test_split_is_exact_to_the_residual_the_bound_assumes():
    """x = h + m + l exactly, with |m| <= 2^-8 |x| and |l| <= 2^-16 |x| (docstring of attn_x6_ref)."""
    for family in ref.FAMILIES:
        q, k = ref.make_qk(family, 1, 2, 50, 70, 7)
        for x in (ref.scaled_q(q, SCALE), k):
            h, m, l = ref.split3(x)
            xd, ax = x.double(), x.double().abs()
            assert bool((m.double().abs() <= 2.0 ** -8 * ax).all()) and bool((l.double().abs() <= 2.0 ** -16 * ax).all())
            assert bool((xd == h.double() + m.double() + l.double()).all())
            assert bool(((h.abs() + m.abs() + l.abs()).double() <= ax * (1 + 2.0 ** -7)).all())


def test_emulation_is_inside_the_bound(measured):
    for key, ((nbad, ratio), _) in measured.items():
        print(f"{key}: emulation worst ratio {ratio:.4f}")
        assert nbad == 0 and ratio <= 1.0, (key, nbad, ratio)


def test_emulation_worst_ratio_is_the_recorded_constant(measured):
    worst = max(r for (_, r), _ in measured.values())
    print(f"worst ratio {worst:.4f} (recorded {EMU_WORST})")
    assert worst <= EMU_WORST * 1.01, worst           # no input family got worse than what is written above
    assert worst >= EMU_WORST * 0.99, worst           # and the constant is the measurement, not a guess above it


def test_reference_rounded_to_f32_is_inside_the_bound(measured):
    for key, (_, (nbad, ratio)) in measured.items():
        assert nbad == 0 and ratio <= 1 / 384, (key, nbad, ratio)   # 2^-24 |ref| against > 384 * 2^-24 A


def test_reference_as_c_operand_misses_the_bound():
    """Why the unmasked kernel does not open its chains with -mref (the f32 kernel's form): with one outlier key in a row
    the accumulator starts at |mref| >> sum|q'||k| of the other keys, every partial product is rounded at ulp(mref), and
    those scores, taken relative to the reference, leave the bound the zero-opened chain keeps."""
    q, k = ref.make_qk("outlier_rows", 1, 1, 32, 64, 3)
    want, bound = ref.reference(q, k, SCALE)
    mref = want.max(dim=-1, keepdim=True).values.float()     # first tile: the reference is the row maximum
    nbad0, r0 = ref.worst_ratio(ref.emulate(q, k, SCALE), want, bound)
    nbad1, r1 = ref.worst_ratio(ref.emulate(q, k, SCALE, c0=-mref), want - mref.double(), bound)
    print(f"zero-opened chain: worst ratio {r0:.4f}; -mref as C: {nbad1} outside, worst ratio {r1:.2f}")
    assert nbad0 == 0 and nbad1 > 0 and r1 > 1.0


def test_unpack_scores_restates_the_tile_layout():
    """[b][h][key block][query block][key][query], padded to 128 queries / 64 keys (csrc/attn_common.h ScoreTiles)."""
    B, H, I, J = 2, 1, 130, 70
    nqt, nkb = 8, 4
    flat = torch.arange(B * H * nkb * nqt * 1024, dtype=torch.float32)
    s = ref.unpack_scores(flat, B, H, I, J)
    assert tuple(s.shape) == (B, H, I, J)
    b, i, j = 1, 129, 69
    want = (((b * H) * nkb + j // 32) * nqt + i // 32) * 1024 + (j % 32) * 32 + i % 32
    assert float(s[b, 0, i, j]) == float(want)


@pytest.mark.parametrize("env,want", [(None, "auto"), ("f32", "f32")])
def test_environment_selects_the_forward(env, want):
    """AMK_ATTENTION_FORWARD is read once, at import: auto unless set; f32 is the switch back to the f32 launches."""
    e = {k: v for k, v in os.environ.items() if k != "AMK_ATTENTION_FORWARD"}
    if env is not None:
        e["AMK_ATTENTION_FORWARD"] = env
    e["PYTHONPATH"] = os.pathsep.join(p for p in sys.path if p)
    out = subprocess.run([sys.executable, "-c", "from amk import ops; print(ops.ATTENTION_FORWARD)"],
                         env=e, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == want
