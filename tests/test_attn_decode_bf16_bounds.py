"""The bf16 decode attention's condition (tests/attn_decode_bf16_ref.py) on the CPU: an emulation of the kernel's chain
with the bf16 lane layout, rounded once, lies inside the RNE interval, and every planted fault lands outside it -- on
inputs where the reference itself is inside."""
import pytest
import torch

import attn_decode_bf16_ref as R16

B, H, CAP = 2, 3, 200
CASES = [(32, 1), (32, 33), (64, 65), (96, 128), (96, 200), (160, 129), (256, 200)]
FAULT_CASES = [c for c in CASES if c[1] > 1]


def _all(D):
    return R16.make_inputs(B, H, D, CAP + 1, seed=1000 + D)


def _case(D, J):
    q, k, v = _all(D)
    return q, k[:, :, :J].contiguous(), v[:, :, :J].contiguous(), D ** -0.5


@pytest.mark.parametrize("D,J", CASES)
def test_emulation_with_the_bf16_lane_layout_is_inside(D, J):
    q, k, v, scale = _case(D, J)
    ref, b32, lo, hi, _ = R16.reference(q, k, v, scale)
    f32 = R16.emulate_f32(q, k, v, scale)
    worst = float(((f32.double() - ref).abs() / b32).max())
    print(f"D {D} J {J}: f32 value |err| / b32 {worst:.3f}")
    assert worst <= 1.0
    assert R16.count_outside(R16.emulate(q, k, v, scale), lo, hi) == 0
    assert R16.count_outside(R16.bf16_rne(ref), lo, hi) == 0      # the reference, rounded, is inside


def test_emulation_with_masks_is_inside():
    q, k, v, scale = _case(64, 200)
    mask = torch.ones(B, 200, dtype=torch.bool)
    mask[0, 5::3] = False
    mask[1] = False
    ref, _, lo, hi, p = R16.reference(q, k, v, scale, mask)
    assert float((p[1] - 1.0 / 200).abs().max()) < 1e-15
    assert R16.count_outside(R16.emulate(q, k, v, scale, mask), lo, hi) == 0


@pytest.mark.parametrize("D,J", FAULT_CASES)
def test_planted_faults_are_outside(D, J):
    q, k_all, v_all = _all(D)
    scale = D ** -0.5
    k, v = k_all[:, :, :J].contiguous(), v_all[:, :, :J].contiguous()
    ref, _, lo, hi, p = R16.reference(q, k, v, scale)
    assert R16.count_outside(R16.bf16_rne(ref), lo, hi) == 0      # the reference alone is inside on these inputs

    def run(kk, vv):
        return R16.bf16_rne(R16.reference(q, kk, vv, scale)[0])

    def outside(got, sl=slice(None)):
        return R16.count_outside(got[sl], lo[sl], hi[sl]) > 0

    # a dropped key with p_j >= 1 / (2 J): for batch 0, head 0 the lightest such key, judged on that row alone
    p00 = p[0, 0]
    big = (p00 >= 1.0 / (2 * J)).nonzero().flatten()
    drop = int(big[p00[big].argmin()])
    keep = [j for j in range(J) if j != drop]
    got = run(k[:, :, keep], v[:, :, keep])
    assert R16.count_outside(got[0, 0], lo[0, 0], hi[0, 0]) > 0, "dropped key"
    # a length off by one, both ways
    assert outside(run(k[:, :, : J - 1], v[:, :, : J - 1])), "length - 1"
    assert outside(run(k_all[:, :, : J + 1], v_all[:, :, : J + 1])), "length + 1"
    # the new row's V taken from a stale cache row
    stale = v.clone()
    stale[:, :, J - 1] = v_all[:, :, J]
    assert outside(run(k, stale)), "stale V"
    # a swapped head stride
    assert outside(run(k.roll(1, dims=1), v.roll(1, dims=1))), "head stride"
    # the store cuts the f32 value to bf16 instead of rounding it to nearest even
    assert outside(R16.emulate(q, k, v, scale, truncate=True)), "truncated output"
    # p rounded to bf16 before the sums
    assert outside(R16.emulate(q, k, v, scale, round_p=True)), "p rounded to bf16"


@pytest.mark.parametrize("D,J", [c for c in FAULT_CASES if c[0] % 64 == 32])
def test_a_dropped_half_step_tail_is_outside(D, J):
    q, k, v, scale = _case(D, J)
    _, _, lo, hi, _ = R16.reference(q, k, v, scale)
    assert R16.count_outside(R16.emulate(q, k, v, scale), lo, hi) == 0
    assert R16.count_outside(R16.emulate(q, k, v, scale, drop_tail=True), lo, hi) > 0
