"""The decode attention's per-element bound (tests/attn_decode_ref.py) on the CPU: an f32 emulation of the kernel's chain,
summed in chunk order, stays inside it, and every planted fault lands outside it -- so the bound the GPU test asserts
can tell a wrong kernel from a right one."""
import pytest
import torch

import attn_decode_ref as R

B, H, CAP = 2, 3, 200
CASES = [(32, 1), (32, 33), (64, 65), (64, 200), (96, 128), (128, 129), (256, 200)]


def _case(D, J):
    q, k, v = R.make_inputs(B, H, D, CAP, seed=1000 + D)
    return q, k[:, :, :J].contiguous(), v[:, :, :J].contiguous(), D ** -0.5


@pytest.mark.parametrize("D,J", CASES)
def test_emulation_in_chunk_order_is_inside_the_bound(D, J):
    q, k, v, scale = _case(D, J)
    ref, bound, _ = R.reference(q, k, v, scale)
    n_bad, worst = R.worst_ratio(R.emulate(q, k, v, scale), ref, bound)
    print(f"D {D} J {J}: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, (n_bad, worst)
    # the fp64 reference rounded to f32 is far inside as well
    assert R.worst_ratio(ref.float(), ref, bound)[0] == 0


def test_emulation_with_masks_is_inside_the_bound():
    q, k, v, scale = _case(64, 200)
    mask = torch.ones(B, 200, dtype=torch.bool)
    mask[0, 5::3] = False          # partly masked
    mask[1] = False                # fully masked: uniform weights over all keys
    ref, bound, p = R.reference(q, k, v, scale, mask)
    assert float((p[1] - 1.0 / 200).abs().max()) < 1e-15
    n_bad, worst = R.worst_ratio(R.emulate(q, k, v, scale, mask), ref, bound)
    print(f"masked: worst |err| / bound {worst:.3f}")
    assert n_bad == 0, (n_bad, worst)


def _outside(got, ref, bound):
    return R.worst_ratio(got, ref, bound)[0] > 0


@pytest.mark.parametrize("D,J", [(32, 33), (64, 65), (64, 200), (128, 129), (256, 200)])
def test_planted_faults_are_outside_the_bound(D, J):
    q, k_all, v_all = R.make_inputs(B, H, D, CAP + 1, seed=1000 + D)
    scale = D ** -0.5
    k, v = k_all[:, :, :J], v_all[:, :, :J]
    ref, bound, p = R.reference(q, k, v, scale)

    def run(kk, vv):
        return R.reference(q, kk, vv, scale)[0]

    # a dropped key with p_j >= 1 / (2 J): for batch 0, head 0 the lightest such key, judged on that row alone
    p00 = p[0, 0]
    big = (p00 >= 1.0 / (2 * J)).nonzero().flatten()
    drop = int(big[p00[big].argmin()])
    keep = [j for j in range(J) if j != drop]
    assert _outside(run(k[:, :, keep], v[:, :, keep])[0, 0], ref[0, 0], bound[0, 0]), "dropped key"
    # a length off by one, both ways (the extra row is whatever the cache held there)
    if J > 1:
        assert _outside(run(k[:, :, : J - 1], v[:, :, : J - 1]), ref, bound), "length - 1"
    assert _outside(run(k_all[:, :, : J + 1], v_all[:, :, : J + 1]), ref, bound), "length + 1"
    # the new row's V taken from a stale cache row
    stale = v.clone()
    stale[:, :, J - 1] = v_all[:, :, J]
    assert _outside(run(k, stale), ref, bound), "stale V"
    # a swapped head stride: head h reads head h + 1's keys and values
    assert _outside(run(k.roll(1, dims=1), v.roll(1, dims=1)), ref, bound), "head stride"
