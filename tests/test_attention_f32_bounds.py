"""CPU checks of the f32 attention checker (tests/attn_f32_ref.py), no GPU needed.

The reference is the oracle: its o is ref_cpu.attention_core run in fp64, its gradients that function's autograd, its lse
the normaliser of the same weights.  Rounding the fp64 reference to f32 moves it by at most REF_FRACTION of any bound.
Not too tight: ref.emulate -- the f32 chain with the most roundings the bound allows -- stays under HALF of every
element's bound for every family x mask at (I, J) = (33, 65) and (130, 257), D in {32, 64, 256}, and under the split-bf16
product models at D = 64.  Tight enough to matter: each planted defect of the emulation puts elements outside the bound.

Which family catches which mutation (D = 64; x = elements outside the bound; measured with this file):

    mutation          mask, (B, H, I, J)        diffuse peaked needles large climb binade   tensors that leave the bound
    drop_key64        none, (2, 1, 33, 65)         x      x      -       x     x     x      o, lse, dv (dq, dk)
    dead_live_only    both, (2, 1, 33, 65)         x      x      x       x     x     x      o, dv
    causal_shift      triu, (2, 1, 33, 65)         x      x      x       x     x     x      all five
    drop_d2           none, (2, 1, 33, 65)         x      x      x       x     x     x      lse, dk, dv (o, dq)
    skip_rescale      none, (1, 1, 130, 257)       -      -      x       -     x     -      o, dq, dk
    dq_drop_block     none, (1, 1, 130, 257)       x      x      -       x     x     x      dq
    delta_bf16_o      none, (2, 1, 33, 65)         -      x      x       -     x     x      dq, dk
    drop_lh (x6)      none, (2, 2, 5, 1)           x      x      x       x     x     x      o

drop_key64 passes on needles (row 1's needle is not key 64: the dropped weight is 1e-11), skip_rescale where the
reference never moves after the first tile, dq_drop_block on needles (one-hot rows: dS is rounding noise), delta_bf16_o
where 2^-9 |dO.o| stays under the residue the bound allows dP - delta (diffuse, large: |dO||v| dominates).  drop_lh is
caught where the contraction is short: a lost (l, h) part is at most 2^-18 of a term, under gamma_(6n) from n = 8 on, so
it shows in o = P.V with one key (n = 1) and in nothing with 65 keys or 64 head dims."""
import pytest
import torch

import attn_f32_ref as ref
from oracle import ref_cpu

REF_FRACTION = 1 / 3   # 2^-24 |ref| against at least gamma_3 sum|t| in every bound (lse of a dead row: gamma_3 1e9)
SHAPES = [(33, 65), (130, 257)]


def _case(family, mask, B, H, I, J, D, seed, model="f32"):
    scale = D ** -0.5
    q, k, v, d_o = ref.make_inputs(family, B, H, I, J, D, scale, seed)
    km, cm = ref.make_masks(mask, B, I, J, seed)
    return (q, k, v, d_o, scale, km, cm), ref.reference(q, k, v, d_o, scale, km, cm, model=model)


@pytest.mark.parametrize("mask", ["none", "both", "dead_batch"])
def test_reference_is_the_oracle_in_fp64(mask):
    (q, k, v, d_o, scale, km, cm), R = _case("diffuse", mask, 2, 2, 33, 65, 64, 3)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    o = ref_cpu.attention_core(qd, kd, vd, scale, km, cm)
    grads = torch.autograd.grad((o * d_o.double()).sum(), [qd, kd, vd])
    assert torch.equal(R["o"], o.detach())
    for n, g in zip(("dq", "dk", "dv"), grads):
        assert float((R[n] - g).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1.0), n   # (per-batch vs batched sums)
    # lse is the normaliser of the oracle's own weights: exp(s - lse) are the weights that give o
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    s = s.masked_fill(ref._masked(2, 33, 65, km, cm), ref_cpu.FILL)
    # (fp64 holds s - lse to 2^-52 |lse|, which is 1e-7 in a dead row, where both are about -1e9)
    tol = 1e-12 + 2.0 ** -50 * R["lse"].abs().unsqueeze(-1)
    assert bool(((torch.exp(s - R["lse"].unsqueeze(-1)) @ v.double() - R["o"]).abs() <= tol).all())
    if mask != "none":   # a dead row: uniform over all J keys, no gradient to q
        dead = ref._masked(2, 33, 65, km, cm).expand(2, 2, 33, 65).all(-1)
        assert bool(dead.any())
        assert float((R["o"][dead] - v.double().mean(2, keepdim=True).expand(2, 2, 33, 64)[dead]).abs().max()) < 1e-12
        assert float(R["dq"][dead].abs().max()) == 0.0


@pytest.mark.parametrize("D", [32, 64, 256])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_reference_rounded_to_f32_is_a_small_fraction_of_the_bound(family, D):
    for mask, (B, H, I, J) in (("none", (1, 1, 1, 1)), ("both", (2, 1, 33, 65)), ("j1_masked", (1, 1, 5, 1)), ("none", (1, 2, 130, 257))):
        _, R = _case(family, mask, B, H, I, J, D, 5)
        rounded = {n: R[n].float() for n in ref.NAMES}
        for n, (nbad, worst) in ref.ratios(rounded, R).items():
            assert nbad == 0 and worst <= REF_FRACTION, (family, mask, D, n, worst)


def _half(family, mask, I, J, D, model):
    args, R = _case(family, mask, 2, 1, I, J, D, 1000 * D + I + len(family) + len(mask), model)
    res = ref.ratios(ref.emulate(*args, model=model), R)
    for n, (nbad, worst) in res.items():
        assert nbad == 0 and worst < 0.5, f"{model} {family}/{mask} ({I}, {J}) D={D} {n}: the emulation reaches {worst:.3f} of the bound"
    return max(w for _, w in res.values())


@pytest.mark.parametrize("D", [32, 64, 256])
@pytest.mark.parametrize("mask", ref.MASKS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_emulation_stays_under_half_of_every_bound(family, mask, D):
    worst = max(_half(family, mask, I, J, D, "f32") for I, J in SHAPES)
    print(f"{family}/{mask} D={D}: worst ratio {worst:.4f}")


@pytest.mark.parametrize("model", ["x6fwd", "x6bwd", "x6"])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_split_bf16_emulation_stays_under_half_of_every_bound(family, model):
    worst = max(_half(family, mask, I, J, 64, model)
                for I, J in SHAPES for mask in (ref.MASKS if I == 33 else ("none", "both")))
    print(f"{model} {family}: worst ratio {worst:.4f}")


def test_one_key_needs_no_special_case():
    """J = 1: dq = dk = 0 in real arithmetic; the bound is the rounding residue of dP - delta and the emulation's noise
    sits inside it."""
    args, R = _case("diffuse", "none", 2, 2, 5, 1, 64, 9)
    assert float(R["dq"].abs().max()) < 1e-12 and float(R["bound_dq"].min()) > 0.0
    res = ref.ratios(ref.emulate(*args), R)
    assert all(nbad == 0 and worst < 0.5 for nbad, worst in res.values()), res


# mutation -> (mask, shape, model, the families that must flag it): the table of the module docstring
ALL = ref.FAMILIES
MUTATIONS = {
    "drop_key64": ("none", (2, 1, 33, 65), "f32", ("diffuse", "peaked", "large", "climb", "binade")),
    "dead_live_only": ("both", (2, 1, 33, 65), "f32", ALL),
    "causal_shift": ("triu", (2, 1, 33, 65), "f32", ALL),
    "drop_d2": ("none", (2, 1, 33, 65), "f32", ALL),
    "skip_rescale": ("none", (1, 1, 130, 257), "f32", ("climb", "needles")),
    "dq_drop_block": ("none", (1, 1, 130, 257), "f32", ("diffuse", "peaked", "large", "climb", "binade")),
    "delta_bf16_o": ("none", (2, 1, 33, 65), "f32", ("peaked", "needles", "climb", "binade")),
    "drop_lh": ("none", (2, 2, 5, 1), "x6", ALL),
}


@pytest.mark.parametrize("mutation,family", [(m, f) for m, spec in MUTATIONS.items() for f in spec[3]])
def test_bound_flags_the_mutation(mutation, family):
    mask, (B, H, I, J), model, _ = MUTATIONS[mutation]
    args, R = _case(family, mask, B, H, I, J, 64, 11, model)
    good = ref.ratios(ref.emulate(*args, model=model), R)
    assert all(nbad == 0 for nbad, _ in good.values()), good
    bad = ref.ratios(ref.emulate(*args, model=model, mutation=mutation), R)
    print(mutation, family, {n: (nbad, f"{w:.3g}") for n, (nbad, w) in bad.items() if nbad})
    assert any(nbad > 0 for nbad, _ in bad.values()), f"{mutation} on {family} inputs passes the bound: {bad}"


def test_climb_moves_the_lazy_reference_in_every_tile():
    """The family's promise: for the upper rows every 64-key tile's maximum passes the reference by more than 2^8."""
    D, I, J = 64, 130, 257
    q, k, _, _ = ref.make_inputs("climb", 1, 1, I, J, D, D ** -0.5, 11)
    x = (q.double() @ k.double().transpose(-1, -2)) * (D ** -0.5 * ref.LOG2E)
    tile_max = torch.stack([x[..., j0:j0 + 64].amax(-1) for j0 in range(0, J, 64)], dim=-1)
    steps = tile_max[..., 1:] - tile_max[..., :-1]
    assert int((steps.amin(-1) > ref.LAZY_TAU).sum()) >= I // 4
    assert int((steps.amax(-1) < ref.LAZY_TAU).sum()) >= 1      # and rows that never move


def test_models_name_the_split_products_of_the_kernels():
    """The split products per model (read from csrc/attn_fwd_x6.hip and attn_bwd_fused_x6.hip) and the closed form."""
    assert ref.MODELS == {"f32": (), "x6fwd": ("s", "pv"), "x6bwd": ("dv", "dk"), "x6": ("s", "pv", "dv", "dk")}
    import attn_x6_ref as x6

    assert ref.chain(64, True) == x6.gamma(x6.N_CHAIN) * (1 + 2.0 ** -7) ** 2 + 2.0 ** -23 * (1 + 2.0 ** -9)
    assert ref.chain(64, False) == ref.gamma(65)
