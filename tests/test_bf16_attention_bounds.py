"""CPU checks of the bf16 attention checker (tests/bf16_attention_ref.py), no GPU needed.

Not too tight: an emulation of the rounding points csrc/attn_bf16.hip documents (f32 scores and softmax, P and dS rounded
to bf16 with round-to-nearest-even for the products, f32 accumulation, dQ as per-256-key-block f32 partials summed in
order, every output rounded once) stays within half of every element's bound, over every input family and the masks.
Sensitive enough: results that are wrong the way a kernel goes wrong -- a key dropped, a 32-query tail left unwritten,
two heads swapped, a 256-key block missing from dQ, delta taken from the wrong row, a key mask ignored -- are flagged."""
import math

import pytest
import torch

import bf16_attention_ref as ref

LOG2E = math.log2(math.e)


def emulate(q, k, v, d_o, scale, key_mask=None, causal_mask=None, mutation=None):
    """{"o", "dq", "dk", "dv"} as the kernels round them, computed in f32 on the CPU; `mutation` plants one bug."""
    f32, bf = torch.float32, ref.bf16_round
    q, k, v, d_o = (t.to(f32) for t in (q, k, v, d_o))
    B, H, I, _ = q.shape
    J = k.shape[2]
    if mutation == "ignore_key_mask_b1":
        key_mask = key_mask.clone()
        key_mask[1] = True
    filled = ref._masked(B, I, J, key_mask, causal_mask).expand(B, H, I, J)
    sc = torch.tensor(scale, dtype=f32)
    c2 = sc * torch.tensor(LOG2E, dtype=f32)
    fill_raw = torch.tensor(-1.0e9, dtype=f32) / sc
    s = torch.where(filled, fill_raw, q @ k.transpose(-1, -2))
    mc = s.amax(-1, keepdim=True) * c2
    pt = torch.exp2(s * c2 - mc)                       # unnormalised weights, f32
    if mutation and mutation.startswith("drop_key"):
        pt[..., int(mutation.split(":")[1])] = 0.0
    l = pt.sum(-1, keepdim=True)
    o = bf((bf(pt) @ v) * (1.0 / l))
    if mutation == "tail_unwritten":
        o[:, :, 32 * ((I - 1) // 32):] = 0.0
    delta = (d_o * o).sum(-1, keepdim=True)            # from the bf16 O
    if mutation == "delta_wrong_row":
        delta = torch.roll(delta, -1, dims=2)
    p = pt * (1.0 / l)
    ds = torch.where(filled, torch.zeros((), dtype=f32), p * (d_o @ v.transpose(-1, -2) - delta))
    dsb = bf(ds)
    dv = bf(bf(p).transpose(-1, -2) @ d_o)
    dk = bf((dsb.transpose(-1, -2) @ q) * sc)
    dq = torch.zeros_like(q)
    for kb in range((J + 255) // 256):
        if mutation == "dq_drop_block" and kb == 1:
            continue
        dq = dq + (dsb[..., 256 * kb:256 * (kb + 1)] @ k[:, :, 256 * kb:256 * (kb + 1)]) * sc
    out = {"o": o, "dq": bf(dq), "dk": dk, "dv": dv}
    if mutation == "swap_heads":
        out = {n: t[:, [1, 0] + list(range(2, H))] for n, t in out.items()}
    return out


def _case(family, mask, B, H, I, J, scale, seed):
    q, k, v, d_o = ref.make_inputs(family, B, H, I, J, scale, seed)
    km, cm = ref.make_masks(mask, B, I, J, seed)
    return (q, k, v, d_o, scale, km, cm), ref.reference(q, k, v, d_o, scale, km, cm)


TIGHT_CASES = [(fam, mask, sc) for fam in ref.FAMILIES for mask, sc in (("none", 0.125), ("both", 0.125))] + [
    ("peaked", "causal", 1.0), ("diffuse", "key", 0.05), ("needles", "dead_rows", 1.0), ("large", "dead_batch", 0.05),
    ("climb", "triu", 1.0), ("needles", "none", 0.05)]


@pytest.mark.parametrize("family,mask,scale", TIGHT_CASES, ids=lambda x: str(x))
def test_bound_not_too_tight(family, mask, scale):
    B, H, I, J = 2, 3, 129, 300
    args, R = _case(family, mask, B, H, I, J, scale, 11)
    for n, (nbad, worst) in ref.ratios(emulate(*args), R).items():
        assert worst < 0.5, f"{family}/{mask}/{scale} {n}: the emulated kernel reaches {worst:.3f} of the bound"


def test_bound_not_too_tight_j1_masked():
    args, R = _case("diffuse", "j1_masked", 2, 2, 33, 1, 0.125, 5)
    for n, (nbad, worst) in ref.ratios(emulate(*args), R).items():
        assert worst < 0.5, (n, worst)
    assert torch.equal(R["dq"], torch.zeros_like(R["dq"])) and torch.equal(R["dk"], torch.zeros_like(R["dk"]))


def test_needles_are_needles():
    """The generator's promise: o is the needle's v row and dv of a needle key collects exactly the dO rows that point
    at it (within a fraction of the bound), at every scale."""
    B, H, I, J = 2, 3, 40, 300
    for scale in (0.125, 1.0, 0.05):
        q, k, v, d_o = ref.make_inputs("needles", B, H, I, J, scale, 3)
        R = ref.reference(q, k, v, d_o, scale)
        nd = ref.needle_of(B, H, I, J)
        vn = torch.gather(v.double(), 2, nd.unsqueeze(-1).expand(B, H, I, ref.D))
        assert float(((R["o"] - vn).abs() / R["bound_o"]).max()) < 0.05
        dvn = torch.zeros_like(R["dv"]).scatter_add_(2, nd.unsqueeze(-1).expand(B, H, I, ref.D), d_o.double())
        assert float(((R["dv"] - dvn).abs() / R["bound_dv"]).max()) < 0.05
        assert len(set(nd[0, 0].tolist())) == len(ref.needle_positions(J))


# mutation -> the input families it must be flagged on: every one, except a missing dQ block on needle inputs (there the
# softmax is one-hot and dS, so dQ, is nothing but rounding noise)
MUTATIONS = {
    "drop_key:299": ref.FAMILIES,                 # the last key
    "drop_key:64": ref.FAMILIES,                  # the first key of the second 64-key tile
    "tail_unwritten": ref.FAMILIES,               # queries 128.. (I = 129)
    "swap_heads": ref.FAMILIES,
    "dq_drop_block": ("diffuse", "peaked", "large", "climb"),
    "delta_wrong_row": ref.FAMILIES,
    "ignore_key_mask_b1": ref.FAMILIES,
}


@pytest.mark.parametrize("mutation,family", [(m, f) for m, fams in MUTATIONS.items() for f in fams])
def test_bound_flags_wrong_results(mutation, family):
    mask = "key" if mutation == "ignore_key_mask_b1" else "none"
    args, R = _case(family, mask, 2, 3, 129, 300, 0.125, 11)
    good = ref.ratios(emulate(*args), R)
    assert all(nbad == 0 for nbad, _ in good.values()), good
    bad = ref.ratios(emulate(*args, mutation=mutation), R)
    assert any(nbad > 0 for nbad, _ in bad.values()), f"{mutation} on {family} inputs passes the bound: {bad}"
