"""CPU checks of the bf16 attention checker at head dims 32 and 128 (tests/bf16_attention_hd_ref.py), no GPU needed.

Not too tight: the emulation of the rounding points csrc/attn_bf16.hip documents (tests/test_bf16_attention_bounds.py),
with dQ summed as per-KEY_BLOCK[D]-key f32 partials in order, stays within half of every element's bound over the same
case list.  Sensitive enough: a dropped dQ block at KEY_BLOCK[D], the first key of the second tile, an unwritten 32-query
tail, swapped heads, delta from the wrong row and an ignored key mask are flagged.  Plus the two pieces of host code the
GPU tests rely on: ops.ATTENTION_BF16_DIMS parsing and KEY_BLOCK against the library's workspace size."""
import math

import pytest
import torch

import bf16_attention_hd_ref as ref
from test_bf16_attention_bounds import MUTATIONS, TIGHT_CASES

LOG2E = math.log2(math.e)
SHAPE = (2, 3, 129, 300)


def emulate(q, k, v, d_o, scale, key_mask=None, causal_mask=None, mutation=None):
    """{"o", "dq", "dk", "dv"} as the kernels round them, computed in f32 on the CPU, the head dim taken from q;
    `mutation` plants one bug."""
    f32, bf = torch.float32, ref.bf16_round
    q, k, v, d_o = (t.to(f32) for t in (q, k, v, d_o))
    B, H, I, D = q.shape
    J = k.shape[2]
    KB = ref.KEY_BLOCK[D]
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
    for kb in range((J + KB - 1) // KB):
        if mutation == "dq_drop_block" and kb == 1:
            continue
        dq = dq + (dsb[..., KB * kb:KB * (kb + 1)] @ k[:, :, KB * kb:KB * (kb + 1)]) * sc
    out = {"o": o, "dq": bf(dq), "dk": dk, "dv": dv}
    if mutation == "swap_heads":
        out = {n: t[:, [1, 0] + list(range(2, H))] for n, t in out.items()}
    return out


def _case(family, mask, B, H, I, J, D, scale, seed):
    q, k, v, d_o = ref.make_inputs(family, B, H, I, J, D, scale, seed)
    km, cm = ref.make_masks(mask, B, I, J, seed)
    return (q, k, v, d_o, scale, km, cm), ref.reference(q, k, v, d_o, scale, km, cm)


@pytest.mark.parametrize("D", ref.HEAD_DIMS)
@pytest.mark.parametrize("family,mask,scale", TIGHT_CASES, ids=lambda x: str(x))
def test_bound_not_too_tight(family, mask, scale, D):
    args, R = _case(family, mask, *SHAPE, D, scale, 11)
    for n, (nbad, worst) in ref.ratios(emulate(*args), R).items():
        assert worst < 0.5, f"D {D} {family}/{mask}/{scale} {n}: the emulated kernel reaches {worst:.3f} of the bound"


@pytest.mark.parametrize("D", ref.HEAD_DIMS)
def test_bound_not_too_tight_j1_masked(D):
    args, R = _case("diffuse", "j1_masked", 2, 2, 33, 1, D, 0.125, 5)
    for n, (nbad, worst) in ref.ratios(emulate(*args), R).items():
        assert worst < 0.5, (n, worst)
    assert torch.equal(R["dq"], torch.zeros_like(R["dq"])) and torch.equal(R["dk"], torch.zeros_like(R["dk"]))


@pytest.mark.parametrize("D", ref.HEAD_DIMS)
@pytest.mark.parametrize("mutation,family", [(m, f) for m, fams in MUTATIONS.items() for f in fams])
def test_bound_flags_wrong_results(mutation, family, D):
    """The mutations of the D = 64 module; dq_drop_block drops keys KEY_BLOCK[D] .. 2 KEY_BLOCK[D] - 1 here."""
    mask = "key" if mutation == "ignore_key_mask_b1" else "none"
    args, R = _case(family, mask, *SHAPE, D, 0.125, 11)
    good = ref.ratios(emulate(*args), R)
    assert all(nbad == 0 for nbad, _ in good.values()), good
    bad = ref.ratios(emulate(*args, mutation=mutation), R)
    assert any(nbad > 0 for nbad, _ in bad.values()), f"D {D}: {mutation} on {family} inputs passes the bound: {bad}"


def test_attention_bf16_dims_parsing():
    """The default is {64}: with the variable unset every call takes the kernels it took before the switch existed."""
    from amk import ops

    assert ops._parse_bf16_dims("64") == {64}
    assert ops._parse_bf16_dims("32,64,128") == {32, 64, 128}
    assert ops._parse_bf16_dims(" 128 , 32 ") == {32, 128}
    for bad in ("", "96", "64,", "32;128", "64,256", "all"):
        with pytest.raises(ValueError, match="AMK_ATTENTION_BF16_DIMS"):
            ops._parse_bf16_dims(bad)


def test_attention_bf16_dims_default_and_refusal_at_import():
    """Read once from the environment when amk.ops is executed: unset -> {64}; a list -> that set; a bad value is a
    ValueError out of the import.  One fresh child process, which executes the module three times."""
    import os
    import subprocess
    import sys

    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "attention-models_amd")
    code = """
import importlib, os, sys
sys.path.insert(0, sys.argv[1])
from amk import ops
print(sorted(ops.ATTENTION_BF16_DIMS))
os.environ["AMK_ATTENTION_BF16_DIMS"] = "32,128"
print(sorted(importlib.reload(ops).ATTENTION_BF16_DIMS))
os.environ["AMK_ATTENTION_BF16_DIMS"] = "64,96"
try:
    importlib.reload(ops)
    print("imported")
except ValueError as e:
    print("ValueError", e)
"""
    env = {k: v for k, v in os.environ.items() if k != "AMK_ATTENTION_BF16_DIMS"}
    r = subprocess.run([sys.executable, "-c", code, pkg], env=env, capture_output=True, text=True)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines[:2] == ["[64]", "[32, 128]"], (r.stdout, r.stderr)
    assert lines[2].startswith("ValueError") and "AMK_ATTENTION_BF16_DIMS" in lines[2] and "96" in lines[2], r.stdout


@pytest.mark.parametrize("D", ref.HEAD_DIMS)
def test_key_block_is_the_library_s(D):
    """amk_attn_bf16_hd_bwd_ws_floats(1, 1, 1, J, D) = 4 row constants + nkblk partial rows of D floats (pure host
    code): nkblk steps up exactly at the multiples of KEY_BLOCK[D]."""
    from amk import lib

    L = lib.load()
    KB = ref.KEY_BLOCK[D]
    nkblk = lambda J: (L.amk_attn_bf16_hd_bwd_ws_floats(1, 1, 1, J, D) - 4) // D
    for J in (1, KB - 1, KB, KB + 1, 2 * KB, 2 * KB + 1, 1024):
        assert nkblk(J) == (J + KB - 1) // KB, (D, J, nkblk(J))
    assert L.amk_attn_bf16_hd_bwd_ws_floats(2, 3, 5, 300, D) == 4 * 2 * 3 * 5 + ((300 + KB - 1) // KB) * 2 * 3 * 5 * D
    for other in (64, 96, 0):
        assert L.amk_attn_bf16_hd_bwd_ws_floats(1, 1, 1, 100, other) == 0
