"""Seeded weights and inputs of the conv-VQGAN fixture tests/golden/vqgan_small.npz (tools/gen_vqgan_golden.py writes it
from the reference's models/vqgan.py; tests/test_vqgan_gpu.py runs amk.models.VQGAN against it).

oracle/fixture_recipe.py does not suit this model: it takes the last axis as the fan, which is 3 for a 3 x 3 convolution,
and does not know ``gn.weight`` as a norm's scale.  The recipe here: the parameters in sorted-name order, parameter
number i drawn from N(0, 1) by a generator seeded ``seed * 1000 + i`` (in f32, n below), then
    *.gn.weight                  1 + 0.1 n
    any bias                     0.1 n
    codebook.embedding.weight    n
    every other weight           n fan_in^-1/2, fan_in = the elements of one output slice (weight[0].numel())
The 68 M parameters of the model are never stored; both sides rebuild them from the seed.
"""
import torch

DIM, CODES = 32, 512            # VQGAN(32, 512)
IMG_SHAPE = (2, 3, 64, 64)
MIN_MARGIN = 5e-4               # the tool takes the first seed whose smallest top-2 distance margin reaches this


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def recipe_state_dict(model, seed):
    """{name: f32 tensor} for every parameter of `model`, by the recipe above."""
    out = {}
    for i, (name, p) in enumerate(sorted(model.named_parameters(), key=lambda kv: kv[0])):
        n = torch.randn(p.shape, generator=_gen(seed * 1000 + i), dtype=torch.float32)
        if name.endswith("gn.weight"):
            v = 1 + 0.1 * n
        elif name.endswith(".bias"):
            v = 0.1 * n
        elif name == "codebook.embedding.weight":
            v = n
        else:
            v = n * float(p[0].numel()) ** -0.5
        out[name] = v
    return out


def inputs(seed):
    """(imgs in [0, 1), cotangent of `out`), f32, IMG_SHAPE."""
    imgs = torch.rand(IMG_SHAPE, generator=_gen(seed * 1000 + 998), dtype=torch.float32)
    cot = torch.randn(IMG_SHAPE, generator=_gen(seed * 1000 + 999), dtype=torch.float32)
    return imgs, cot


def stored_grad_names(model):
    """The parameters whose gradients the fixture stores: every gn.weight / gn.bias, pre_quant, post_quant, the codebook."""
    return [n for n, _ in model.named_parameters()
            if n.endswith(("gn.weight", "gn.bias")) or n.startswith(("pre_quant.", "post_quant.", "codebook."))]
