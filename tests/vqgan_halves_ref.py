"""Seeded inputs of the two-halves fixture of the conv VQGAN, tests/golden/vqgan_small_halves.npz
(tools/gen_vqgan_halves_golden.py writes it from the reference's models/vqgan.py in fp64; tests/test_vqgan_bf16_gpu.py runs
amk.models.VQGAN under bf16 autocast against it).  The weights, the images and the seed are those of tests/vqgan_ref.py and
tests/golden/vqgan_small.json; neither half contains the codebook lookup.

    encoder half   e = pre_quant(encoder(imgs)),  (e * cot_e).sum().backward():  e, the gradient of imgs and of every
                   encoder gn.weight / gn.bias
    decoder half   out = decoder(post_quant(zq)),  (out * cot_out).sum().backward():  out, the gradient of zq and of every
                   decoder gn.weight / gn.bias
"""
import torch

import vqgan_ref

ZQ_SHAPE = (2, vqgan_ref.DIM, 4, 4)


def inputs(seed):
    """dict of f32 tensors: imgs (IMG_SHAPE), cot_e (ZQ_SHAPE), zq (ZQ_SHAPE), cot_out (IMG_SHAPE)."""
    imgs, cot_out = vqgan_ref.inputs(seed)
    n = lambda k: torch.randn(ZQ_SHAPE, generator=torch.Generator().manual_seed(seed * 1000 + k), dtype=torch.float32)  # noqa: E731
    return dict(imgs=imgs, cot_e=n(996), zq=n(997), cot_out=cot_out)


def gn_names(model, half):
    """The gn.weight / gn.bias parameters of `half` ("encoder" or "decoder"), by name."""
    return [n for n, _ in model.named_parameters() if n.startswith(half + ".") and n.endswith(("gn.weight", "gn.bias"))]


def run_halves(model, inp, autocast=None):
    """{name: tensor} of both halves on `model` (the reference's VQGAN or amk.models.VQGAN), inputs in the dtype and on the
    device of `inp`.  Keys: enc:out, enc:grad_imgs, enc:grad:<param>, dec:out, dec:grad_zq, dec:grad:<param>."""
    import contextlib

    ctx = (lambda: torch.autocast("cuda", dtype=autocast)) if autocast is not None else contextlib.nullcontext
    params = dict(model.named_parameters())
    res = {}
    for half, x_key, cot_key, gname in (("enc", "imgs", "cot_e", "grad_imgs"), ("dec", "zq", "cot_out", "grad_zq")):
        model.zero_grad(set_to_none=True)
        x = inp[x_key].detach().clone().requires_grad_(True)
        with ctx():
            y = model.pre_quant(model.encoder(x)) if half == "enc" else model.decoder(model.post_quant(x))
        (y.to(inp[cot_key].dtype) * inp[cot_key]).sum().backward()
        res[half + ":out"] = y.detach()
        res[half + ":" + gname] = x.grad
        for n in gn_names(model, "encoder" if half == "enc" else "decoder"):
            res[f"{half}:grad:{n}"] = params[n].grad.detach().clone()
    model.zero_grad(set_to_none=True)
    return res
