"""Write tests/golden/vqgan_small.npz and vqgan_small.json: the conv VQGAN, computed by the REFERENCE's own models/vqgan.py
on the CPU in fp64, with the f32 run's deviation from it recorded.

    AMK_REFERENCE=<reference checkout> python tools/gen_vqgan_golden.py

VQGAN(32, 512) with the weights of tests/vqgan_ref.py's recipe; forward + backward of (out * cot).sum() + loss on the seeded
(2, 3, 64, 64) input.  The first seed whose smallest top-2 distance margin of the codebook lookup is at least
vqgan_ref.MIN_MARGIN is taken, so that no index depends on f32 rounding.  Stored: the fp64 out, loss, indices, input gradient
and the gradients of every gn.weight / gn.bias, of pre_quant, post_quant and the codebook; in the .json the seed, the margin
and max |f32 - fp64| / max |fp64| of every stored tensor.
"""
import importlib
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vqgan_ref  # noqa: E402
from oracle.gen_golden import REF  # noqa: E402  (the reference checkout; AMK_REFERENCE overrides)
from tools.gen_agent_golden_dh import save  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def load_reference_vqgan():
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg
    return importlib.import_module("models.vqgan")


def run(ref, seed, dtype):
    """{name: tensor} of one forward + backward in `dtype`, and the smallest top-2 margin of the lookup."""
    torch.manual_seed(0)
    model = ref.VQGAN(vqgan_ref.DIM, vqgan_ref.CODES)
    model.load_state_dict(vqgan_ref.recipe_state_dict(model, seed), strict=True)
    model = model.to(dtype)
    imgs, cot = vqgan_ref.inputs(seed)
    imgs = imgs.to(dtype).requires_grad_(True)
    out, loss = model(imgs)
    ((out * cot.to(dtype)).sum() + loss).backward()
    with torch.no_grad():
        z = model.pre_quant(model.encoder(imgs)).permute(0, 2, 3, 1).reshape(-1, vqgan_ref.DIM)
        zn = torch.nn.functional.normalize(z, dim=-1)
        en = torch.nn.functional.normalize(model.codebook.embedding.weight, dim=-1)
        d = (zn * zn).sum(1, keepdim=True) + (en * en).sum(1) - 2 * zn @ en.t()
        two = d.topk(2, dim=1, largest=False).values
        margin = float((two[:, 1] - two[:, 0]).min())
        idx = d.argmin(1)
    res = {"out": out.detach(), "loss": loss.detach(), "indices": idx, "grad_imgs": imgs.grad}
    params = dict(model.named_parameters())
    for n in vqgan_ref.stored_grad_names(model):
        res["grad:" + n] = params[n].grad
    assert all(p.grad is None for n, p in params.items() if ".proj_out." in n)
    return res, margin


def main():
    ref = load_reference_vqgan()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    for seed in range(1, 20):
        r64, margin = run(ref, seed, torch.float64)
        print(f"seed {seed}: smallest top-2 margin {margin:.3e}", flush=True)
        if margin >= vqgan_ref.MIN_MARGIN:
            break
    else:
        raise SystemExit("no seed reaches the margin")
    r32, _ = run(ref, seed, torch.float32)
    assert torch.equal(r32["indices"], r64["indices"]), "the f32 indices differ from the fp64 ones"
    dev = {}
    for k, v in r64.items():
        if k == "indices":
            continue
        scale = float(v.abs().max())
        dev[k] = float((r32[k].double() - v).abs().max()) / scale if scale > 0 else float((r32[k].double() - v).abs().max())
    size = save("vqgan_small", {k: v.numpy() for k, v in r64.items()})
    gn = max(v for k, v in dev.items() if ".gn." in k)
    meta = {"seed": seed, "min_top2_margin": margin, "model": f"VQGAN({vqgan_ref.DIM}, {vqgan_ref.CODES})",
            "input": list(vqgan_ref.IMG_SHAPE), "f32_vs_fp64_deviation": dev, "worst_gn_gradient_deviation": gn}
    with open(os.path.join(OUT, "vqgan_small.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote vqgan_small.npz ({size} bytes), seed {seed}; deviations: out {dev['out']:.2e}, "
          f"grad_imgs {dev['grad_imgs']:.2e}, worst gn gradient {gn:.2e}")


if __name__ == "__main__":
    main()
