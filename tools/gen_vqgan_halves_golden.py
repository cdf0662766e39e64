"""Write tests/golden/vqgan_small_halves.npz: the two halves of the conv VQGAN around the codebook lookup, computed by the
REFERENCE's own models/vqgan.py on the CPU in fp64.

    AMK_REFERENCE=<reference checkout> python tools/gen_vqgan_halves_golden.py

VQGAN(32, 512) with the weights of tests/vqgan_ref.py's recipe and the seed of tests/golden/vqgan_small.json; the inputs and
what is stored are those of tests/vqgan_halves_ref.py: pre_quant(encoder(imgs)) and decoder(post_quant(zq)), each against a
seeded cotangent, with the input gradient and the gradients of every gn.weight / gn.bias of that half.  The whole model cannot
be pinned under bf16 (the smallest top-2 margin of the lookup, 5e-4, is far below bf16 noise); these halves can.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vqgan_halves_ref  # noqa: E402
import vqgan_ref  # noqa: E402
from tools.gen_agent_golden_dh import save  # noqa: E402
from tools.gen_vqgan_golden import OUT, load_reference_vqgan  # noqa: E402


def main():
    ref = load_reference_vqgan()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with open(os.path.join(OUT, "vqgan_small.json")) as f:
        seed = json.load(f)["seed"]
    torch.manual_seed(0)
    model = ref.VQGAN(vqgan_ref.DIM, vqgan_ref.CODES)
    model.load_state_dict(vqgan_ref.recipe_state_dict(model, seed), strict=True)
    model = model.to(torch.float64)
    inp = {k: v.to(torch.float64) for k, v in vqgan_halves_ref.inputs(seed).items()}
    res = vqgan_halves_ref.run_halves(model, inp)
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
    size = save("vqgan_small_halves", {k: v.numpy() for k, v in res.items()})
    n_gn = sum(1 for k in res if ":grad:" in k)
    print(f"wrote vqgan_small_halves.npz ({size} bytes), seed {seed}: {len(res)} tensors, {n_gn} gn gradients; "
          f"max |enc out| {float(res['enc:out'].abs().max()):.3f}, max |dec out| {float(res['dec:out'].abs().max()):.3f}")


if __name__ == "__main__":
    main()
