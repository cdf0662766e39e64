"""Write tests/golden/softmax_attention_bf16_d{32,128}.npz: SoftmaxAttention at head dims 32 and 128 under
torch.autocast("cpu", dtype=torch.bfloat16) -- the reference's shipped training precision (cfg/vitvqgan.yaml:73) -- and
in f32, both computed by the REFERENCE's own models/softmax_attention.py on the CPU.

    AMK_REFERENCE=<reference checkout> python tools/gen_attention_bf16_golden_dh.py

Writes only these two files (golden_meta.json and the other fixtures are left as they are).  The reference module is
loaded as tools/gen_attention_golden_dh.py loads it, the model is that tool's small one (width 32, 2 heads), and the
weights and inputs come from oracle.fixture_recipe, so a rerun on the same torch build reproduces both files bit for bit.

Each file: the module's state (w:*), x, context, cotangent, the masks, and for three variants -- self-attention,
cross-attention with a key-padding mask, self-attention under a causal mask -- the output and the input gradients, and
for the two masked variants the parameter gradients, under autocast (`<variant>:out`, `:gx`, `:gctx`, `:g:<param>`) and
in f32 (`:out_f32`, `:gx_f32`, `:gctx_f32`, `:g32:<param>`), and `<variant>:err` = (err_out, err_gx, err_gctx,
err_gparams): max |autocast - f32| / max |f32| of the reference against ITSELF, the tolerance the mode supports at this
head dim (err_gctx 0 without a context).  0.2 MB and 0.6 MB.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_attention_golden_dh import B, DIM, H, J, PARAM_GRADS, T, VARIANTS, load_reference_softmax, save  # noqa: E402
from oracle.fixture_recipe import randomize_, seeded  # noqa: E402

# (head dim, parameter seed, x seed, context seed, cotangent seed)
CASES = [(32, 64, 761, 762, 763), (128, 65, 771, 772, 773)]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def gen(SA, d, pseed, xseed, cseed, gseed):
    torch.manual_seed(0)
    m = SA(DIM, H, d)
    randomize_(m, pseed)
    x = seeded((B, T, DIM), xseed)
    ctx = seeded((B, J, DIM), cseed)
    cot = seeded((B, T, DIM), gseed)
    causal = torch.ones(T, T).triu(1).bool()
    ctxmask = torch.ones(B, J, dtype=torch.bool)
    ctxmask[0, -7:] = False
    ctxmask[1, :4] = False
    kw = {"self": dict(), "cross_ctxmask": dict(context=ctx, context_mask=ctxmask), "self_causal": dict(causal_mask=causal)}
    names = [n for n, _ in sorted(m.named_parameters())]
    params = [p for _, p in sorted(m.named_parameters())]
    arrays = {"w:" + k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    arrays.update(x=x.numpy(), context=ctx.numpy(), cot=cot.numpy(), causal=causal.numpy(), ctxmask=ctxmask.numpy(),
                  dims=np.array([DIM, H, d]))
    for v in VARIANTS:
        res = {}
        for mode in ("f32", "bf16"):
            xr = x.clone().requires_grad_(True)
            kw2 = dict(kw[v])
            wrt = [xr]
            if "context" in kw2:
                kw2["context"] = ctx.clone().requires_grad_(True)
                wrt.append(kw2["context"])
            if mode == "bf16":
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    out = m(xr, **kw2)
            else:
                out = m(xr, **kw2)
            gs = torch.autograd.grad((out.float() * cot).sum(), wrt + params)
            res[mode] = (out.detach().float(), [g.detach().float() for g in gs])
        (o32, g32), (o16, g16) = res["f32"], res["bf16"]
        arrays[f"{v}:out"], arrays[f"{v}:out_f32"] = o16.numpy(), o32.numpy()
        arrays[f"{v}:gx"], arrays[f"{v}:gx_f32"] = g16[0].numpy(), g32[0].numpy()
        off, err_gctx = 1, 0.0
        if "context" in kw[v]:
            arrays[f"{v}:gctx"], arrays[f"{v}:gctx_f32"] = g16[1].numpy(), g32[1].numpy()
            off, err_gctx = 2, rel(g16[1], g32[1])
        if v in PARAM_GRADS:
            for n, a, b in zip(names, g16[off:], g32[off:]):
                arrays[f"{v}:g:{n}"], arrays[f"{v}:g32:{n}"] = a.numpy(), b.numpy()
        arrays[f"{v}:err"] = np.array([rel(o16, o32), rel(g16[0], g32[0]), err_gctx,
                                       max(rel(a, b) for a, b in zip(g16[off:], g32[off:]))], dtype=np.float64)
    return arrays


def main():
    SA = load_reference_softmax().SoftmaxAttention
    torch.set_num_threads(1)   # a fixed reduction order for the reference's CPU kernels
    for d, pseed, xseed, cseed, gseed in CASES:
        arrays = gen(SA, d, pseed, xseed, cseed, gseed)
        n = save(f"softmax_attention_bf16_d{d}", arrays)
        print(f"softmax_attention_bf16_d{d}.npz: {n} bytes; reference autocast vs f32 (out, gx, gctx, gparams):",
              {v: [float(f"{e:.3g}") for e in arrays[f"{v}:err"]] for v in VARIANTS})


if __name__ == "__main__":
    main()
