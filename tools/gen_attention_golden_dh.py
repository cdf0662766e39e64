"""Write tests/golden/softmax_attention_d{96,192,256}.npz: SoftmaxAttention at head dims 96, 192 and 256, computed by
the REFERENCE's own models/softmax_attention.py on the CPU.

    AMK_REFERENCE=<reference checkout> python tools/gen_attention_golden_dh.py

Writes only these three files (golden_meta.json and the other fixtures are left as they are).  The reference module is
loaded by path through a namespace stub for its ``models`` package, as oracle/gen_golden.py does; the weights come from
oracle.fixture_recipe, so a rerun on the same torch build reproduces every file bit for bit.

Each file: the module's state (w:*), x, context, cotangent, the masks, and for three variants -- self-attention,
cross-attention with a key-padding mask, self-attention under a causal mask -- the output and the input gradients;
the parameter gradients of the two masked variants.  Model width 32 with 2 heads keeps each file under 1 MB.
"""
import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.fixture_recipe import randomize_, seeded  # noqa: E402
from oracle.gen_golden import REF  # noqa: E402  (the reference checkout; AMK_REFERENCE overrides)

OUT = os.path.join(ROOT, "tests", "golden")

# (head dim, parameter seed, x seed, context seed, cotangent seed)
CASES = [(96, 61, 731, 732, 733), (192, 62, 741, 742, 743), (256, 63, 751, 752, 753)]
DIM, H, B, T, J = 32, 2, 2, 20, 27
VARIANTS = ("self", "cross_ctxmask", "self_causal")
PARAM_GRADS = ("cross_ctxmask", "self_causal")


def load_reference_softmax():
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg
    return importlib.import_module("models.softmax_attention")


def save(name, arrays):
    """np.savez_compressed with a fixed member timestamp, so that reruns are byte-identical."""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    return os.path.getsize(path)


def gen(SA, d, pseed, xseed, cseed, gseed):
    torch.manual_seed(0)
    m = SA(DIM, H, d)
    randomize_(m, pseed)
    x = seeded((B, T, DIM), xseed).requires_grad_(True)
    ctx = seeded((B, J, DIM), cseed).requires_grad_(True)
    cot = seeded((B, T, DIM), gseed)
    causal = torch.ones(T, T).triu(1).bool()
    ctxmask = torch.ones(B, J, dtype=torch.bool)
    ctxmask[0, -7:] = False
    ctxmask[1, :4] = False
    kw = {"self": dict(), "cross_ctxmask": dict(context=ctx, context_mask=ctxmask), "self_causal": dict(causal_mask=causal)}
    names = [n for n, _ in sorted(m.named_parameters())]
    params = [p for _, p in sorted(m.named_parameters())]
    arrays = {"w:" + k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    arrays.update(x=x.detach().numpy(), context=ctx.detach().numpy(), cot=cot.numpy(), causal=causal.numpy(),
                  ctxmask=ctxmask.numpy(), dims=np.array([DIM, H, d]))
    for v in VARIANTS:
        out = m(x, **kw[v])
        wrt = [x] + ([ctx] if "context" in kw[v] else []) + params
        gs = torch.autograd.grad((out * cot).sum(), wrt)
        arrays[f"{v}:out"] = out.detach().numpy()
        arrays[f"{v}:gx"] = gs[0].numpy()
        off = 1
        if "context" in kw[v]:
            arrays[f"{v}:gctx"] = gs[1].numpy()
            off = 2
        if v in PARAM_GRADS:
            for n, g in zip(names, gs[off:]):
                arrays[f"{v}:g:{n}"] = g.numpy()
    return arrays


def main():
    SA = load_reference_softmax().SoftmaxAttention
    torch.set_num_threads(1)   # a fixed reduction order for the reference's CPU kernels
    for d, pseed, xseed, cseed, gseed in CASES:
        n = save(f"softmax_attention_d{d}", gen(SA, d, pseed, xseed, cseed, gseed))
        print(f"softmax_attention_d{d}.npz: {n} bytes")


if __name__ == "__main__":
    main()
