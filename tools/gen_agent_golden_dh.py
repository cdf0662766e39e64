"""Write tests/golden/agent_d32.npz and tests/golden/agent_d128.npz: AgentAttention at head dims 32 and 128, computed
by the REFERENCE's own models/agent_attention.py on the CPU (same layout as oracle/gen_golden.py's agent_small).

    AMK_REFERENCE=<reference checkout> python tools/gen_agent_golden_dh.py

Writes only these two files (golden_meta.json and the other fixtures are left as they are).  The reference module is
loaded by path through a namespace stub for its ``models`` package, as oracle/gen_golden.py does; the weights come from
oracle.fixture_recipe, so a rerun on the same torch build reproduces both files bit for bit.
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

# (head dim, parameter seed, x seed, cotangent seed); dim 64, h 2, agent_num 4 (pool 2 == h), B 2, T 20
CASES = [(32, 53, 711, 712), (128, 54, 721, 722)]
DIM, H, AGENT_NUM, B, T = 64, 2, 4, 2, 20


def load_reference_agent():
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg
    return importlib.import_module("models.agent_attention")


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


def gen(AA, d, pseed, xseed, cseed):
    torch.manual_seed(0)
    m = AA(DIM, H, d, agent_num=AGENT_NUM)
    randomize_(m, pseed)
    with torch.no_grad():
        m.bias1.fill_(0.3)
        m.bias2.fill_(-0.2)
    x = seeded((B, T, DIM), xseed).requires_grad_(True)
    cot = seeded((B, T, DIM), cseed)
    out = m(x)
    names = [n for n, _ in sorted(m.named_parameters())]
    params = [p for _, p in sorted(m.named_parameters())]
    gs = torch.autograd.grad((out * cot).sum(), [x] + params, allow_unused=True)
    arrays = {"w:" + k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    arrays.update(x=x.detach().numpy(), cot=cot.numpy(), out=out.detach().numpy(), gx=gs[0].numpy(),
                  dims=np.array([DIM, H, d, AGENT_NUM]))
    for n, g in zip(names, gs[1:]):
        if g is not None:
            arrays["g:" + n] = g.numpy()
    return arrays


def main():
    AA = load_reference_agent().AgentAttention
    torch.set_num_threads(1)   # a fixed reduction order for the reference's CPU kernels
    for d, pseed, xseed, cseed in CASES:
        n = save(f"agent_d{d}", gen(AA, d, pseed, xseed, cseed))
        print(f"agent_d{d}.npz: {n} bytes")


if __name__ == "__main__":
    main()
