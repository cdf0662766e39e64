"""The masked-token sampling step (csrc/sample.hip) alone, at the Muse decode shape: B x 1024 rows of V = 8192 logits.

    python tools/kbench_sample.py [--batch 8] [--iters 50]

Four forms: with and without classifier-free guidance, with explicit Gumbel noise and with the in-kernel Philox
stream.  AMK_LIB=<libamk.so> selects the library, so two builds are compared by alternating runs of this tool.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
sys.path.insert(0, ROOT)
from bench import time_launches  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    from amk import lib, ops

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, T, V = a.batch, 1024, 8192
    logits = 2.0 * torch.randn(B, T, V, device=dev)
    null = 2.0 * torch.randn(B, T, V, device=dev)
    g = -torch.empty(B, T, V, device=dev).exponential_().log()
    ids = torch.zeros(B, T, dtype=torch.int64, device=dev)
    print(f"library {lib.LIB_PATH}, rows {B * T}, V {V}")
    for name, kw in (("guided, philox", dict(null_logits=null, seed=1)), ("guided, explicit", dict(null_logits=null, gumbel=g)),
                     ("plain, philox", dict(seed=1)), ("plain, explicit", dict(gumbel=g))):
        t = time_launches(lambda: ops.sample_step(logits, ids, tau=0.5, p=0.9, **kw), a.iters)
        print(f"{name:18s} {t * 1e3:8.4f} ms")


if __name__ == "__main__":
    main()
