"""AgentAttention module timings (B 2 = the BASELINE.md row, B 64 = the chip-filling case).

    python tools/kbench_agent.py [--iters 20] [--dim-head 32|64|128]

The core's forward and backward are also given as a fraction of the 8 TB/s HBM peak, with bench.py's agent_block
byte count (16 * B*h*T*d forward, 28 * B*h*T*d backward: scales with the head dim).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
sys.path.insert(0, ROOT)
from tools.kbench_moe import time_launches  # noqa: E402

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dim-head", type=int, default=64, choices=[32, 64, 128])
    a = ap.parse_args()
    d = a.dim_head
    from amk import ops
    from amk.models import AgentAttention

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ag = AgentAttention(384, 6, d).to(dev)
    for B in (2, 8, 64):
        x = torch.randn(B, 1024, 384, device=dev, requires_grad=True)
        cot = torch.randn(B, 1024, 384, device=dev)
        qkv = ag.qkv(x).detach().requires_grad_(True)
        cw, cb = ag.dwc[1].weight, ag.dwc[1].bias
        core = lambda: ops.agent_attention(qkv, cw, cb, 6, d, ag.pool_size, ag.scale)
        co = torch.randn(B, 1024, 6 * d, device=dev)

        def core_fb():
            core().backward(co)

        def fb():
            ag(x).backward(cot)
        t_c = time_launches(core, a.iters)
        t_cfb = time_launches(core_fb, a.iters)
        t_f = time_launches(lambda: ag(x), a.iters)
        t_fb = time_launches(fb, a.iters)
        unit = float(B * 6 * 1024 * d)
        byt_f, byt_b, t_cb = 16.0 * unit, 28.0 * unit, t_cfb - t_c   # q, k, v read + o written; q, k, v, dO read + dq, dk, dv written
        print(f"d {d:3d} B {B:3d}: core fwd {t_c*1e3:7.3f} ms ({byt_f/t_c/1e9:7.1f} GB/s algorithmic, {byt_f/t_c/1e9/HBM_PEAK_GBS:.3f} of HBM peak)"
              f"  core bwd {t_cb*1e3:7.3f} ms ({byt_b/t_cb/1e9/HBM_PEAK_GBS:.3f} of HBM peak)  core fwd+bwd {t_cfb*1e3:7.3f} ms"
              f" | module fwd {t_f*1e3:7.3f} ms  fwd+bwd {t_fb*1e3:7.3f} ms")


if __name__ == "__main__":
    main()
