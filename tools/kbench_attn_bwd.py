"""Attention core at the ViT-VQGAN layer shape: forward with / without kept scores, fused backward with
128 / 256 keys per workgroup, recomputed / kept scores, and the kept-scores backward with its dV / dK products on
split-bf16 MFMA (AMK_ATTN_BWD_X6) back to back with the f32 one, arms alternating, dq by atomics and reproducible.
    python tools/kbench_attn_bwd.py [--batch 32] [--iters 30] [--rounds 5]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))

import torch  # noqa: E402

from bench import time_launches  # noqa: E402

PEAK = 157.3

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--H", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the f32 / split-bf16 kept-scores backward")
    a = ap.parse_args()
    from amk import lib, ops

    L_ws = lambda B_, H_, I_, J_: lib.load().amk_attn_bwd_ws_floats(B_, H_, I_, J_, 8 | 64 | 32)

    dev = torch.device("cuda:0")
    B, H, T, D = a.batch, a.H, a.T, 64
    g = torch.Generator().manual_seed(99)
    mk = lambda: torch.randn(B, T, H, D, generator=g).to(dev).permute(0, 2, 1, 3)
    q, k, v, d_o = mk(), mk(), mk(), mk()
    scale = D ** -0.5
    core = 4.0 * B * H * T * T * D
    rows = []
    t = time_launches(lambda: ops._attn_forward(q, k, v, None, None, scale), a.iters)
    rows.append(("attn_fwd", t, core))
    t = time_launches(lambda: ops._attn_forward(q, k, v, None, None, scale, keep_scores=True), a.iters)
    rows.append(("attn_fwd_keep", t, core))
    q, k, v, o, stats, scores = ops._attn_forward(q, k, v, None, None, scale, keep_scores=True)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    delta = torch.empty(B, H, T, device=dev)
    ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, None, None, scale, stages=1, delta=delta)
    for keys, bit in ((128, 16), (256, 32)):
        for kept in (False, True):
            fn = lambda: ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, None, None, scale, stages=8 | bit,
                                            delta=delta, scores=scores if kept else None)
            t = time_launches(fn, a.iters)
            rows.append((f"attn_bwd_fused keys={keys} {'kept' if kept else 'recompute'}", t, 2 * core))
    big = torch.empty(L_ws(B, H, T, T), device=dev)
    for kept in (False, True):
        fn = lambda: ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, None, None, scale, stages=8 | 64 | 32,
                                        delta=big, scores=scores if kept else None)
        ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, None, None, scale, stages=1, delta=big)
        t = time_launches(fn, a.iters)
        rows.append((f"attn_bwd_fused keys=256 {'kept' if kept else 'recompute'} reproducible dq", t, 2 * core))
    # f32 against split-bf16 dV / dK, kept scores, 256 keys: the arms alternate so that clock and temperature drift hits both
    arms = [(f"attn_bwd_fused keys=256 kept {'x6 dV/dK' if x6 else 'f32'}{' reproducible dq' if repro else ''}", 8 | 32 | repro | x6)
            for repro in (0, 64) for x6 in (0, 128)]
    times = {name: [] for name, _ in arms}
    for _ in range(a.rounds):
        for name, st in arms:
            fn = lambda: ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, None, None, scale, stages=st, delta=big, scores=scores)
            times[name].append(time_launches(fn, a.iters, warm=max(3, a.iters)))
    for name, t, fl in rows:
        print(f"{name:44s} {t * 1e3:8.4f} ms  {fl / t / 1e12:7.2f} TFLOP/s  {fl / t / 1e12 / PEAK:.3f} of f32 MFMA peak", flush=True)
    for name, _ in arms:
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        print(f"{name:52s} median {med * 1e3:7.4f} ms  min {ts[0] * 1e3:7.4f}  max {ts[-1] * 1e3:7.4f}  ({a.rounds} alternating rounds)  "
              f"{2 * core / med / 1e12:7.2f} algorithmic TFLOP/s", flush=True)
