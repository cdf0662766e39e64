"""bf16-MFMA attention core (csrc/attn_bf16.hip; head dims 32 / 128: csrc/attn_bf16_hd.hip) at the ViT-VQGAN layer
shape: forward and backward launch times, algorithmic TFLOP/s against the dense bf16 MFMA peak (2500 TFLOP/s), next to
the exact-f32 kernels.
    python tools/kbench_attn_bf16.py [--batch 32] [--iters 20] [--head-dim 64] [--heads 8]
    python tools/kbench_attn_bf16.py --compare [--rounds 5] --head-dim 128 --heads 4
--compare: two arms on the same bf16 inputs, alternating in one process for --rounds rounds -- "bf16": the head dim in
ops.ATTENTION_BF16_DIMS (the bf16-MFMA kernels), both under autocast; "before": the head dim not in the set (q, kv and dO upcast, the exact-f32
kernels, an f32 o) -- forward and forward + backward per round, the median and the spread (max - min over the rounds)
of each arm, and the peak memory above the inputs of one forward + backward."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402

from bench import time_launches  # noqa: E402

BF16_PEAK = 2500.0

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-f32", action="store_true", help="skip the exact-f32 kernels' line")
    ap.add_argument("--head-dim", type=int, default=64)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--compare", action="store_true", help="alternate the bf16 kernels and the path without them")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from amk import ops

    dev = torch.device("cuda:0")
    B, H, T, D = a.batch, a.heads, 1024, a.head_dim
    ops.ATTENTION_BF16_DIMS = frozenset(ops.ATTENTION_BF16_DIMS | {D})
    g = torch.Generator().manual_seed(0)
    q2 = torch.randn(B, T, H * D, generator=g).to(dev).bfloat16().requires_grad_(True)
    kv2 = torch.randn(B, T, 2 * H * D, generator=g).to(dev).bfloat16().requires_grad_(True)
    cot = torch.randn(B, T, H * D, generator=g).to(dev).bfloat16()
    core = 4.0 * B * H * T * T * D
    if a.compare:
        import statistics

        arms = {"bf16": frozenset(ops.ATTENTION_BF16_DIMS), "before": frozenset(ops.ATTENTION_BF16_DIMS - {D})}
        def fwd():   # under autocast, as a model calls it: there the path before upcasts its bf16 inputs
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return ops.attention_fused_kv(q2, kv2, H, D, D ** -0.5)

        fwd_bwd = lambda: torch.autograd.grad(fwd(), [q2, kv2], cot)
        times = {arm: {"f": [], "fb": []} for arm in arms}
        peak = {}
        for arm, dims in arms.items():   # one untimed pass of each arm first, with its peak memory above the inputs
            ops.ATTENTION_BF16_DIMS = dims
            fwd_bwd()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            g = fwd_bwd()
            torch.cuda.synchronize()
            peak[arm] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            del g
        for r in range(a.rounds):
            for arm, dims in arms.items():
                ops.ATTENTION_BF16_DIMS = dims
                times[arm]["f"].append(time_launches(fwd, a.iters))
                times[arm]["fb"].append(time_launches(fwd_bwd, a.iters))
                print(f"round {r} {arm:6s} h{H} d{D}: forward {times[arm]['f'][-1]*1e6:8.1f} us, forward + backward {times[arm]['fb'][-1]*1e6:8.1f} us")
        med = {arm: {k: statistics.median(v) for k, v in t.items()} for arm, t in times.items()}
        spr = {arm: {k: max(v) - min(v) for k, v in t.items()} for arm, t in times.items()}
        for arm in arms:
            print(f"{arm:6s} B{B} h{H} T{T} d{D}: forward median {med[arm]['f']*1e6:.1f} us (spread {spr[arm]['f']*1e6:.1f}), "
                  f"forward + backward median {med[arm]['fb']*1e6:.1f} us (spread {spr[arm]['fb']*1e6:.1f}), "
                  f"peak memory above the inputs {peak[arm]:.1f} MiB")
        tb = med["bf16"]["fb"] - med["bf16"]["f"]
        print(f"bf16 kernels h{H} d{D}: forward {core/med['bf16']['f']/1e12:.1f} TFLOP/s ({core/med['bf16']['f']/1e12/BF16_PEAK:.3f} of bf16 peak), "
              f"backward {2.5*core/tb/1e12:.1f} TFLOP/s on its five products ({2.5*core/tb/1e12/BF16_PEAK:.3f}); "
              f"against the path before: forward {med['before']['f']/med['bf16']['f']:.2f}x, forward + backward {med['before']['fb']/med['bf16']['fb']:.2f}x")
        sys.exit(0)
    o = ops.attention_fused_kv(q2, kv2, H, D, D ** -0.5)
    t_f = time_launches(lambda: ops.attention_fused_kv(q2, kv2, H, D, D ** -0.5), a.iters)
    t_fb = time_launches(lambda: torch.autograd.grad(ops.attention_fused_kv(q2, kv2, H, D, D ** -0.5), [q2, kv2], cot), a.iters)
    t_b = t_fb - t_f
    print(f"bf16 attention B{B} h{H} T{T} d{D}: forward {t_f*1e6:.1f} us = {core/t_f/1e12:.1f} TFLOP/s ({core/t_f/1e12/BF16_PEAK:.3f} of bf16 peak); "
          f"backward (delta + fused + dq reduce) {t_b*1e6:.1f} us = {2.5*core/t_b/1e12:.1f} TFLOP/s on its five products "
          f"({2.5*core/t_b/1e12/BF16_PEAK:.3f})")
    if a.no_f32:
        sys.exit(0)
    qf, kvf = q2.detach().float().requires_grad_(True), kv2.detach().float().requires_grad_(True)
    t_f32 = time_launches(lambda: ops.attention_fused_kv(qf, kvf, H, D, D ** -0.5), a.iters)
    t_fb32 = time_launches(lambda: torch.autograd.grad(ops.attention_fused_kv(qf, kvf, H, D, D ** -0.5), [qf, kvf], cot.float()), a.iters)
    print(f"exact-f32 kernels, same shape: forward {t_f32*1e6:.1f} us, backward {(t_fb32-t_f32)*1e6:.1f} us")
