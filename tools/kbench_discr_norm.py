"""BatchNorm2d + LeakyReLU of the PatchGAN discriminator at the benchmark's three BN-layer shapes (batch 32):
ATen (MIOpen batch norm, leaky_relu, composite double backward) against csrc/discr_norm.hip, interleaved round by
round in one process so both see the same warm chip.  Per call and per step (4 forwards, 5 first-order backwards,
1 double backward per layer), and the native kernels' rate against their algorithmic bytes (3 / 5 / 8 array passes)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from amk import ops  # noqa: E402
from amk.models.discriminator import input_grad_only  # noqa: E402

SHAPES = [(128, 64), (256, 32), (512, 31)]   # (C, H = W) of model.3 / .6 / .9 at 256 px
PASSES = {"fwd": 3, "bwd": 5, "dbl": 8}
PER_STEP = {"fwd": 4, "bwd": 5, "dbl": 1}
PEAK = 6.3e12   # bytes/s a device copy reaches


def make(C, H, B, dev, native):
    bn = nn.BatchNorm2d(C).to(dev)
    x = (0.5 + torch.randn(B, C, H, H, device=dev)).requires_grad_()
    gz = torch.randn_like(x).requires_grad_()
    ggx = torch.randn_like(x)

    def f(inp):
        if native:
            return ops.bn_leaky_relu(inp, bn, 0.2)
        return nn.functional.leaky_relu(bn(inp), 0.2, inplace=True)

    z = f(x)
    with input_grad_only():
        (gx,) = torch.autograd.grad(z, x, gz, create_graph=True)

    def fwd():
        with torch.no_grad():
            f(x)

    def bwd():
        torch.autograd.grad(z, x, gz.detach(), retain_graph=True)

    def dbl():
        torch.autograd.grad(gx, (x, bn.weight, gz), ggx, retain_graph=True)

    return {"fwd": fwd, "bwd": bwd, "dbl": dbl}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cases = {(C, H, nat): make(C, H, args.batch, dev, nat) for C, H in SHAPES for nat in (False, True)}
    res = {k: {op: [] for op in PASSES} for k in cases}
    for r in range(args.rounds + 1):
        for C, H in SHAPES:
            for op in PASSES:
                for nat in (False, True):
                    ms = timed(cases[(C, H, nat)][op], args.iters)
                    if r:   # round 0 warms up
                        res[(C, H, nat)][op].append(ms)
    step = {False: 0.0, True: 0.0}
    print(f"batch {args.batch}, median of {args.rounds} interleaved rounds x {args.iters} calls")
    print(f"{'layer':>16} {'op':>4} {'aten ms':>9} {'amk ms':>9} {'speedup':>8} {'amk GB/s':>9} {'of 6.3TB/s':>10}")
    for C, H in SHAPES:
        nbytes = args.batch * C * H * H * 4
        for op in PASSES:
            a = statistics.median(res[(C, H, False)][op])
            n = statistics.median(res[(C, H, True)][op])
            step[False] += a * PER_STEP[op]
            step[True] += n * PER_STEP[op]
            gbs = PASSES[op] * nbytes / (n * 1e-3) / 1e9
            print(f"{f'{C}x{H}x{H}':>16} {op:>4} {a:9.4f} {n:9.4f} {a / n:8.2f} {gbs:9.0f} {gbs * 1e9 / PEAK:10.2f}")
    print(f"per step (4 fwd + 5 bwd + 1 double bwd per layer): aten {step[False]:.3f} ms, amk {step[True]:.3f} ms, "
          f"saved {step[False] - step[True]:.3f} ms")


if __name__ == "__main__":
    main()
