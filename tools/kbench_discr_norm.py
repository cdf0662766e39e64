"""BatchNorm2d + LeakyReLU of the PatchGAN discriminator at the benchmark's three BN-layer shapes (batch 32):
ATen (MIOpen batch norm, leaky_relu, composite double backward) against csrc/discr_norm.hip, interleaved round by
round in one process so both see the same warm chip.  Per call and per step (4 forwards, 5 first-order backwards,
1 double backward per layer), and the native kernels' rate against their algorithmic bytes (3 / 5 / 8 array passes).
    python tools/kbench_discr_norm.py [--batch 32] [--bf16]
--bf16: the same on bf16 tensors, as the pair runs under torch.autocast(bfloat16) behind a bf16 convolution: the modules
under autocast (MIOpen batch norm on bf16, ATen's leaky_relu and its composite double backward in bf16) against
ops.bn_leaky_relu_bf16 (amk_bnact_bf16_*), with the spread (max - min over the rounds) of each arm, and the fused op's rate
against a device copy measured in the same run: a copy of a tensor of the layer's own size (which the Infinity Cache helps
as it helps the op's second launch) and a copy of 1 GiB (which it cannot)."""
import argparse
import contextlib
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


def make(C, H, B, dev, native, bf16=False):
    bn = nn.BatchNorm2d(C).to(dev)
    dt = torch.bfloat16 if bf16 else torch.float32
    x = (0.5 + torch.randn(B, C, H, H, device=dev)).to(dt).requires_grad_()
    gz = torch.randn_like(x).requires_grad_()
    ggx = torch.randn_like(x)
    amp = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if bf16 else contextlib.nullcontext

    def f(inp):
        if native:
            return ops.bn_leaky_relu_bf16(inp, bn, 0.2) if bf16 else ops.bn_leaky_relu(inp, bn, 0.2)
        with amp():
            return nn.functional.leaky_relu(bn(inp), 0.2, inplace=True)

    if native and bf16:
        assert ops.bn_leaky_relu_bf16_ok(bn, x)
    z = f(x)
    assert z.dtype == dt
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


def copy_rate(nbytes, dev, iters, rounds):
    """bytes/s (read + write) of a device copy of nbytes, median over the rounds."""
    src = torch.empty(nbytes, device=dev, dtype=torch.uint8).random_(0, 255)
    dst = torch.empty_like(src)
    ms = [timed(lambda: dst.copy_(src), iters) for _ in range(rounds + 1)][1:]
    return 2 * nbytes / (statistics.median(ms) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bf16", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cases = {(C, H, nat): make(C, H, args.batch, dev, nat, args.bf16) for C, H in SHAPES for nat in (False, True)}
    res = {k: {op: [] for op in PASSES} for k in cases}
    for r in range(args.rounds + 1):
        for C, H in SHAPES:
            for op in PASSES:
                for nat in (False, True):
                    ms = timed(cases[(C, H, nat)][op], args.iters)
                    if r:   # round 0 warms up
                        res[(C, H, nat)][op].append(ms)
    step = {False: 0.0, True: 0.0}
    esize = 2 if args.bf16 else 4
    print(f"batch {args.batch}, {'bf16 (modules under autocast)' if args.bf16 else 'f32'}, median of {args.rounds} interleaved "
          f"rounds x {args.iters} calls; library {os.path.basename(os.environ.get('AMK_LIB', '')) or 'in-tree'}")
    if args.bf16:
        big = copy_rate(1 << 30, dev, 10, 5)
        print(f"device copy of 1 GiB: {big / 1e9:.0f} GB/s (read + write)")
        print(f"{'layer':>16} {'op':>4} {'aten ms':>9} {'spread':>7} {'amk ms':>9} {'spread':>7} {'speedup':>8} {'amk GB/s':>9} "
              f"{'copy GB/s':>10} {'of copy':>8} {'of 1GiB':>8}")
    else:
        print(f"{'layer':>16} {'op':>4} {'aten ms':>9} {'amk ms':>9} {'speedup':>8} {'amk GB/s':>9} {'of 6.3TB/s':>10} "
              f"{'amk spread':>10}")
    for C, H in SHAPES:
        nbytes = args.batch * C * H * H * esize
        same = copy_rate(nbytes, dev, args.iters, args.rounds) if args.bf16 else None
        for op in PASSES:
            ra, rn = res[(C, H, False)][op], res[(C, H, True)][op]
            a, n = statistics.median(ra), statistics.median(rn)
            step[False] += a * PER_STEP[op]
            step[True] += n * PER_STEP[op]
            gbs = PASSES[op] * nbytes / (n * 1e-3) / 1e9
            if args.bf16:
                print(f"{f'{C}x{H}x{H}':>16} {op:>4} {a:9.4f} {max(ra) - min(ra):7.4f} {n:9.4f} {max(rn) - min(rn):7.4f} "
                      f"{a / n:8.2f} {gbs:9.0f} {same / 1e9:10.0f} {gbs * 1e9 / same:8.2f} {gbs * 1e9 / big:8.2f}")
            else:
                print(f"{f'{C}x{H}x{H}':>16} {op:>4} {a:9.4f} {n:9.4f} {a / n:8.2f} {gbs:9.0f} {gbs * 1e9 / PEAK:10.2f} "
                      f"{max(rn) - min(rn):10.4f}")
    print(f"per step (4 fwd + 5 bwd + 1 double bwd per layer): aten {step[False]:.3f} ms, amk {step[True]:.3f} ms, "
          f"saved {step[False] - step[True]:.3f} ms")


if __name__ == "__main__":
    main()
