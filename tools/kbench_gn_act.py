"""GroupNorm(32, C, eps=1e-6) + Swish of the conv VQGAN at its five layer shapes (batch 8): nn.GroupNorm + x * sigmoid(x)
against csrc/gn_act.hip (ops.group_norm_act), forward + backward, interleaved round by round in one process so both arms
see the same warm chip.  Per arm: median ms with the spread over the rounds, GB/s on the algorithmic bytes (five array
passes: x -> z, then x, gz -> gx) against the rate of a device copy measured in the same run, and the peak memory above the
inputs (x, gz and the parameters) during one forward + backward.

--autocast bf16: the same under torch.autocast(dtype=bfloat16) on a bf16 x and gz, as the layers sit between two convolutions
there: the module path (the cast to f32 that autocast puts in front of group_norm, the f32 norm, sigmoid and mul, and the cast
of the result to bf16 that the next convolution makes) against amk_gnact_bf16_* (AMK_GN_ACT_BF16); the algorithmic bytes are
the same five passes at 2 bytes per element."""
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

SHAPES = [(128, 256), (128, 128), (256, 64), (256, 32), (512, 16)]   # (C, H = W)
PASSES = 5


def make(C, H, B, dev, fused, bf16=False):
    gn = nn.GroupNorm(32, C, eps=1e-6).to(dev)
    dtype = torch.bfloat16 if bf16 else torch.float32
    x = torch.randn(B, C, H, H, device=dev).to(dtype).requires_grad_()
    gz = torch.randn(B, C, H, H, device=dev).to(dtype)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            if fused:
                z = ops.group_norm_act(x, gn, 1)
            else:
                y = gn(x)
                z = (y * torch.sigmoid(y)).to(dtype)       # under autocast: the cast the next convolution makes
        assert z.dtype == dtype and ("GNAct" in type(z.grad_fn).__name__) == fused
        z.backward(gz)
        x.grad = gn.weight.grad = gn.bias.grad = None

    return step


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def copy_rate(dev, iters):
    """bytes/s of dst.copy_(src) on 512 MiB (read + write counted)."""
    src = torch.empty(128 << 20, device=dev)
    dst = torch.empty_like(src)
    timed(lambda: dst.copy_(src), 3)
    ms = statistics.median(timed(lambda: dst.copy_(src), iters) for _ in range(5))
    return 2 * src.numel() * 4 / (ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--autocast", choices=["bf16"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_gn_act needs an MI355X; no device is visible")
    assert ops.GN_ACT or os.environ.get("AMK_GN_ACT") is None, "AMK_GN_ACT=0 would time the modules twice"
    ops.GN_ACT = True
    bf16 = args.autocast == "bf16"
    assert not bf16 or ops.GN_ACT_BF16 or os.environ.get("AMK_GN_ACT_BF16") is None, "AMK_GN_ACT_BF16=0 would time the modules twice"
    ops.GN_ACT_BF16 = True
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    peak = copy_rate(dev, args.iters)
    print(f"batch {args.batch}, {'bf16 autocast' if bf16 else 'f32'}, forward + backward, median [min, max] of {args.rounds} interleaved rounds x {args.iters} calls; "
          f"device copy {peak / 1e9:.0f} GB/s")
    print(f"{'layer':>14} {'modules ms':>24} {'fused ms':>24} {'speedup':>8} {'mod GB/s':>9} {'fused GB/s':>10} {'of copy':>8} "
          f"{'mod MiB':>8} {'fused MiB':>9}")
    tot = {False: 0.0, True: 0.0}
    for C, H in SHAPES:
        arms = {f: make(C, H, args.batch, dev, f, bf16) for f in (False, True)}
        res = {False: [], True: []}
        for r in range(args.rounds + 1):
            for f in (False, True):
                ms = timed(arms[f], args.iters)
                if r:   # round 0 warms up
                    res[f].append(ms)
        mem = {f: peak_above_inputs(arms[f]) for f in (False, True)}
        nbytes = PASSES * args.batch * C * H * H * (2 if bf16 else 4)
        med = {f: statistics.median(res[f]) for f in res}
        fmt = lambda f: f"{med[f]:8.4f} [{min(res[f]):.4f}, {max(res[f]):.4f}]"  # noqa: E731
        gbs = {f: nbytes / (med[f] * 1e-3) / 1e9 for f in res}
        for f in res:
            tot[f] += med[f]
        print(f"{f'{C}x{H}x{H}':>14} {fmt(False):>24} {fmt(True):>24} {med[False] / med[True]:8.2f} {gbs[False]:9.0f} "
              f"{gbs[True]:10.0f} {gbs[True] * 1e9 / peak:8.2f} {mem[False]:8.0f} {mem[True]:9.0f}")
    print(f"sum over the five shapes: modules {tot[False]:.3f} ms, fused {tot[True]:.3f} ms")


if __name__ == "__main__":
    main()
