"""The LPIPS distance head at the five level shapes of the GAN step at 256 px (64 x 256^2, 128 x 128^2, 256 x 64^2, 512 x 32^2,
512 x 16^2): the torch chain of lpips 0.1.4 (ops._lpips_chain) against csrc/lpips.hip (ops.lpips_distance with AMK_LPIPS on),
forward + backward for the first feature tensor, the arms interleaved round by round in one process after a warm-up round so
both see the same warm chip.  Per arm: median ms with the spread over the rounds, GB/s on the bytes the algorithm needs (seven
array passes: a and b twice forward, a and b once and ga once backward) against the rate of a device copy measured in the
same run, and the peak memory above the inputs (a, b, w) during one forward + backward.

--autocast bf16: the same under torch.autocast(dtype=bfloat16) on bf16 features, as the convolutions hand them over there
(amk_lpips_bf16_*); seven passes at 2 bytes per element.
--batch: 8 (default) or 32, the shipped batch.
--px P: the five level shapes of a P px image instead (224: 196 pixels at the last level, no multiple of 8).
--step: the whole GAN step (bench.py's model and discriminator) with per_loss = LPIPS() at weight 1 and the switch
alternated: one trainer (the same initial weights) and one captured step per arm, replayed in alternating rounds; the losses
are checked after every round and the tool stops at a non-finite one.  As it stands the two-arm flow ends that way in its
first round, so it has given no step-level figure yet.  With one arm (--arms 0 --no-per-loss) it runs to the end with finite
losses that are still wrong (an l1 of 12.6 next to an l2 of 0.67 on the same reconstruction), while the same model, batch
and seed without the two tuning calls below replay cleanly: DESIGN.md section 4k.  --arms, --no-per-loss and
--no-conv-autotune are there to narrow that down."""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402

from amk import ops  # noqa: E402

CHANNELS = (64, 128, 256, 512, 512)   # level k is CHANNELS[k] x (px / 2^k)^2
PASSES = 7


def make(C, H, B, dev, fused, bf16=False):
    dtype = torch.bfloat16 if bf16 else torch.float32
    a = torch.relu(torch.randn(B, C, H, H, device=dev)).to(dtype).requires_grad_()
    b = torch.relu(torch.randn(B, C, H, H, device=dev)).to(dtype)
    w = torch.rand(C, device=dev)

    def step():
        ops.LPIPS = fused
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            out = ops.lpips_distance(a, b, w)
        assert ("LpipsDist" in type(out.grad_fn).__name__) == fused
        out.sum().backward()
        a.grad = None

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


def heads(args, dev, bf16):
    peak = copy_rate(dev, args.iters)
    print(f"batch {args.batch}, {'bf16 autocast' if bf16 else 'f32'}, forward + backward, median [min, max] of {args.rounds} "
          f"interleaved rounds x {args.iters} calls; device copy {peak / 1e9:.0f} GB/s")
    print(f"{'level':>14} {'chain ms':>24} {'fused ms':>24} {'speedup':>8} {'chain GB/s':>10} {'fused GB/s':>10} {'of copy':>8} "
          f"{'chain MiB':>9} {'fused MiB':>9}")
    tot = {False: 0.0, True: 0.0}
    for C, H in [(c, args.px >> k) for k, c in enumerate(CHANNELS)]:
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
        print(f"{f'{C}x{H}x{H}':>14} {fmt(False):>24} {fmt(True):>24} {med[False] / med[True]:8.2f} {gbs[False]:10.0f} "
              f"{gbs[True]:10.0f} {gbs[True] * 1e9 / peak:8.2f} {mem[False]:9.0f} {mem[True]:9.0f}", flush=True)
        del arms
        torch.cuda.empty_cache()
    print(f"sum over the five levels: chain {tot[False]:.3f} ms, fused {tot[True]:.3f} ms")


def whole_step(args, dev, bf16):
    import bench
    from amk import tuning
    from amk.models import LPIPS, ViTVQGAN
    from amk.models.discriminator import NLayerDiscriminator
    from amk.train import VQGANTrainStep

    tuning.enable_gemm_tuning()
    tuning.enable_conv_autotune(not args.no_conv_autotune)
    img = torch.rand(args.batch, 3, 256, 256, device=dev)
    torch.manual_seed(0)
    model, discr, per = ViTVQGAN(bench.VIT, bench.CODEBOOK).to(dev), NLayerDiscriminator(3, 64, 3).to(dev), LPIPS().to(dev)
    trs, mem = {}, {}
    arms = [c == "1" for c in args.arms]
    for arm in arms:                     # one trainer and one captured step per arm, the same initial weights
        ops.LPIPS = arm                  # the switch is read per call, so each capture records its own arm
        tr = trs[arm] = VQGANTrainStep(copy.deepcopy(model), copy.deepcopy(discr), autocast=torch.bfloat16 if bf16 else None,
                                       capturable=True, per_loss=None if args.no_per_loss else per,
                                       per_loss_weight=1.0)
        for i in range(3):               # eager first (also fixes the set of parameters with gradients)
            logs = tr.step(img)
        print(f"AMK_LPIPS={int(arm)}, after 3 eager steps: " + ", ".join(f"{k} {float(v):.4f}" for k, v in logs.items()), flush=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tr.capture(img)
        torch.cuda.synchronize()
        mem[arm] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    times = {arm: [] for arm in arms}
    for r in range(args.rounds + 1):
        for arm in arms:
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(args.iters):
                logs = trs[arm].step(img)
            torch.cuda.synchronize()
            dt = (time.time() - t0) / args.iters * 1e3
            if not all(bool(torch.isfinite(v)) for v in logs.values()):      # a timing of NaN steps says nothing
                raise SystemExit(f"round {r}, AMK_LPIPS={int(arm)}: the step's losses are not finite: "
                                 + ", ".join(f"{k} {float(v)}" for k, v in logs.items()))
            print(f"round {r}, AMK_LPIPS={int(arm)}: {dt:.3f} ms per step, losses "
                  + ", ".join(f"{k} {float(v):.4f}" for k, v in logs.items()), flush=True)
            if r:                        # round 0 warms up
                times[arm].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"GAN step with per_loss, batch {args.batch}, {'bf16 autocast' if bf16 else 'f32'}; losses "
          + ", ".join(f"{k} {float(v):.4f}" for k, v in logs.items()))
    for arm in arms:
        v = times[arm]
        print(f"captured step, AMK_LPIPS={int(arm)}: median {med[arm]:.3f} ms, min {min(v):.3f}, max {max(v):.3f}, spread "
              f"{max(v) - min(v):.3f} ms over {args.rounds} rounds x {args.iters} replays; peak memory of the capture above what "
              f"was allocated before it {mem[arm]:.2f} GiB")
    if len(arms) == 2:
        print(f"AMK_LPIPS=1 against 0: {med[False] - med[True]:+.3f} ms per step saved")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--autocast", choices=["bf16"], default=None)
    ap.add_argument("--px", type=int, default=256, help="image size of the head shapes (224: 14 x 14 at the last level, "
                    "which bf16 walks one element at a time)")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--arms", default="01", choices=["01", "0", "1"], help="with --step: the values of the switch to run")
    ap.add_argument("--no-per-loss", action="store_true", help="with --step: the same flow without the perceptual term")
    ap.add_argument("--no-conv-autotune", action="store_true", help="with --step: leave the convolutions' algorithms to the library's default choice")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_lpips needs an MI355X; no device is visible")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    (whole_step if args.step else heads)(args, dev, args.autocast == "bf16")


if __name__ == "__main__":
    main()
