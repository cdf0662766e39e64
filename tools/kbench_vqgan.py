"""One forward + backward of the conv VQGAN(256, 8192) at 256 px with the fused GroupNorm + Swish kernels (AMK_GN_ACT) off
and on, alternated round by round in one process, at the largest batch of 8, 4, 2 or 1 that fits.  Per arm: median ms with
the spread over the rounds, the peak memory of a step, and the share of the step the gnact_* calls take (device events around
every call, in a pass of its own after the timed rounds).

--autocast bf16: the step under torch.autocast(dtype=bfloat16), AMK_GN_ACT on in both arms and AMK_GN_ACT_BF16 off (the modules:
group_norm, sigmoid and mul in f32 between bf16 convolutions) and on (amk_gnact_bf16_*)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402

from amk import ops  # noqa: E402
from amk.models import VQGAN  # noqa: E402


def step(model, imgs, bf16=False):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        out, loss = model(imgs)
        total = torch.nn.functional.mse_loss(out, imgs) + loss
    total.backward()
    for p in model.parameters():
        p.grad = None


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
    ap.add_argument("--batch", type=int, default=0, help="0: the largest of 8, 4, 2, 1 that fits")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--autocast", choices=["bf16"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kbench_vqgan needs an MI355X; no device is visible")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = VQGAN(256, 8192).to(dev)

    bf16 = args.autocast == "bf16"
    switch = "AMK_GN_ACT_BF16" if bf16 else "AMK_GN_ACT"

    def arm(fused, imgs):
        if bf16:
            ops.GN_ACT, ops.GN_ACT_BF16 = True, fused
        else:
            ops.GN_ACT = fused
        step(model, imgs, bf16)

    for batch in ([args.batch] if args.batch else [8, 4, 2, 1]):
        imgs = torch.rand(batch, 3, 256, 256, device=dev)
        try:
            for fused in (False, True):      # warm-up: code objects, the convolution library's choice of algorithms
                arm(fused, imgs)
                arm(fused, imgs)
            torch.cuda.synchronize()
            break
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
            if batch == 1 or args.batch:
                raise
    res = {False: [], True: []}
    for _ in range(args.rounds):
        for fused in (False, True):
            res[fused].append(timed(lambda: arm(fused, imgs), args.iters))
    mem = {}
    for fused in (False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        arm(fused, imgs)
        torch.cuda.synchronize()
        mem[fused] = torch.cuda.max_memory_allocated() / 2 ** 30
    ops.KERNEL_EVENTS = {}
    arm(True, imgs)
    torch.cuda.synchronize()
    ev = ops.kernel_event_summary(ops.KERNEL_EVENTS)
    ops.KERNEL_EVENTS = None
    med = {f: statistics.median(res[f]) for f in res}
    spread = {f: max(res[f]) - min(res[f]) for f in res}
    print(f"VQGAN(256, 8192), batch {batch} x 3 x 256 x 256, {'bf16 autocast' if bf16 else 'f32'}, forward + backward; median [min, max] of {args.rounds} "
          f"alternated rounds x {args.iters} steps")
    for fused, name in ((False, switch + "=0 (modules)"), (True, switch + "=1 (fused)")):
        print(f"{name:>29}: {med[fused]:9.2f} ms [{min(res[fused]):.2f}, {max(res[fused]):.2f}]   peak memory {mem[fused]:.2f} GiB")
    gn = sum(n * ms for k, (n, ms) in ev.items() if k.startswith("gnact_"))
    print("fused calls per step: " + ", ".join(f"{k} {n} x {ms:.3f} ms" for k, (n, ms) in sorted(ev.items()) if k.startswith("gnact_"))
          + f" = {gn:.2f} ms, {100 * gn / med[True]:.1f}% of the fused step")
    gain = med[False] - med[True]
    print(f"difference: {gain:.2f} ms ({100 * gain / med[False]:.1f}%), spread of the arms {spread[False]:.2f} / {spread[True]:.2f} ms "
          f"-> the switch ships {'on' if gain > max(spread.values()) else 'off'}")


if __name__ == "__main__":
    main()
