"""The transformer FFN under bf16 autocast at the Muse decoder's shape (M 8192 rows, dim 1024, inner 4096): the fused path
(ops.geglu_ffn -> _GEGLUFFNMixed, csrc/geglu_ln_bf16.hip) against the path before (AMK_GEGLU_FFN_BF16=0: nn.Linear under
autocast, an upcast copy, the f32 gate, the f32 LayerNorm, a downcast copy), forward + backward of a bare
transformer.FeedForward(1024, mult=6), ALTERNATING round by round in one process after a warm-up so both see the same warm
chip.  Per arm: median ms, the spread of repeated rounds of the same code (max - min of the rounds'
times), torch.cuda.max_memory_allocated above the resident inputs for one forward + backward.

Then the two fused kernels alone through ops.geglu_ln_bf16_fwd / _bwd: median microseconds and the achieved GB/s on the
bytes they must move (forward: ab read + y written; backward: ab and dy read, d_ab written, plus the dgamma / dbeta
partials written), against the copy rate measured on the same box in the same process (a bf16 tensor of ab's size copied
with Tensor.copy_: bytes read + bytes written over the median time)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402

from amk import lib, ops  # noqa: E402
from amk.models import transformer  # noqa: E402

BF16 = torch.bfloat16


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return (peak - base) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--mult", type=float, default=6)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ff = transformer.FeedForward(args.dim, mult=args.mult).to(dev)
    inner = ff.ff[3].weight.shape[1]
    M = args.rows
    x = torch.randn(M, args.dim, device=dev, dtype=BF16).requires_grad_()   # a branch input: the bf16 output of a mixed LayerNorm
    cot = torch.randn(M, args.dim, device=dev, dtype=BF16)
    params = [ff.ff[0].weight, ff.ff[2].gamma, ff.ff[3].weight]

    def arm(on):
        def run():
            ops.GEGLU_FFN_BF16 = on
            with torch.autocast("cuda", dtype=BF16):
                out = ff(x)
            return torch.autograd.grad(out, [x] + params, cot)
        return run

    fns = {"before": arm(False), "fused": arm(True)}
    print(f"FeedForward({args.dim}, mult={args.mult:g}): M {M}, inner {inner}, bf16 autocast, forward + backward")
    print(f"median of {args.rounds} alternating rounds x {args.iters} calls; spread = max - min of the rounds")
    res = {k: [] for k in fns}
    for r in range(args.rounds + 1):
        for k in ("before", "fused"):
            ms = timed(fns[k], args.iters)
            if r:   # round 0 warms up
                res[k].append(ms)
    mem = {k: peak_mb(fns[k]) for k in fns}
    print(f"{'arm':>8} {'ms':>9} {'spread':>8} {'peak MB above inputs':>22}")
    for k in ("before", "fused"):
        print(f"{k:>8} {statistics.median(res[k]):9.3f} {max(res[k]) - min(res[k]):8.3f} {mem[k]:22.0f}")
    print(f"fused / before = {statistics.median(res['fused']) / statistics.median(res['before']):.3f}", flush=True)

    # the two kernels alone against the box's copy rate
    H = inner
    ab = torch.randn(M, 2 * H, device=dev).to(BF16)
    dy = torch.randn(M, H, device=dev).to(BF16)
    gamma, beta = 0.5 + torch.rand(H, device=dev), torch.randn(H, device=dev)
    dst = torch.empty_like(ab)
    y, mean, rstd = ops.geglu_ln_bf16_fwd(ab, gamma, beta)
    nparts = lib.load().amk_geglu_ln_bf16_num_partials(M, H)
    kern = {"copy": (lambda: dst.copy_(ab), 2 * ab.numel() * 2),
            "geglu_ln_bf16_fwd": (lambda: ops.geglu_ln_bf16_fwd(ab, gamma, beta), ab.numel() * 2 + M * H * 2),
            "geglu_ln_bf16_bwd": (lambda: ops.geglu_ln_bf16_bwd(ab, dy, gamma, mean, rstd),
                                  2 * ab.numel() * 2 + M * H * 2 + nparts * 2 * H * 4)}
    kres = {k: [] for k in kern}
    for r in range(args.rounds + 1):
        for k, (fn, _) in kern.items():
            ms = timed(fn, args.iters)
            if r:
                kres[k].append(ms)
    rate = {k: kern[k][1] / (statistics.median(kres[k]) * 1e-3) / 1e9 for k in kern}
    print(f"{'kernel':>20} {'us':>9} {'spread':>8} {'MB moved':>9} {'GB/s':>8} {'of copy':>8}   ({nparts} partials)")
    for k in kern:
        print(f"{k:>20} {statistics.median(kres[k]) * 1e3:9.1f} {(max(kres[k]) - min(kres[k])) * 1e3:8.1f} {kern[k][1] / 1e6:9.1f} "
              f"{rate[k]:8.0f} {rate[k] / rate['copy']:8.2f}")


if __name__ == "__main__":
    main()
