"""The masked-token loss head: ops.linear_cross_entropy (csrc/ce_head.hip) against the parent path, F.linear +
F.cross_entropy(ignore_index), forward + backward, ALTERNATING round by round in one process after a warm-up so both see
the same warm chip.  Per case: median ms of both paths, the spread of repeated rounds of the same code (max - min of the
rounds' times, per path), torch.cuda.max_memory_allocated above the resident inputs for one forward + backward of each
path, and the fused op's credited TFLOP/s -- 2 M V K for each of the parent's three products (logits, dx, dw) over ALL
rows, the work the fused op replaces -- against the f32 MFMA peak.

Cases: the Muse head of bench.py --model muse (8192 rows, 8192 words, dim 1024) with targets drawn by fill_mask's cosine
schedule; a MaskGit-sized head (8 x 256 tokens, dim 768, 8192 words, same schedule); the Muse head with every row valid.
The default rule of AMK_CE_HEAD (README): on only if the fused op is not slower than the parent path at the Muse size by
more than the spread.

--autocast bf16: the same three cases inside torch.autocast("cuda", bfloat16) with bf16 inputs and an f32 master weight,
as the autocast train step has them: the fused op is then csrc/ce_head_bf16.hip, the parent path F.linear +
F.cross_entropy as autocast runs them (bf16 GEMMs over all rows, bf16 logits, their f32 copy for the softmax), and the
credited TFLOP/s are set against the dense bf16 MFMA peak.  The same rule decides the default of AMK_CE_HEAD_BF16.

--bias: the op with a bias (ops.linear_cross_entropy(..., bias=b): amk_ce_head_bias_*) against F.linear(x, w, b) +
F.cross_entropy at Parti's head (8192 rows, all valid, 8192 words) at dim 512 and 1024, and beside them the BIASLESS fused
op on the same tensors, a third arm of the same rounds: the difference is what the bias preload and db cost."""
import argparse
import contextlib
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from amk import ops  # noqa: E402

PEAK = 157.3   # TFLOP/s, f32 MFMA
PEAK_BF16 = 2500.0   # TFLOP/s, dense bf16 MFMA (the figure DESIGN.md uses)
CASES = [("muse 8x1024 d1024 V8192", 8, 1024, 1024, 8192, "schedule"),
         ("maskgit 8x256 d768 V8192", 8, 256, 768, 8192, "schedule"),
         ("muse, every row valid", 8, 1024, 1024, 8192, "all")]
CASES_BIAS = [("parti 8x1024 d512 V8192", 8, 1024, 512, 8192, "all"),
              ("parti rows, d1024 V8192", 8, 1024, 1024, 8192, "all")]


def schedule_targets(B, T, V, dev, mode):
    """MUSE.fill_mask's targets: a uniform timestep per image, cos(t pi / 2) T tokens masked (the rest -1)."""
    tokens = torch.randint(0, V, (B, T), device=dev)
    if mode == "all":
        return tokens
    t = torch.rand(B, device=dev)
    n_masked = (T * torch.cos(t * math.pi / 2).clip(0)).round().clamp(min=1)
    order = torch.rand(B, T, device=dev).argsort(dim=-1)
    return tokens.masked_fill(~(order < n_masked.unsqueeze(-1)), -1)


def make(B, T, K, V, mode, dev, autocast=None, bias=False):
    x = torch.randn(B, T, K, device=dev, dtype=torch.bfloat16 if autocast else torch.float32).requires_grad_()
    w = (torch.randn(V, K, device=dev) * 0.02).requires_grad_()
    tgt = schedule_targets(B, T, V, dev, mode)

    def amp():
        return torch.autocast("cuda", dtype=autocast) if autocast else contextlib.nullcontext()

    def fused():
        with amp():
            loss = ops.linear_cross_entropy(x, w, tgt, -1)
        return torch.autograd.grad(loss, (x, w))

    def parent():
        with amp():
            loss = F.cross_entropy(F.linear(x, w).transpose(1, 2), tgt, ignore_index=-1)
        return torch.autograd.grad(loss, (x, w))

    if bias:
        b = torch.randn(V, device=dev).requires_grad_()

        def fused_b():
            with amp():
                loss = ops.linear_cross_entropy(x, w, tgt, -1, bias=b)
            return torch.autograd.grad(loss, (x, w, b))

        def parent_b():
            with amp():
                loss = F.cross_entropy(F.linear(x, w, b).transpose(1, 2), tgt, ignore_index=-1)
            return torch.autograd.grad(loss, (x, w, b))

        return {"fused": fused_b, "parent": parent_b, "biasless": fused}, float((tgt != -1).float().mean())
    return {"fused": fused, "parent": parent}, float((tgt != -1).float().mean())


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--autocast", choices=["none", "bf16"], default="none")
    ap.add_argument("--bias", action="store_true")
    args = ap.parse_args()
    autocast = torch.bfloat16 if args.autocast == "bf16" else None
    peak = PEAK_BF16 if autocast else PEAK
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    print(f"autocast {args.autocast}: fused = {'csrc/ce_head_bf16.hip' if autocast else 'csrc/ce_head.hip'}, credited TFLOP/s "
          f"against {peak:g}")
    print(f"forward + backward, median of {args.rounds} alternating rounds x {args.iters} calls; spread = max - min of the rounds")
    print(f"{'case':>26} {'valid':>6} {'parent ms':>10} {'spread':>7} {'fused ms':>9} {'spread':>7} {'fused/parent':>12} "
          f"{'parent MB':>10} {'fused MB':>9} {'credited TF':>11} {'of peak':>8}"
          + (f" {'biasless ms':>12} {'spread':>7} {'biasless MB':>12}" if args.bias else ""))
    for name, B, T, K, V, mode in (CASES_BIAS if args.bias else CASES):
        fns, frac = make(B, T, K, V, mode, dev, autocast, args.bias)
        res = {k: [] for k in fns}
        for r in range(args.rounds + 1):
            for k in (("parent", "fused", "biasless") if args.bias else ("parent", "fused")):
                ms = timed(fns[k], args.iters)
                if r:   # round 0 warms up
                    res[k].append(ms)
        mem = {k: peak_mb(fns[k]) for k in fns}
        p, f = statistics.median(res["parent"]), statistics.median(res["fused"])
        sp, sf = max(res["parent"]) - min(res["parent"]), max(res["fused"]) - min(res["fused"])
        tf = 3 * 2.0 * B * T * V * K / (f * 1e-3) / 1e12
        print(f"{name:>26} {frac:6.2f} {p:10.3f} {sp:7.3f} {f:9.3f} {sf:7.3f} {f / p:12.2f} {mem['parent']:10.0f} "
              f"{mem['fused']:9.0f} {tf:11.1f} {tf / peak:8.3f}"
              + (f" {statistics.median(res['biasless']):12.3f} {max(res['biasless']) - min(res['biasless']):7.3f} "
                 f"{mem['biasless']:12.0f}" if args.bias else ""), flush=True)
        del fns


if __name__ == "__main__":
    main()
