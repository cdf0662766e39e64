"""The routed expert products of MoELayer under bf16 autocast: each entry point of csrc/moe_bf16.hip against its f32
counterpart of csrc/moe.hip on the same (offsets, perm) lists, through the C ABI, ALTERNATING round by round in one
process after a warm-up so both see the same warm chip.  Per kernel: median ms of both arms, the spread of repeated
rounds of the same code (max - min of the rounds' times, per arm), the ratio, and the bf16 kernel's credited TFLOP/s --
2 P N Kd, the product's useful work -- named as a share of the DENSE bf16 MFMA peak (2.5 PFLOP/s, the figure DESIGN.md
uses), which no grouped kernel with 64-pair tiles and a gather reaches.

Cases: the ViTMoE layer of BASELINE.json configs[3] -- 4160 tokens (batch 64 x 65), 32 experts, top-2: P = 8320 pairs
routed by amk_moe_route from random logits, N = Kd = 1024 -- and the same size with a skewed routing
(moe_ref.skewed_counts(8320, 32): a few long experts next to ones of a handful of pairs).
The default rule of AMK_MOE_BF16 (README): each bf16 kernel must beat its f32 counterpart by more than the two arms'
spreads combined; the train step decides the rest (bench.py --model vitmoe --autocast bf16 against the parent commit)."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from amk import lib, ops  # noqa: E402

PEAK_BF16 = 2500.0   # TFLOP/s, dense bf16 MFMA
E, K_SEL, TOKENS, N, KD = 32, 2, 4160, 1024, 1024


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def lists(kind, dev):
    if kind == "random logits":
        r = ops.moe_route(torch.randn(TOKENS, E, device=dev), K_SEL)
        return r["offsets"], r["perm"]
    import moe_ref

    _, off, perm = moe_ref.make_lists(moe_ref.skewed_counts(TOKENS * K_SEL, E), seed=0)
    return off.to(dev), perm.to(dev)


def make(off, perm, dev):
    """{kernel: {arm: callable}} on one set of lists; the bf16 arms read the bf16 copies of the f32 arms' operands."""
    L = lib.load()
    P = TOKENS * K_SEL
    x = torch.randn(TOKENS, KD, device=dev)
    g = torch.randn(TOKENS, N, device=dev)
    W = torch.randn(E, N, KD, device=dev) / 32
    bias, scale = torch.randn(E, N, device=dev), torch.rand(P, device=dev)
    x16, g16, W16 = x.bfloat16(), g.bfloat16(), W.bfloat16()
    Y, dX = torch.empty(P, N, device=dev), torch.empty(P, KD, device=dev)
    dW, db = torch.empty(E, N, KD, device=dev), torch.empty(E, N, device=dev)

    def chk(rc):
        lib.check(rc, "kbench_moe_bf16")

    return {
        "nt": {"f32": lambda: chk(L.amk_grouped_gemm_nt(_p(x), KD, K_SEL, _p(W), _p(bias), _p(off), _p(perm), P, E, N, KD, _p(Y), _s())),
               "bf16": lambda: chk(L.amk_grouped_gemm_nt_bf16(_p(x16), KD, K_SEL, _p(W16), _p(bias), _p(off), _p(perm), P, E, N, KD, _p(Y), _s()))},
        "nn": {"f32": lambda: chk(L.amk_grouped_gemm_nn(_p(g), N, K_SEL, _p(W), _p(scale), _p(off), _p(perm), P, E, N, KD, _p(dX), _s())),
               "bf16": lambda: chk(L.amk_grouped_gemm_nn_bf16(_p(g16), N, K_SEL, _p(W16), _p(scale), _p(off), _p(perm), P, E, N, KD, _p(dX), _s()))},
        "wgrad": {"f32": lambda: chk(L.amk_grouped_gemm_wgrad(_p(g), N, K_SEL, _p(x), KD, K_SEL, _p(scale), _p(off), _p(perm), P, E, N, KD,
                                                              _p(dW), _p(db), _s())),
                  "bf16": lambda: chk(L.amk_grouped_gemm_wgrad_bf16(_p(g16), N, K_SEL, _p(x16), KD, K_SEL, _p(scale), _p(off), _p(perm), P, E, N, KD,
                                                                    _p(dW), _p(db), _s()))},
    }, (x, g, W, bias, scale, x16, g16, W16, Y, dX, dW, db)


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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    P = TOKENS * K_SEL
    flop = 2.0 * P * N * KD
    print(f"P {P} pairs, E {E}, N {N}, Kd {KD}: {flop / 1e9:.1f} GFLOP per launch; median of {args.rounds} alternating rounds x "
          f"{args.iters} launches; spread = max - min of the rounds; credited TFLOP/s of the bf16 arm against the dense bf16 peak {PEAK_BF16:g}")
    print(f"{'routing':>14} {'kernel':>6} {'f32 ms':>8} {'spread':>7} {'bf16 ms':>8} {'spread':>7} {'f32/bf16':>9} {'faster by > spreads':>20} "
          f"{'credited TF':>11} {'of dense peak':>13}")
    for kind in ("random logits", "skewed"):
        off, perm = lists(kind, dev)
        fns, keep = make(off, perm, dev)
        for kernel, arms in fns.items():
            res = {k: [] for k in arms}
            for r in range(args.rounds + 1):
                for k in ("f32", "bf16"):
                    ms = timed(arms[k], args.iters)
                    if r:   # round 0 warms up
                        res[k].append(ms)
            a, b = statistics.median(res["f32"]), statistics.median(res["bf16"])
            sa, sb = max(res["f32"]) - min(res["f32"]), max(res["bf16"]) - min(res["bf16"])
            tf = flop / (b * 1e-3) / 1e12
            print(f"{kind:>14} {kernel:>6} {a:8.4f} {sa:7.4f} {b:8.4f} {sb:7.4f} {a / b:9.2f} {str(a - b > sa + sb):>20} {tf:11.1f} "
                  f"{tf / PEAK_BF16:13.3f}", flush=True)
        del fns, keep


if __name__ == "__main__":
    main()
