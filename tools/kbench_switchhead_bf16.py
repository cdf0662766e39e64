"""SwitchHeadAttention's experts under bf16 autocast at the ViTMoE layer of BASELINE.json configs[3] -- 4160 tokens (batch
64 x 65), 8 heads, top-2, 32 experts, dim 1024, head dim 64 -- on the distinct (token, expert) lists of
amk_moe_route_distinct from random logits (P = 4160 x 32 virtual pairs, a_div = 32).

Per kernel, through the C ABI, three arms ALTERNATING round by round in one process after a warm-up: the f32 kernel the
narrow bf16 kernel replaces (csrc/moe.hip), the wide bf16 entry point of csrc/moe_bf16.hip on the same shape, and the
narrow bf16 entry point.  Then the two Functions, forward + backward, under bf16 autocast with AMK_SWITCHHEAD_BF16 off
and on (ops.SWITCHHEAD_BF16 toggled between rounds).  Median ms of the rounds, the spread of repeated rounds of the
same code (max - min, per arm), and whether the narrow arm wins by more than the two spreads combined.
The switch's default follows the train step (bench.py --model vitmoe --autocast bf16 against the parent commit), as
README's "Switches" states; this log says where the time goes."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402

from amk import lib, ops  # noqa: E402

G, H, K_SEL, E, DIM, D = 4160, 8, 2, 32, 1024, 64
FAN = H * K_SEL
BF16 = torch.bfloat16


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def make(dev):
    """{kernel: {arm: callable}}; the bf16 arms read the bf16 copies of the f32 arms' operands."""
    L = lib.load()
    U = G * H
    P = G * E
    ids, gate = ops._topk(torch.randn(U, E, device=dev), K_SEL)
    off, perm = ops._route_distinct(ids, G, FAN, E)
    x, dout = torch.randn(G, DIM, device=dev), torch.randn(G, DIM, device=dev)
    a, dv = torch.randn(U, D, device=dev), torch.randn(U, D, device=dev)
    Wv, Wo = torch.randn(E, D, DIM, device=dev) / 32, torch.randn(E, DIM, D, device=dev) / 8
    Z = torch.randn(G, E * D, device=dev)
    x16, dout16, Wv16, Wo16, Z16 = (t.to(BF16) for t in (x, dout, Wv, Wo, Z))
    V, dWv, dWo = torch.empty(P, D, device=dev), torch.empty(E, D, DIM, device=dev), torch.empty(E, DIM, D, device=dev)
    Zo, Zo16 = torch.empty(G, E * D, device=dev), torch.empty(G, E * D, device=dev, dtype=BF16)
    keep = (ids, gate, off, perm, x, dout, a, dv, Wv, Wo, Z, x16, dout16, Wv16, Wo16, Z16, V, dWv, dWo, Zo, Zo16)
    o, pm, st = _p(off), _p(perm), _s

    def chk(rc):
        lib.check(rc, "kbench_switchhead_bf16")

    fns = {
        "nt  V = x Wv^T (N 64, K 1024)": {
            "f32": lambda: chk(L.amk_grouped_gemm_nt(_p(x), DIM, E, _p(Wv), None, o, pm, P, E, D, DIM, _p(V), st())),
            "wide": lambda: chk(L.amk_grouped_gemm_nt_bf16(_p(x16), DIM, E, _p(Wv16), None, o, pm, P, E, D, DIM, _p(V), st())),
            "narrow": lambda: chk(L.amk_grouped_gemm_nt64_bf16(_p(x16), DIM, E, _p(Wv16), None, o, pm, P, E, D, DIM, _p(V), st()))},
        "nn  D = dOut Wo (N 1024, K 64)": {
            "f32": lambda: chk(L.amk_grouped_gemm_nn(_p(dout), DIM, E, _p(Wo), None, o, pm, P, E, DIM, D, _p(V), st())),
            "wide": lambda: chk(L.amk_grouped_gemm_nn_bf16(_p(dout16), DIM, E, _p(Wo16), None, o, pm, P, E, DIM, D, _p(V), st())),
            "narrow": lambda: chk(L.amk_grouped_gemm_nn64_bf16(_p(dout16), DIM, E, _p(Wo16), None, o, pm, P, E, DIM, D, _p(V), st()))},
        "wgrad dWv = Z^T x (N 64, K 1024)": {
            "f32": lambda: chk(L.amk_grouped_gemm_wgrad(_p(Z), D, 1, _p(x), DIM, E, None, o, pm, P, E, D, DIM, _p(dWv), None, st())),
            "wide": lambda: chk(L.amk_grouped_gemm_wgrad_bf16(_p(Z16), D, 1, _p(x16), DIM, E, None, o, pm, P, E, D, DIM, _p(dWv), None, st())),
            "narrow": lambda: chk(L.amk_grouped_gemm_wgrad64_bf16(_p(Z16), D, 1, _p(x16), DIM, E, None, o, pm, P, E, D, DIM, _p(dWv), st()))},
        "wgrad dWo = dOut^T Z (N 1024, K 64)": {
            "f32": lambda: chk(L.amk_grouped_gemm_wgrad(_p(dout), DIM, E, _p(Z), D, 1, None, o, pm, P, E, DIM, D, _p(dWo), None, st())),
            "wide": lambda: chk(L.amk_grouped_gemm_wgrad_bf16(_p(dout16), DIM, E, _p(Z16), D, 1, None, o, pm, P, E, DIM, D, _p(dWo), None, st())),
            "narrow": lambda: chk(L.amk_grouped_gemm_wgrad64_bf16(_p(dout16), DIM, E, _p(Z16), D, 1, None, o, pm, P, E, DIM, D, _p(dWo), st()))},
        "expert sums of gate x dV (f32 rows)": {
            "f32": lambda: chk(L.amk_moe_expert_sums(_p(dv), D, K_SEL, _p(ids), _p(gate), G, FAN, E, D, _p(Zo), st())),
            "narrow": lambda: chk(L.amk_moe_expert_sums_bf16(_p(dv), 0, D, K_SEL, _p(ids), _p(gate), G, FAN, E, D, _p(Zo16), st()))},
    }
    return fns, keep


def make_functions(dev):
    """Forward + backward of the two Functions under bf16 autocast, the switch off ("f32") and on ("narrow")."""
    U = G * H
    x = torch.randn(G, DIM, device=dev, requires_grad=True)
    a = torch.randn(U, D, device=dev, requires_grad=True)
    ls = torch.randn(U, E, device=dev, requires_grad=True)
    ld = torch.randn(U, E, device=dev)
    Wv = (torch.randn(E, D, DIM, device=dev) / 32).requires_grad_(True)
    Wo = (torch.randn(E, DIM, D, device=dev) / 8).requires_grad_(True)
    dv, dout = torch.randn(U, D, device=dev), torch.randn(G, DIM, device=dev)

    def run(fn, args, d_out, on):
        def f():
            ops.SWITCHHEAD_BF16 = on
            for t in args:
                t.grad = None
            with torch.autocast("cuda", dtype=BF16):
                out, _ = fn(*args, K_SEL, H)
            out.backward(d_out.to(out.dtype))
        return f
    return {
        "shared_row_experts fwd + bwd": {"f32": run(ops.shared_row_experts, (x, ls, Wv), dv, False),
                                         "narrow": run(ops.shared_row_experts, (x, ls, Wv), dv, True)},
        "summed_experts fwd + bwd": {"f32": run(ops.summed_experts, (a, ld, Wo), dout, False),
                                     "narrow": run(ops.summed_experts, (a, ld, Wo), dout, True)},
    }


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
    default = ops.SWITCHHEAD_BF16
    print(f"G {G} tokens, H {H}, top-{K_SEL}, E {E}, dim {DIM}, d {D}: median of {args.rounds} alternating rounds x {args.iters} launches; "
          f"spread = max - min of the rounds.  f32: the kernel / path before; wide: the 256-output / 128 x 128 bf16 entry point; "
          f"narrow: this change")
    print(f"{'kernel':>38} {'f32 ms':>8} {'spread':>7} {'wide ms':>8} {'spread':>7} {'narrow ms':>9} {'spread':>7} {'f32/narrow':>10} "
          f"{'wide/narrow':>11} {'beats f32 by > spreads':>23}")
    fns, keep = make(dev)
    fns.update(make_functions(dev))
    try:
        for kernel, arms in fns.items():
            res = {k: [] for k in arms}
            for r in range(args.rounds + 1):
                for k in arms:
                    ms = timed(arms[k], args.iters)
                    if r:   # round 0 warms up
                        res[k].append(ms)
            med = {k: statistics.median(v) for k, v in res.items()}
            spr = {k: max(v) - min(v) for k, v in res.items()}
            wide = f"{med['wide']:8.4f} {spr['wide']:7.4f}" if "wide" in arms else f"{'-':>8} {'-':>7}"
            ratio_w = f"{med['wide'] / med['narrow']:11.2f}" if "wide" in arms else f"{'-':>11}"
            print(f"{kernel:>38} {med['f32']:8.4f} {spr['f32']:7.4f} {wide} {med['narrow']:9.4f} {spr['narrow']:7.4f} "
                  f"{med['f32'] / med['narrow']:10.2f} {ratio_w} {str(med['f32'] - med['narrow'] > spr['f32'] + spr['narrow']):>23}", flush=True)
    finally:
        ops.SWITCHHEAD_BF16 = default
    del fns, keep


if __name__ == "__main__":
    main()
