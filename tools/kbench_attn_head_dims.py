"""f32 attention core across head dims: forward and backward TFLOP/s and share of the f32 MFMA peak at B*H = 64,
T = 1024, D in {32, 64, 96, 128, 160, 192, 224, 256}; then D = 96 native against D = 96 zero-padded to 128 (q/k/v
copied into 128-wide buffers, the D = 128 path, o sliced; backward likewise with dO), interleaved in one process.
    python tools/kbench_attn_head_dims.py [--iters 20] [--rounds 4]
FLOPs: forward 2 products (4*B*H*T*T*D), backward credited as 4 products (8*B*H*T*T*D), as the other rows of this
project; the backward is the library's default path (delta + the one-pass kernel where one exists, else delta + the
two recompute kernels).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))

import torch  # noqa: E402

from bench import time_launches  # noqa: E402

PEAK = 157.3
DIMS = (32, 64, 96, 128, 160, 192, 224, 256)


def operands(B, H, T, D, dev, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda: torch.randn(B, T, H, D, generator=g).to(dev).permute(0, 2, 1, 3)   # the projection layout
    return mk(), mk(), mk(), mk()


def fwd_bwd(ops, q, k, v, d_o, scale):
    """(forward fn, backward fn) on these operands; the backward reuses one forward's o / stats."""
    B, H, T, D = q.shape
    fwd = lambda: ops._attn_forward(q, k, v, None, None, scale)
    q2, k2, v2, o, stats, _ = fwd()
    dq, dk, dv = (torch.empty_like(t) for t in (q2, k2, v2))

    def bwd():
        dq.zero_()   # the one-pass kernels accumulate dq with atomics
        ops._attn_backward(q2, k2, v2, o, stats, d_o, dq, dk, dv, None, None, scale)
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--H", type=int, default=8)
    ap.add_argument("--T", type=int, default=1024)
    a = ap.parse_args()
    from amk import ops

    dev = torch.device("cuda:0")
    B, H, T = a.B, a.H, a.T
    print(f"B*H = {B * H}, T = {T}; f32 MFMA peak {PEAK} TFLOP/s", flush=True)
    for D in DIMS:
        q, k, v, d_o = operands(B, H, T, D, dev, D)
        fwd, bwd = fwd_bwd(ops, q, k, v, d_o, D ** -0.5)
        core = 4.0 * B * H * T * T * D
        tf = time_launches(fwd, a.iters)
        tb = time_launches(bwd, a.iters)
        print(f"D={D:3d}  fwd {tf * 1e3:8.3f} ms {core / tf / 1e12:7.2f} TFLOP/s {core / tf / 1e12 / PEAK:.3f} of peak   "
              f"bwd {tb * 1e3:8.3f} ms {2 * core / tb / 1e12:7.2f} TFLOP/s {2 * core / tb / 1e12 / PEAK:.3f} of peak", flush=True)
        del q, k, v, d_o, fwd, bwd
        torch.cuda.empty_cache()

    # D = 96 native vs zero-padded to 128, interleaved
    D, P = 96, 128
    scale = D ** -0.5
    q, k, v, d_o = operands(B, H, T, D, dev, 7)
    nat_f, nat_b = fwd_bwd(ops, q, k, v, d_o, scale)
    qp, kp, vp, dop = (torch.zeros(B, T, H, P, device=dev).permute(0, 2, 1, 3) for _ in range(4))

    def pad_f():
        for dst, src in ((qp, q), (kp, k), (vp, v)):
            dst[..., :D].copy_(src)
        return ops._attn_forward(qp, kp, vp, None, None, scale)[3][..., :D]
    for dst, src in ((qp, q), (kp, k), (vp, v), (dop, d_o)):
        dst[..., :D].copy_(src)
    _, pad_b0 = fwd_bwd(ops, qp, kp, vp, dop, scale)

    def pad_b():
        dop[..., :D].copy_(d_o)
        pad_b0()
    # the padded path computes the same o
    o_nat = ops._attn_forward(q, k, v, None, None, scale)[3]
    err = float((pad_f() - o_nat).abs().max() / o_nat.abs().max())
    print(f"D=96 native vs padded-128: max |o diff| / max |o| = {err:.2e}", flush=True)
    core = 4.0 * B * H * T * T * D
    for rnd in range(a.rounds):
        for name, f, b in (("native  ", nat_f, nat_b), ("pad->128", pad_f, pad_b)):
            tf = time_launches(f, a.iters)
            tb = time_launches(b, a.iters)
            print(f"round {rnd} D=96 {name}  fwd {tf * 1e3:8.3f} ms {core / tf / 1e12 / PEAK:.3f} of peak   "
                  f"bwd {tb * 1e3:8.3f} ms {2 * core / tb / 1e12 / PEAK:.3f} of peak", flush=True)


if __name__ == "__main__":
    main()
