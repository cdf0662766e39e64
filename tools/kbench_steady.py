"""The hand-written attention / VQ kernels of the ViT-VQGAN step, back to back, interleaved for several rounds inside ONE process:
the last rounds are the steady state of a warm chip.  (Single-shot timings of a fresh process, and timings taken after minutes of
full load, differ from these by up to 10 %: the chip's clock follows its power / thermal state.)
    python tools/kbench_steady.py [--batch 32] [--rounds 4] [--x6-shapes]
--x6-shapes: instead, the f32 and the split-bf16 forward (both keeping scores, pre-pass included) at the shapes that set
ops.ATTENTION_X6_MIN_KEYS / _MIN_SCORES: (I, J) = (1024, 1024), (1024, 77), (65, 65), and the first two with a key mask.
The split-bf16 rows (csrc/attn_fwd_x6.hip): "masked kernel" = attn_fwd_x6_kernel on the unmasked call (AMK_ATTN_FWD_PLAIN=0),
the loop the unmasked specialisation replaced."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tools.kbench_moe import time_launches  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--x6-shapes", action="store_true")
a = ap.parse_args()
from amk import lib, ops  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
B, H, T, D = a.batch, 8, 1024, 64


def fwd_as(mode, env=None, **kw):
    """_attn_forward of (q, k, v) under ops.ATTENTION_FORWARD = mode and, for the call, the environment switch `env`."""
    def run(q, k, v, key_mask=None):
        old, ops.ATTENTION_FORWARD = ops.ATTENTION_FORWARD, mode
        if env:
            os.environ[env[0]] = env[1]
        try:
            return ops._attn_forward(q, k, v, key_mask, None, D ** -0.5, **kw)
        finally:
            ops.ATTENTION_FORWARD = old
            if env:
                del os.environ[env[0]]
    return run


if a.x6_shapes:
    for I, J, masked in ((1024, 1024, False), (1024, 77, False), (65, 65, False), (1024, 77, True), (1024, 1024, True)):
        q, k, v = (torch.randn(B, n, H, D, device=dev).permute(0, 2, 1, 3) for n in (I, J, J))
        km = (torch.rand(B, J, device=dev) < 0.8).to(torch.uint8) if masked else None   # a key-padding mask: the mask kernels
        fl = 4.0 * B * H * I * J * D
        for rnd in range(a.rounds):
            for name, fn in (("f32 keep", fwd_as("f32", keep_scores=True)), ("x6 keep", fwd_as("bf16x6", keep_scores=True)),
                             ("f32", fwd_as("f32")), ("x6", fwd_as("bf16x6"))):
                t = time_launches(lambda: fn(q, k, v, km), a.iters)
                print(f"round {rnd} I {I:5d} J {J:5d} {'key mask' if masked else 'no mask ':8s} {name:9s} {t*1e3:.4f} ms  {fl/t/1e12:6.1f} TFLOP/s")
    sys.exit(0)
q, k, v, d_o = (torch.randn(B, T, H, D, device=dev).permute(0, 2, 1, 3) for _ in range(4))
s = D ** -0.5
core = 4.0 * B * H * T * T * D
q, k, v, o, stats, scores = ops._attn_forward(q, k, v, None, None, s, keep_scores=True)
dq, dk, dv = (torch.empty_like(q) for _ in range(3))
delta = torch.empty(lib.load().amk_attn_bwd_ws_floats(B, H, T, T, 72), device=dev)
bwd = lambda st, sc=None: ops._attn_backward(q, k, v, o, stats, d_o, dq, dk, dv, None, None, s, stages=st, delta=delta, scores=sc)
N, K, C = B * T, 8192, 32
z = torch.randn(N, C, device=dev)
cb = torch.randn(K, C, device=dev)
rows = [("attn_fwd (plain kernel)", lambda: ops._attn_forward(q, k, v, None, None, s), core),
        ("attn_fwd keeping scores", lambda: ops._attn_forward(q, k, v, None, None, s, keep_scores=True), core),
        ("attn_fwd x6, masked kernel (+ pre-pass)", lambda: fwd_as("bf16x6", ("AMK_ATTN_FWD_PLAIN", "0"))(q, k, v), core),
        ("attn_fwd x6 plain (+ pre-pass)", lambda: fwd_as("bf16x6")(q, k, v), core),
        ("attn_fwd x6 keeping scores (+ pre-pass)", lambda: fwd_as("bf16x6", keep_scores=True)(q, k, v), core),
        ("attn_bwd fused, kept scores (+ dq memset)", lambda: bwd(8, scores), 2 * core),
        ("attn_bwd fused, recomputing", lambda: bwd(8), 2 * core),
        ("vq_lookup_fwd (prep + argmin + finalize)", lambda: ops.vq_lookup(z, cb, 0.25), 2.0 * N * K * C)]
for rnd in range(a.rounds):
    for name, fn, fl in rows:
        t = time_launches(fn, a.iters)
        print(f"round {rnd} {name:44s} {t*1e3:.4f} ms  {fl/t/1e12:6.1f} TFLOP/s  {fl/t/1e12/157.3:.3f} of the f32 MFMA peak")
