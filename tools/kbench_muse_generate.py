"""MUSE.generate at the README's Muse shape (dim 1024, 16 heads of 64, depth 6, 8192 codes, 1024 tokens, 77 text positions,
18 steps, batch 8; the VQ decoder is a stub that returns the ids, so what is timed is the parallel decode), DESIGN.md
section 4g.1:
  (a) ``f32``          generate outside autocast: the loop as it always ran;
  (b) ``bf16 eager``   bf16 autocast with fused_sampling=False: the torch op chain on bf16 logits, the only way the decode
                       ran under autocast before the guided head;
  (c) ``bf16 guided``  bf16 autocast, fused sampling on ops.guided_logits (amk_cfg_layernorm_bf16 + amk_gemm_bf16_f32out)
                       and amk_sample_step.
The arms ALTERNATE round by round in one process after a warm-up round, so all see the same warm chip; per arm the median
of the rounds and the spread max - min (host wall time around a device synchronize).

``--part head``: the head of one step alone on the same hidden states (batch x 1024 rows): guided LayerNorm + one product
with f32 logits + sampler, against LayerNorm to bf16 + two bf16 F.linear + two casts to f32 + the sampler with its own
guidance (what a fused-sampling decode under autocast would have had to run); event time over 10 calls per round.
``--part gemm``: the logits product alone, 8192 x 8192 x 1024: both output paths of amk_gemm_bf16_f32out
(AMK_GEMM16_F32OUT=lds|direct, read per call), amk_gemm_bf16 (bf16 out) and the library's bf16 F.linear, alternating.
    python tools/kbench_muse_generate.py [--part all|model|head|gemm] [--rounds 5] [--batch 8] [--steps 18]
"""
import argparse
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from amk import dense, ops  # noqa: E402
from amk.models import MUSE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["all", "model", "head", "gemm"], default="all")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--steps", type=int, default=18)
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
DIM, HEADS, D_HEAD, DEPTH, V, T, L = 1024, 16, 64, 6, 8192, 1024, 77
B = a.batch


def med_spread(xs):
    return statistics.median(xs), max(xs) - min(xs)


def bf16(fn):
    def run():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return fn()
    return run


def alternate_events(arms, calls=10):
    """{arm: [us per call]}: event time over `calls` calls, a.rounds alternating rounds after two warm-up rounds."""
    res = {k: [] for k in arms}
    with torch.no_grad():
        for r in range(a.rounds + 2):
            for k, fn in arms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(calls):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    res[k].append(t0.elapsed_time(t1) * 1e3 / calls)
    return res


def report(res, unit="us"):
    med = {}
    for k, xs in res.items():
        med[k], sp = med_spread(xs)
        print(f"  {k:>28}: median {med[k]:.1f} {unit}, spread {sp:.1f}")
    return med


def model_part():
    class StubVQ(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.codebook = types.SimpleNamespace(codebook_size=V)
            self.num_patches = T

        def decode_indices(self, ids):
            return ids

    m = MUSE(dim=DIM, vq=StubVQ(), n_heads=HEADS, d_head=D_HEAD, depth=DEPTH, mult=4).to(dev).eval()
    text = torch.randn(B, L, 768, device=dev)

    def gen(fused):
        def run():
            m.fused_sampling = fused
            return m.generate(text, timesteps=a.steps)
        return run

    arms = {"(a) f32": gen(True), "(b) bf16 eager sampling": bf16(gen(False)), "(c) bf16 guided head": bf16(gen(True))}
    print(f"MUSE.generate: batch {B}, {T} tokens, {V} codes, depth {DEPTH}, {a.steps} steps; {a.rounds} alternating rounds "
          f"after one warm-up round; host wall time, spread = max - min; AMK_GUIDED_HEAD {int(ops.GUIDED_HEAD)}")
    res = {k: [] for k in arms}
    for r in range(a.rounds + 1):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert tuple(ids.shape) == (B, T) and bool(((ids >= 0) & (ids < V)).all())
            if r:
                res[k].append(1e3 * dt)
    med = report(res, "ms")
    for k in arms:
        print(f"  {k:>28}: {med[k] / a.steps:.2f} ms per step")
    print(f"  (c) against (a): {med['(a) f32'] / med['(c) bf16 guided head']:.2f}x; (c) against (b): "
          f"{med['(b) bf16 eager sampling'] / med['(c) bf16 guided head']:.2f}x")
    ops.KERNEL_EVENTS = {}
    bf16(gen(True))()
    torch.cuda.synchronize()
    for name, (n, ms) in sorted(ops.kernel_event_summary(ops.KERNEL_EVENTS).items()):
        if name.startswith(("cfg_layernorm", "gemm_bf16_f32out")):
            print(f"  kernel events of one guided generate: {name}: {n} launches, {1e3 * ms:.1f} us each")
    ops.KERNEL_EVENTS = None


def head_part():
    M = B * T
    h, hn = torch.randn(B, T, DIM, device=dev), torch.randn(B, T, DIM, device=dev)
    gamma, beta = torch.rand(DIM, device=dev) + 0.5, torch.zeros(DIM, device=dev)
    w = torch.randn(V, DIM, device=dev) * 0.02
    w16 = w.to(torch.bfloat16)
    ids = torch.zeros(B, T, dtype=torch.long, device=dev)
    mask = torch.ones(B, T, dtype=torch.bool, device=dev)

    def guided():
        lg = ops.guided_logits(h, gamma, beta, w, null_h=hn, cfg_scale=3.0, w16=w16)
        return ops.sample_step(lg, ids, mask=mask, tau=0.5, p=0.9, seed=1)

    def two_linears():
        _, y = ops.layer_norm_to_bf16(h, None, gamma, beta)
        _, yn = ops.layer_norm_to_bf16(hn, None, gamma, beta)
        lg, nl = F.linear(y, w16).float(), F.linear(yn, w16).float()
        return ops.sample_step(lg, ids, mask=mask, null_logits=nl, cfg_scale=3.0, tau=0.5, p=0.9, seed=1)

    print(f"the head of one step alone: {M} rows x {V} words x {DIM}; event time over 10 calls, {a.rounds} alternating rounds")
    med = report(alternate_events({"guided LN + 1 GEMM + sampler": guided, "2 LN + 2 F.linear + sampler": two_linears}))
    print(f"  two products / guided = {med['2 LN + 2 F.linear + sampler'] / med['guided LN + 1 GEMM + sampler']:.2f}")
    u = torch.empty(M, DIM, device=dev, dtype=torch.bfloat16).normal_()
    lg = torch.empty(M, V, device=dev)
    nl = torch.empty(M, V, device=dev).normal_()
    lg.normal_()
    pieces = {
        "sampler, one f32 tensor": lambda: ops.sample_step(lg.view(B, T, V), ids, mask=mask, tau=0.5, p=0.9, seed=1),
        "sampler, two f32 tensors": lambda: ops.sample_step(lg.view(B, T, V), ids, mask=mask, null_logits=nl.view(B, T, V),
                                                            cfg_scale=3.0, tau=0.5, p=0.9, seed=1),
        "F.linear bf16 + cast": lambda: F.linear(u, w16).float(),
    }
    report(alternate_events(pieces))


def gemm_part():
    M = B * T
    u = torch.randn(M, DIM, device=dev).to(torch.bfloat16)
    w16 = (torch.randn(V, DIM, device=dev) * 0.02).to(torch.bfloat16)
    gamma, beta = torch.ones(DIM, device=dev), torch.zeros(DIM, device=dev)
    hid = torch.randn(M, DIM, device=dev)
    w32 = w16.float()

    def f32out(layout):
        def run():
            os.environ["AMK_GEMM16_F32OUT"] = layout
            return ops.guided_logits(hid, gamma, beta, w32, w16=w16)
        return run

    print(f"the logits product alone: {M} x {V} x {DIM} ({2 * M * V * DIM / 1e9:.0f} GFLOP); f32out arms include the LayerNorm "
          f"pass, timed on its own below; event time over 10 calls, {a.rounds} alternating rounds")
    saved = os.environ.get("AMK_GEMM16_F32OUT")
    arms = {"LN + f32out through LDS": f32out("lds"), "LN + f32out direct": f32out("direct"),
            "amk_gemm_bf16 (bf16 out)": lambda: dense.gemm_nt_bf16(u, w16), "F.linear bf16": lambda: F.linear(u, w16),
            "LayerNorm to bf16 alone": lambda: ops.layer_norm_to_bf16(hid, None, gamma, beta)}
    med = report(alternate_events(arms))
    if saved is None:
        os.environ.pop("AMK_GEMM16_F32OUT", None)
    else:
        os.environ["AMK_GEMM16_F32OUT"] = saved
    ln = med["LayerNorm to bf16 alone"]
    for k in ("LN + f32out through LDS", "LN + f32out direct"):
        us = med[k] - ln
        print(f"  {k} minus the LayerNorm: {us:.1f} us, {2 * M * V * DIM / us / 1e6:.0f} TFLOP/s")
    with torch.no_grad():
        os.environ["AMK_GEMM16_F32OUT"] = "lds"
        x = ops.guided_logits(hid, gamma, beta, w32, w16=w16)
        os.environ["AMK_GEMM16_F32OUT"] = "direct"
        y = ops.guided_logits(hid, gamma, beta, w32, w16=w16)
        os.environ.pop("AMK_GEMM16_F32OUT", None)
    print(f"  the two output paths agree bitwise: {bool(torch.equal(x, y))}")


if a.part in ("all", "gemm"):
    gemm_part()
if a.part in ("all", "head"):
    head_part()
if a.part in ("all", "model"):
    model_part()
