"""A Parti training forward + backward at dim 512, 8 heads, d_head 64, depth 6, 1024 image tokens, 8192 codes, 77 text
positions, batch 8, with a stub tokenizer (fixed ids): per-iteration device times from HIP events, their median and
spread, and the attention kernels' share from ops.KERNEL_EVENTS.
    python tools/kbench_parti.py [--batch 8] [--iters 10]
"""
import argparse
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402

from amk import ops  # noqa: E402
from amk.models import Parti  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
DIM, HEADS, D_HEAD, DEPTH, T, V, L = 512, 8, 64, 6, 1024, 8192, 77


class StubVQ(torch.nn.Module):
    def __init__(self, ids):
        super().__init__()
        self.codebook = types.SimpleNamespace(codebook_size=V)
        self.num_patches = T
        self.ids = ids

    def encode_imgs(self, imgs):
        return self.ids


B = a.batch
model = Parti(DIM, StubVQ(torch.randint(0, V, (B, T), device=dev)), None, None, L, HEADS, D_HEAD, DEPTH).to(dev)
print(f"parameters: {sum(p.numel() for p in model.parameters()) / 1e6:.1f} M, batch {B}, {T} tokens, {V} codes")
text = torch.randn(B, L, DIM, device=dev)
imgs = torch.zeros(B, 3, 8, 8, device=dev)


def step():
    model.zero_grad(set_to_none=True)
    model(text, imgs).backward()


for _ in range(3):
    step()
torch.cuda.synchronize()
times = []
for _ in range(a.iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    step()
    t1.record()
    torch.cuda.synchronize()
    times.append(t0.elapsed_time(t1))
med = statistics.median(times)
print(f"forward + backward: median {med:.2f} ms, min {min(times):.2f}, max {max(times):.2f} ({B * 1e3 / med:.1f} images/s)")
ops.KERNEL_EVENTS = {}
step()
torch.cuda.synchronize()
attn = 0.0
for name, (n, ms) in sorted(ops.kernel_event_summary(ops.KERNEL_EVENTS).items()):
    if name.startswith("attn_"):
        attn += n * ms
        print(f"  {name}: {n} launches, {ms:.3f} ms each")
ops.KERNEL_EVENTS = None
print(f"attention kernels (self + cross, forward + backward): {attn:.2f} ms of the step")
