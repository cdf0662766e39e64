"""A Parti training forward + backward at dim 512, 8 heads, d_head 64, depth 6, 1024 image tokens, 8192 codes, 77 text
positions, batch 8, with a stub tokenizer (fixed ids).  Two arms -- ops.CE_HEAD on (the fused logits + bias +
cross-entropy head, Parti.loss_from_hidden) and off (to_logits + F.cross_entropy) -- ALTERNATE round by round in one
process after a warm-up, so both see the same warm chip.  Per arm: the median of the rounds'
per-step device times (HIP events), the spread max - min of the rounds, and the loss head's share of the step: for the
fused arm the ce_head launches of ops.KERNEL_EVENTS; for the module arm, whose head is library kernels without a label,
final_norm's output -> to_logits -> F.cross_entropy, forward + backward, timed apart on tensors of the step's shapes.
The attention kernels' share comes from ops.KERNEL_EVENTS as before.
    python tools/kbench_parti.py [--batch 8] [--iters 5] [--rounds 5] [--autocast bf16]
"""
import argparse
import contextlib
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from amk import ops  # noqa: E402
from amk.models import Parti  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--autocast", choices=["none", "bf16"], default="none")
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
DIM, HEADS, D_HEAD, DEPTH, T, V, L = 512, 8, 64, 6, 1024, 8192, 77


def amp():
    return torch.autocast("cuda", dtype=torch.bfloat16) if a.autocast == "bf16" else contextlib.nullcontext()


class StubVQ(torch.nn.Module):
    def __init__(self, ids):
        super().__init__()
        self.codebook = types.SimpleNamespace(codebook_size=V)
        self.num_patches = T
        self.ids = ids

    def encode_imgs(self, imgs):
        return self.ids


B = a.batch
labels = torch.randint(0, V, (B, T), device=dev)
model = Parti(DIM, StubVQ(labels), None, None, L, HEADS, D_HEAD, DEPTH).to(dev)
print(f"parameters: {sum(p.numel() for p in model.parameters()) / 1e6:.1f} M, batch {B}, {T} tokens, {V} codes, autocast "
      f"{a.autocast}")
text = torch.randn(B, L, DIM, device=dev)
imgs = torch.zeros(B, 3, 8, 8, device=dev)
ARMS = {"fused head": True, "module head": False}


def step():
    model.zero_grad(set_to_none=True)
    with amp():
        loss = model(text, imgs)
    loss.backward()


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


res = {k: [] for k in ARMS}
for r in range(a.rounds + 1):
    for k, on in ARMS.items():
        ops.CE_HEAD = on
        ms = timed(step, a.iters)
        if r:   # round 0 warms up
            res[k].append(ms)

hidden = torch.randn(B, T, DIM, device=dev).requires_grad_()


def module_head():
    model.zero_grad(set_to_none=True)
    with amp():
        loss = F.cross_entropy(model.to_logits(hidden).transpose(1, 2), labels)
    return torch.autograd.grad(loss, (hidden, model.to_logits.weight, model.to_logits.bias))


timed(module_head, 2)
head_module = statistics.median(timed(module_head, a.iters) for _ in range(a.rounds))

print(f"forward + backward, median of {a.rounds} alternating rounds x {a.iters} steps; spread = max - min of the rounds")
for k, on in ARMS.items():
    ops.CE_HEAD = on
    ops.KERNEL_EVENTS = {}
    step()
    torch.cuda.synchronize()
    summ = ops.kernel_event_summary(ops.KERNEL_EVENTS)
    ops.KERNEL_EVENTS = None
    attn = sum(n * ms for name, (n, ms) in summ.items() if name.startswith("attn_") or name.startswith("bf16_attn_"))
    head = sum(n * ms for name, (n, ms) in summ.items() if "ce_head" in name)
    med, sp = statistics.median(res[k]), max(res[k]) - min(res[k])
    if on:
        assert head > 0, "the fused head did not run (AMK_CE_HEAD=0 in the environment?)"
        where = "ce_head launches of this step"
    else:
        assert head == 0
        head, where = head_module, "to_logits + F.cross_entropy timed apart"
    print(f"{k:>12}: median {med:.2f} ms, spread {sp:.2f} ({B * 1e3 / med:.1f} images/s); loss head {head:.2f} ms = "
          f"{100 * head / med:.1f} % of the step ({where}); attention kernels {attn:.2f} ms")
    for name, (n, ms) in sorted(summ.items()):
        if "ce_head" in name:
            print(f"  {name}: {n} launches, {ms:.3f} ms each")
f, m = statistics.median(res["fused head"]), statistics.median(res["module head"])
sf, sm = max(res["fused head"]) - min(res["fused head"]), max(res["module head"]) - min(res["module head"])
print(f"fused - module: {f - m:+.2f} ms against the spreads {sf:.2f} + {sm:.2f}: "
      f"{'the fused head is faster by more than the spreads' if m - f > sf + sm else 'NOT faster by more than the spreads'}")
