"""A prompt through Parti's KV-cached decoder at dim 512, 8 heads, d_head 64, depth 6, 8192 codes, 77 text positions,
batch 8, stub tokenizer, f32 and under bf16 autocast:
  (a) ``prefill``: the start token and the n given tokens in ONE pass on the many-row kernel (csrc/attn_prefill.hip);
  (b) ``n next_logits``: the only way before it, one eager step per given token;
and, for (b)'s best case, n x the captured per-token time of profiles/kbench_parti_sample*.log (a captured step cannot
be fed given tokens without a host write per step, so this is a floor for (b), not an arm).
The arms ALTERNATE round by round in one process after a warm-up round on the same decode state; per arm the median of
the rounds and the spread max - min (host wall time around a device synchronize: (b) is launch bound and the host is
part of what is measured).  Both arms end with the last row's logits and the same caches.

``--part kernel``: the attention launch alone, f32, (B 8, H 8, D 64), p0 = 0, n rows: amk_attn_prefill (VALU, the
decode kernel's chain per row, no mask tensor, fills the cache) against ops.attention_fused_kv with the byte causal
mask on the same q and kv (the MFMA tile kernels the training forward runs).  Eager launches, device time by events
over 20 calls per round; whichever way the ratio falls it is printed.
    python tools/kbench_parti_prefill.py [--part all|model|kernel] [--prefix 512,1023] [--rounds 3] [--batch 8]
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

from amk import ops  # noqa: E402
from amk.models import Parti  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["all", "model", "kernel"], default="all")
ap.add_argument("--prefix", default="512,1023")
ap.add_argument("--steps", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=8)
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
DIM, HEADS, D_HEAD, DEPTH, V, L = 512, 8, 64, 6, 8192, 77
B = a.batch
PREFIXES = [int(x) for x in a.prefix.split(",")]


def captured_ms():
    """{"f32", "bf16"}: ms per token of sample(graph=True) at this configuration, read from the two "graph" lines of
    profiles/kbench_parti_sample_bf16.log (both arms measured in one process), so the figures follow that log."""
    import re

    out = {}
    with open(os.path.join(ROOT, "profiles", "kbench_parti_sample_bf16.log")) as f:
        for line in f:
            m = re.match(r"\s*graph (f32|bf16): .*; ([0-9.]+) ms per token step", line)
            if m:
                out[m.group(1)] = float(m.group(2))
    if set(out) != {"f32", "bf16"}:
        raise RuntimeError("profiles/kbench_parti_sample_bf16.log holds no 'graph f32' / 'graph bf16' lines")
    return out


CAPTURED_MS = captured_ms()


def med_spread(xs):
    return statistics.median(xs), max(xs) - min(xs)


class StubVQ(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.codebook = types.SimpleNamespace(codebook_size=V)
        self.num_patches = a.steps

    def decode_indices(self, ids):
        return ids


def model_part():
    model = Parti(DIM, StubVQ(), None, None, L, HEADS, D_HEAD, DEPTH).to(dev).eval()
    text = torch.randn(B, L, DIM, device=dev)
    ids = torch.randint(0, V, (B, a.steps), device=dev)
    print(f"Parti prompt: batch {B}, capacity {a.steps}, {V} codes, {a.rounds} alternating rounds after one warm-up round; "
          f"spread = max - min of the rounds")
    for mode in ("f32", "bf16"):
        def ctx():
            return torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16")

        with ctx():
            state = model.begin_decode(text)
        for n in PREFIXES:
            def prefill():
                state.reset()
                return model.prefill(state, ids[:, :n])

            def steps():
                state.reset()
                lg = model.next_logits(state, None)
                for i in range(n):
                    lg = model.next_logits(state, ids[:, i])
                return lg

            arms = {"prefill": prefill, "n next_logits": steps}
            res, last = {k: [] for k in arms}, {}
            for r in range(a.rounds + 1):
                for k, fn in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with ctx():
                        last[k] = fn()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    assert state.host_pos == n + 1
                    if r:
                        res[k].append(dt)
            dev_abs = float((last["prefill"] - last["n next_logits"]).abs().max())
            med = {}
            line = [f"  {mode:>4} prefix {n:4d} ({n + 1} rows):"]
            for k in arms:
                med[k], sp = med_spread(res[k])
                line.append(f"{k} median {1e3 * med[k]:.2f} ms (spread {1e3 * sp:.2f})")
            floor = CAPTURED_MS[mode] * (n + 1)
            line.append(f"prefill is {med['n next_logits'] / med['prefill']:.1f}x the eager steps; n x the captured step "
                        f"({CAPTURED_MS[mode]} ms) = {floor:.1f} ms, {floor / (1e3 * med['prefill']):.1f}x the prefill; "
                        f"max |last-row logits, prefill - steps| {dev_abs:.2e}")
            print(line[0] + " " + "; ".join(line[1:]))
        ops.KERNEL_EVENTS = {}
        with ctx():
            state.reset()
            model.prefill(state, ids[:, :PREFIXES[-1]])
        torch.cuda.synchronize()
        for name, (cnt, ms) in sorted(ops.kernel_event_summary(ops.KERNEL_EVENTS).items()):
            print(f"    kernel events of one {mode} prefill of {PREFIXES[-1]} tokens: {name}: {cnt} launches, {1e3 * ms:.1f} us each")
        ops.KERNEL_EVENTS = None


def kernel_part():
    H, D, cap = HEADS, D_HEAD, a.steps
    scale = D ** -0.5
    print(f"the attention launch alone, f32: B {B}, H {H}, D {D}, p0 = 0, capacity {cap}; eager launches, device time by "
          f"events over 20 calls, {a.rounds} alternating rounds after three warm-up rounds, spread = max - min")
    for n in (512, 1023):
        q2 = torch.randn(B, n, H * D, device=dev)
        kv2 = torch.randn(B, n, 2 * H * D, device=dev)
        cache = torch.zeros(B, cap, 2 * H * D, device=dev)
        p0 = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.attention_prefill_ws_floats(B, H, D, cap, n), device=dev)
        mask = ops.causal_mask(n, n, dev)
        arms = {"attn_prefill (VALU)": lambda: ops.attention_prefill(q2, kv2, cache, p0, H, D, scale, ws=ws),
                "attention_fused_kv (MFMA tiles, byte mask)": lambda: ops.attention_fused_kv(q2, kv2, H, D, scale, causal_mask=mask)}
        with torch.no_grad():
            err = float((arms["attn_prefill (VALU)"]() - arms["attention_fused_kv (MFMA tiles, byte mask)"]()).abs().max())
            res = {k: [] for k in arms}
            for r in range(a.rounds + 3):
                for k, fn in arms.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(20):
                        fn()
                    t1.record()
                    torch.cuda.synchronize()
                    if r >= 3:
                        res[k].append(t0.elapsed_time(t1) * 1e3 / 20)
        med = {}
        line = [f"  n {n:4d} (max |prefill - fused_kv| {err:.1e}):"]
        for k in arms:
            med[k], sp = med_spread(res[k])
            line.append(f"{k} {med[k]:.1f} us (spread {sp:.1f})")
        ratio = med["attn_prefill (VALU)"] / med["attention_fused_kv (MFMA tiles, byte mask)"]
        line.append(f"prefill / fused_kv = {ratio:.2f}")
        print(line[0] + " " + "; ".join(line[1:]))
    print("  (the choice of the VALU form for the prefill rested on no measurement before this one)")


if a.part in ("all", "kernel"):
    kernel_part()
if a.part in ("all", "model"):
    model_part()
