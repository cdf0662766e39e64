"""Sampling from Parti at dim 512, 8 heads, d_head 64, depth 6, 8192 codes, 77 text positions, batch 8, stub tokenizer
(DESIGN.md section 4i), in tokens/s and ms per token:
  (a) ``generate``: the reference's loop, the whole prefix through the decoder at every step;
  (b) ``sample``: the KV-cached causal decode, eager;
  (c) ``sample(graph=True)``: the same with the step captured once and replayed.
The arms ALTERNATE round by round in one process after a warm-up round, so all see the same warm chip; per arm the median
of the rounds and the spread max - min (host wall time around a device synchronize: the loops are launch bound and the
host is part of what is measured).  ``--steps`` sets the tokens per sample for ALL arms (the tokenizer's num_patches and
with it the cache capacity); (a) grows with the square of it.

``--part kernel``: amk_attn_decode alone at (B 8, H 8, D 64), capacity 1024, n = 128 / 512 / 1024 valid rows (read
mode), against amk_attn_fwd with I = 1 on the same cache rows -- how the library computed one row before -- and against
a device copy of the same rows in the same run (bytes read by the kernel / time, as a fraction of the copy's bytes read /
time).  Every arm is 50 calls captured into one HIP graph and timed over 20 replays per round, so the figures are device
time per call, not the host's launch rate; the decode arm reuses one workspace, as DecoderState does.  The
keys per chunk are a build-time default that AMK_ATTN_DECODE_KEYS = 32 / 64 / 128 overrides, read once per process: run this part once per value to compare split counts (the line printed names the value in force).
    python tools/kbench_parti_sample.py [--part all|model|kernel] [--steps 1024] [--rounds 3] [--batch 8]

``--autocast bf16``: the decode under bf16 autocast against the f32 one (profiles/kbench_parti_sample_bf16.log):
  model   ``sample(graph=True)`` in f32 (the parent's arm) and under bf16 autocast on a bf16 decode state, on two modules
          with the same weights, ALTERNATING round by round in one process; the eager bf16 ``sample`` rides along.
  kernel  amk_attn_decode_bf16 alone at n = 128 / 512 / 1024 against amk_attn_decode on the same values in f32 and
          against a device copy of the same bf16 bytes, captured-replay timing as above.
  gemm    amk_gemm_rows_bf16 against F.linear on the same bf16 operands at M = batch for the step's weight shapes,
          captured-replay timing; a bf16 result, and f32 with the f32 bias for the head.
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
ap.add_argument("--part", choices=["all", "model", "kernel", "gemm"], default="all")
ap.add_argument("--autocast", choices=["none", "bf16"], default="none")
ap.add_argument("--steps", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--arms", default="generate,sample,graph")
a = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)
DIM, HEADS, D_HEAD, DEPTH, V, L = 512, 8, 64, 6, 8192, 77
B = a.batch


def med_spread(xs):
    return statistics.median(xs), max(xs) - min(xs)


def graphed(fn, launches=50):
    """`launches` calls of fn captured into one HIP graph: a replay is device time, free of the host's launch cost."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g, launches


def timed(graph, replays=20):
    g, launches = graph
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (replays * launches)   # us per call


def alternate(arms):
    """{arm: [us per call]} over a.rounds alternating rounds after three warm-up rounds."""
    with torch.no_grad():
        graphs = {k: graphed(fn) for k, fn in arms.items()}
        res = {k: [] for k in arms}
        for r in range(a.rounds + 3):
            for k in arms:
                us = timed(graphs[k])
                if r >= 3:
                    res[k].append(us)
    return res


def kernel_part_bf16():
    keys = os.environ.get("AMK_ATTN_DECODE_KEYS", "64 (default)")
    cap, H, D = 1024, HEADS, D_HEAD
    scale = D ** -0.5
    cache16 = torch.randn(B, cap, 2 * H * D, device=dev).to(torch.bfloat16)
    q16 = torch.randn(B, 1, H * D, device=dev).to(torch.bfloat16)
    cache32, q32 = cache16.float(), q16.float()
    sink = torch.empty_like(cache16)
    ws = torch.empty(ops.attention_decode_ws_floats(B, H, D, cap), device=dev)
    print(f"amk_attn_decode_bf16 alone: B {B}, H {H}, D {D}, capacity {cap}, keys per chunk {keys}, read mode; "
          f"{a.rounds} alternating rounds, spread = max - min")
    for n in (128, 512, 1024):
        n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
        arms = {
            "decode bf16": lambda: ops.attention_decode(q16, None, cache16, n_dev, H, D, scale, ws=ws),
            "decode f32": lambda: ops.attention_decode(q32, None, cache32, n_dev, H, D, scale, ws=ws),
            "copy bf16": lambda: sink[:, :n].copy_(cache16[:, :n]),
        }
        with torch.no_grad():
            err = float((arms["decode bf16"]().float() - arms["decode f32"]()).abs().max())
        res = alternate(arms)
        nbytes = B * n * 2 * H * D * 2
        line = [f"n {n:5d} ({nbytes / 1e6:.1f} MB of bf16 read, max |bf16 - f32 kernel| {err:.1e}):"]
        med = {}
        for k in arms:
            med[k], sp = med_spread(res[k])
            line.append(f"{k} {med[k]:.1f} us (spread {sp:.1f})")
        line.append(f"bf16 decode reads at {med['copy bf16'] / med['decode bf16']:.2f} of the copy's rate, "
                    f"{med['decode f32'] / med['decode bf16']:.2f}x the f32 kernel")
        print("  " + "; ".join(line))


def gemm_part_bf16():
    inner = int(DIM * 4 * 2 / 3)
    hd = HEADS * D_HEAD
    shapes = [("self q|kv", 3 * hd, DIM, False), ("W_o / cross q", DIM, hd, False), ("ffn 1", 2 * inner, DIM, False),
              ("ffn 2", DIM, inner, False), ("head (f32 out, bias)", V, DIM, True)]
    print(f"amk_gemm_rows_bf16 against F.linear on bf16, M = {B}; captured-replay us per call, {a.rounds} alternating "
          f"rounds, spread = max - min")
    for name, N, K, head in shapes:
        x = torch.randn(B, K, device=dev).to(torch.bfloat16)
        w = ops.empty_w16(N, K, dev)
        w.copy_(torch.randn(N, K, device=dev) * K ** -0.5)
        bias = torch.randn(N, device=dev) if head else None
        if K % 8:
            x = ops._rows_padded(x)   # rows at a stride of 8 elements, as the step hands them over
        if head:
            w32, b16 = w.float(), bias.to(torch.bfloat16)
            arms = {"rows": lambda: ops.linear_rows_bf16(x, w, bias, torch.float32),
                    "library bf16 + cast": lambda: torch.nn.functional.linear(x, w, b16).float(),
                    "library f32 master": lambda: torch.nn.functional.linear(x.float(), w32, bias)}
        else:
            arms = {"rows": lambda: ops.linear_rows_bf16(x, w), "library bf16": lambda: torch.nn.functional.linear(x, w)}
        res = alternate(arms)
        line = [f"{name:>22} N {N:5d} K {K:5d} ({N * K * 2 / 1e6:.2f} MB of W):"]
        med = {}
        for k in arms:
            med[k], sp = med_spread(res[k])
            line.append(f"{k} {med[k]:.1f} us (spread {sp:.1f})")
        best = min((v, k) for k, v in med.items() if k != "rows")
        line.append(f"rows / best library = {med['rows'] / best[0]:.2f}")
        print("  " + "; ".join(line))


def model_part_bf16():
    import copy

    class StubVQ(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.codebook = types.SimpleNamespace(codebook_size=V)
            self.num_patches = a.steps

        def decode_indices(self, ids):
            return ids

    m32 = Parti(DIM, StubVQ(), None, None, L, HEADS, D_HEAD, DEPTH).to(dev).eval()
    m16 = copy.deepcopy(m32)
    text = torch.randn(B, L, DIM, device=dev)

    def bf16(fn):
        def run():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return fn()
        return run

    arms = {"graph f32": lambda: m32.sample(text, graph=True), "graph bf16": bf16(lambda: m16.sample(text, graph=True)),
            "eager f32": lambda: m32.sample(text), "eager bf16": bf16(lambda: m16.sample(text))}
    print(f"Parti sampling, f32 against bf16 autocast: batch {B}, {a.steps} tokens per sample, {V} codes, {a.rounds} "
          f"alternating rounds after one warm-up round; spread = max - min of the rounds")
    res = {k: [] for k in arms}
    for r in range(a.rounds + 1):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert tuple(ids.shape) == (B, a.steps)
            if r:
                res[k].append(dt)
    for k in arms:
        m, sp = med_spread(res[k])
        print(f"  {k:>10}: median {m:.3f} s, spread {sp:.3f} s; {1e3 * m / a.steps:.3f} ms per token step, "
              f"{B * a.steps / m:.0f} tokens/s")
    print(f"  captures: f32 {m32.decode_graph_captures}, bf16 {m16.decode_graph_captures}")
    ops.KERNEL_EVENTS = {}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        state = m16.begin_decode(text)
        m16.next_logits(state, None)
        state.set_position(a.steps - 1)
        m16.next_logits(state, torch.zeros(B, dtype=torch.long, device=dev))
    torch.cuda.synchronize()
    for name, (n, ms) in sorted(ops.kernel_event_summary(ops.KERNEL_EVENTS).items()):
        print(f"  kernel events of the first and the last bf16 step: {name}: {n} launches, {1e3 * ms:.1f} us each")
    ops.KERNEL_EVENTS = None


def kernel_part():
    keys = os.environ.get("AMK_ATTN_DECODE_KEYS", "64 (default)")
    cap, H, D = 1024, HEADS, D_HEAD
    scale = D ** -0.5
    cache = torch.randn(B, cap, 2 * H * D, device=dev)
    q2 = torch.randn(B, 1, H * D, device=dev)
    sink = torch.empty_like(cache)
    print(f"amk_attn_decode alone: B {B}, H {H}, D {D}, capacity {cap}, keys per chunk {keys} "
          f"({-(-cap // int(keys.split()[0]))} chunks per (batch, head) at full length), read mode")

    def graphed(fn, launches=50):
        """`launches` calls of fn captured into one HIP graph: a replay is device time, free of the host's launch cost."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(launches):
                fn()
        return g, launches

    def timed(graph, replays=20):
        g, launches = graph
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(replays):
            g.replay()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / (replays * launches)   # us per call

    ws = torch.empty(ops.attention_decode_ws_floats(B, H, D, cap), device=dev)
    for n in (128, 512, 1024):
        n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
        kv = cache[:, :n].view(B, n, 2, H, D)
        q4 = q2.view(B, 1, H, D).permute(0, 2, 1, 3)
        k4, v4 = kv[:, :, 0].permute(0, 2, 1, 3), kv[:, :, 1].permute(0, 2, 1, 3)
        arms = {
            "decode": lambda: ops.attention_decode(q2, None, cache, n_dev, H, D, scale, ws=ws),
            "attn_fwd I=1": lambda: ops._attn_forward(q4, k4, v4, None, None, scale),
            "copy": lambda: sink[:, :n].copy_(cache[:, :n]),
        }
        with torch.no_grad():
            ref = ops._attn_forward(q4, k4, v4, None, None, scale)[3].permute(0, 2, 1, 3).reshape(B, 1, H * D)
            err = float((arms["decode"]() - ref).abs().max())
            graphs = {k: graphed(fn) for k, fn in arms.items()}
            res = {k: [] for k in arms}
            for r in range(a.rounds + 3):
                for k in arms:
                    us = timed(graphs[k])
                    if r:
                        res[k].append(us)
        nbytes = B * n * 2 * H * D * 4
        line = [f"n {n:5d} ({nbytes / 1e6:.1f} MB read, max |decode - attn_fwd| {err:.1e}):"]
        rate = {}
        for k in arms:
            m, sp = med_spread(res[k])
            rate[k] = nbytes / m / 1e3   # GB/s of bytes READ
            line.append(f"{k} {m:.1f} us (spread {sp:.1f}, {rate[k]:.0f} GB/s read)")
        line.append(f"decode = {rate['decode'] / rate['copy']:.2f} of the copy's rate, "
                    f"{statistics.median(res['attn_fwd I=1']) / statistics.median(res['decode']):.1f}x attn_fwd")
        print("  " + "; ".join(line))


def model_part():
    class StubVQ(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.codebook = types.SimpleNamespace(codebook_size=V)
            self.num_patches = a.steps

        def decode_indices(self, ids):
            return ids

    model = Parti(DIM, StubVQ(), None, None, L, HEADS, D_HEAD, DEPTH).to(dev).eval()
    text = torch.randn(B, L, DIM, device=dev)
    all_arms = {"generate": lambda: model.generate(text), "sample": lambda: model.sample(text),
                "graph": lambda: model.sample(text, graph=True)}
    arms = {k: all_arms[k] for k in a.arms.split(",")}
    print(f"Parti sampling: batch {B}, {a.steps} tokens per sample (all arms), {V} codes, {a.rounds} alternating rounds "
          f"after one warm-up round; spread = max - min of the rounds")
    res = {k: [] for k in arms}
    for r in range(a.rounds + 1):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert tuple(ids.shape) == (B, a.steps)
            if r:
                res[k].append(dt)
    for k in arms:
        m, sp = med_spread(res[k])
        print(f"  {k:>8}: median {m:.3f} s, spread {sp:.3f} s; {1e3 * m / a.steps:.3f} ms per token step, "
              f"{B * a.steps / m:.0f} tokens/s")
    if "sample" in arms:
        ops.KERNEL_EVENTS = {}
        state = model.begin_decode(text)
        model.next_logits(state, None)
        state.set_position(a.steps - 1)   # the last position: the longest key range
        model.next_logits(state, torch.zeros(B, dtype=torch.long, device=dev))
        torch.cuda.synchronize()
        for name, (n, ms) in sorted(ops.kernel_event_summary(ops.KERNEL_EVENTS).items()):
            print(f"  kernel events of the first and the last step: {name}: {n} launches, {1e3 * ms:.1f} us each")
        ops.KERNEL_EVENTS = None


if a.autocast == "bf16":
    if a.part in ("all", "kernel"):
        kernel_part_bf16()
    if a.part in ("all", "gemm"):
        gemm_part_bf16()
    if a.part in ("all", "model"):
        model_part_bf16()
else:
    if a.part in ("all", "kernel"):
        kernel_part()
    if a.part in ("all", "model"):
        model_part()
