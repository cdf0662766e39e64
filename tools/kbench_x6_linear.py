"""Every Linear product of the ViT-VQGAN train step (batch 32: M = 32768 rows) on the exact-f32 path as amk.ops dispatches
it today against the split-bf16 forms on cached planes (csrc/gemm_x6.hip; planes made once, outside the timing, by the
table-driven split the optimizer runs once per step), fused forms included.  The two sides are interleaved in one process
for several rounds with an untimed pass in front of each timed one (tools/kbench_steady.py's rule); the last round is
reported, with the error of both against fp64 (max |c - c64| / max |c64|, on the first 2048 rows) and the cost of the
split itself.  Then the five weight gradients (dWq | dWkv as one launch, dWo, dW12, dW3, each with its bias sums) on
dense.gemm_tn (exact f32) against dense.gemm_x6_tn (csrc/gemm_x6_tn.hip, both operands split inside the kernel), the same
way, their error against fp64 over the whole gradient (AMK_X6_TN_TK=128 | 256 forces that kernel's tile width).
--only short_k: the three forward products with K = 256 (the gate with and without (a | b), q | kv) on the tile kernel
against the row-block-stationary one (amk_gemm_x6_short_k off / on), the two arms alternating in one process for five
rounds: medians and spreads, after a check that the two arms agree bit for bit.
    python tools/kbench_x6_linear.py [--batch 32] [--iters 20] [--rounds 3] [--only all|fwd|dw|short_k]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))

import torch  # noqa: E402

from bench import time_launches  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=("all", "fwd", "dw", "short_k"), default="all",
                    help="fwd: the nine forward / input-gradient rows; dw: the weight gradients; short_k: tile kernel against short-K kernel")
    a = ap.parse_args()
    from amk import dense, ops, tuning

    tuning.enable_gemm_tuning()
    dev = torch.device("cuda:0")
    M, Dm, Hh, Hf = a.batch * 1024, 256, 512, 1368
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    W = {"q": r(Hh, Dm) * Dm ** -0.5, "kv": r(2 * Hh, Dm) * Dm ** -0.5, "wo": r(Dm, Hh) * Hh ** -0.5,
         "w12": r(2 * Hf, Dm) * Dm ** -0.5, "w3": r(Dm, Hf) * Hf ** -0.5}
    names = list(W)
    ent, off = [], 0
    for n in names:
        ent.append((off, W[n].shape[0], W[n].shape[1], n == "w12"))
        off += -(-W[n].numel() // 256) * 256
    flat = torch.zeros(off, device=dev)
    for (o, R, K, _), n in zip(ent, names):
        flat[o:o + R * K] = W[n].reshape(-1).to(dev)
    W = {n: flat[o:o + R * K].view(R, K) for (o, R, K, _), n in zip(ent, names)}
    table, nblk, elems, spans = dense.x6_split_plan(ent)
    table = table.to(dev)
    buf = torch.zeros(elems, device=dev, dtype=torch.bfloat16)
    dense.x6_split_table(flat, table, nblk, buf)
    P = {n: dense.X6Planes(buf[dw:dw + nw], buf[dt:dt + nt], gt, R, K) for (_, R, K, gt), (dw, nw, dt, nt), n in zip(ent, spans, names)}
    t_split = time_launches(lambda: dense.x6_split_table(flat, table, nblk, buf), a.iters, warm=a.iters)
    print(f"table-driven split of one layer's five weights ({flat.numel() * 4 / 1e6:.2f} MB f32 -> {elems * 2 / 1e6:.2f} MB of planes): "
          f"{t_split * 1e6:.1f} us per launch", flush=True)

    x = r(M, Dm).to(dev)
    att = r(M, Hh).to(dev)
    dq, dkv = r(M, Hh).to(dev), r(M, 2 * Hh).to(dev)
    dout = r(M, Dm).to(dev)
    b12, b3, bo = r(2 * Hf).to(dev), r(Dm).to(dev), r(Dm).to(dev)
    gate, ab = dense.gemm_nt_swiglu(x, W["w12"], b12)
    d_ab = dense.gemm_nn(dout, W["w3"], swiglu_ab=ab)
    lin = torch.nn.functional.linear

    def ffn_ref(xx):
        p, q_ = lin(xx, W["w12"].double(), b12.double()).chunk(2, -1)
        return torch.nn.functional.silu(p) * q_

    def dab_ref(dd, abb):
        H = abb.shape[1] // 2
        p, q_ = abb[:, :H], abb[:, H:]
        s = torch.sigmoid(p)
        dg = dd @ W["w3"].double()
        return torch.cat([dg * q_ * s * (1 + p * (1 - s)), dg * p * s], 1)

    R_ = slice(0, 2048)   # rows of the fp64 check
    # (name, flop, f32 path as dispatched today, x6 form on the cached planes, fp64 reference of the checked rows)
    cases = [
        ("q | kv forward (one f32 launch, two x6)", 2.0 * M * Dm * 3 * Hh,
         lambda: dense.gemm_nt(x, W["q"], None, w2=W["kv"])[1],
         lambda: (dense.gemm_x6_nt(x, P["q"].w, Hh), dense.gemm_x6_nt(x, P["kv"].w, 2 * Hh))[1],
         lambda: x[R_].double() @ W["kv"].double().t()),
        ("W_o forward + bias", 2.0 * M * Dm * Hh,
         lambda: lin(att, W["wo"], bo), lambda: dense.gemm_x6_nt(att, P["wo"].w, Dm, bo),
         lambda: lin(att[R_].double(), W["wo"].double(), bo.double())),
        ("w12 + SwiGLU gate, (a | b) kept", 2.0 * M * Dm * 2 * Hf,
         lambda: dense.gemm_nt_swiglu(x, W["w12"], b12, keep_ab=True)[0],
         lambda: dense.gemm_x6_nt_swiglu(x, P["w12"].w, Hf, b12, keep_ab=True)[0], lambda: ffn_ref(x[R_].double())),
        ("w12 + SwiGLU gate, gate only", 2.0 * M * Dm * 2 * Hf,
         lambda: dense.gemm_nt_swiglu(x, W["w12"], b12, keep_ab=False)[0],
         lambda: dense.gemm_x6_nt_swiglu(x, P["w12"].w, Hf, b12, keep_ab=False)[0], lambda: ffn_ref(x[R_].double())),
        ("w3 forward + bias", 2.0 * M * Dm * Hf,
         lambda: lin(gate, W["w3"], b3), lambda: dense.gemm_x6_nt(gate, P["w3"].w, Dm, b3),
         lambda: lin(gate[R_].double(), W["w3"].double(), b3.double())),
        ("dX of q | kv (two segments)", 2.0 * M * Dm * 3 * Hh,
         lambda: dense.gemm_nn(dq, W["q"], a2=dkv, w2=W["kv"]),
         lambda: dense.gemm_x6_nt(dq, P["q"].wt, Dm, a2=dkv, planes2=P["kv"].wt),
         lambda: dq[R_].double() @ W["q"].double() + dkv[R_].double() @ W["kv"].double()),
        ("dX of W_o", 2.0 * M * Dm * Hh,
         lambda: ops._nn_plain(dout, W["wo"]), lambda: dense.gemm_x6_nt(dout, P["wo"].wt, Hh),
         lambda: dout[R_].double() @ W["wo"].double()),
        ("dGate = dY W3 + SwiGLU backward", 2.0 * M * Dm * Hf,
         lambda: dense.gemm_nn(dout, W["w3"], swiglu_ab=ab), lambda: dense.gemm_x6_nt_swiglu_bwd(dout, P["w3"].wt, ab),
         lambda: dab_ref(dout[R_].double(), ab[R_].double())),
        ("dX of w12", 2.0 * M * Dm * 2 * Hf,
         lambda: ops._nn_plain(d_ab, W["w12"]), lambda: dense.gemm_x6_nt(d_ab, P["w12"].wt, Dm),
         lambda: d_ab[R_].double() @ W["w12"].double()),
    ]
    if a.only == "short_k":
        import statistics

        from amk import lib

        L = lib.load()
        rows = [("w12 + SwiGLU gate, (a | b) kept", 2.0 * M * Dm * 2 * Hf, lambda: dense.gemm_x6_nt_swiglu(x, P["w12"].w, Hf, b12, keep_ab=True)),
                ("w12 + SwiGLU gate, gate only", 2.0 * M * Dm * 2 * Hf, lambda: dense.gemm_x6_nt_swiglu(x, P["w12"].w, Hf, b12, keep_ab=False)[:1]),
                ("q | kv forward (two launches | one)", 2.0 * M * Dm * 3 * Hh, lambda: dense.gemm_x6_nt_cols2(x, P["q"].w, Hh, P["kv"].w, 2 * Hh))]
        for name, fl, fn in rows:
            outs = []
            for on in (0, 1):
                L.amk_gemm_x6_short_k(on)
                outs.append(fn())
            same = all(torch.equal(u, v) for u, v in zip(*outs))
            del outs
            ts = {0: [], 1: []}
            for rnd in range(5):
                for on in (0, 1):
                    L.amk_gemm_x6_short_k(on)
                    ts[on].append(time_launches(fn, a.iters, warm=a.iters) * 1e6)
            L.amk_gemm_x6_short_k(1)
            m0, m1 = statistics.median(ts[0]), statistics.median(ts[1])
            print(f"{name:38s} tile kernel {m0:7.1f} us [{min(ts[0]):.1f} .. {max(ts[0]):.1f}] {fl / m0 / 1e6:6.1f} TF/s | short-K {m1:7.1f} us "
                  f"[{min(ts[1]):.1f} .. {max(ts[1]):.1f}] {fl / m1 / 1e6:6.1f} TF/s | x{m0 / m1:.2f} | bit-equal {same}", flush=True)
        sys.exit(0)
    tot = [0.0, 0.0]
    for name, fl, f32, x6, ref in (cases if a.only != "dw" else []):
        want = ref()
        errs = [float((fn()[R_].double() - want).abs().max() / want.abs().max()) for fn in (f32, x6)]
        for rnd in range(a.rounds):
            ts = [time_launches(fn, a.iters, warm=a.iters) for fn in (f32, x6)]
        tot[0] += ts[0]
        tot[1] += ts[1]
        print(f"{name:42s} f32 {ts[0] * 1e6:7.1f} us {fl / ts[0] / 1e12:6.1f} TF/s err {errs[0]:.1e} | x6 {ts[1] * 1e6:7.1f} us "
              f"{fl / ts[1] / 1e12:6.1f} TF/s err {errs[1]:.1e} | x{ts[0] / ts[1]:.2f}", flush=True)
    if a.only != "dw":
        print(f"sum over the nine products (the gate counted in both forms): f32 {tot[0] * 1e3:.3f} ms, x6 {tot[1] * 1e3:.3f} ms")
    if a.only == "fwd":
        sys.exit(0)

    # ---- the weight gradients: (name, (y, y2 or None), x); every launch takes its bias sums along, as the step's do
    dws = [("dWq | dWkv (512 | 1024 x 256, one launch)", (dq, dkv), x), ("dWo (256 x 512)", (dout, None), att),
           ("dW12 (2736 x 256)", (d_ab, None), x), ("dW3 (256 x 1368)", (dout, None), gate)]
    tot = [0.0, 0.0]
    for name, (y, y2), xx in dws:
        fns = [lambda tn=tn: tn(y, xx, y2=y2, want_bias=True) for tn in (dense.gemm_tn, dense.gemm_x6_tn)]
        want = (torch.cat([y, y2], 1) if y2 is not None else y).double().t() @ xx.double()
        errs = []
        for fn in fns:
            dw, dw2, _ = fn()
            got = torch.cat([dw, dw2], 0) if dw2 is not None else dw
            errs.append(float((got.double() - want).abs().max() / want.abs().max()))
        del want
        fl = 2.0 * M * (y.shape[1] + (y2.shape[1] if y2 is not None else 0)) * xx.shape[1]
        for rnd in range(a.rounds):
            ts = [time_launches(fn, a.iters, warm=a.iters) for fn in fns]
        tot[0] += ts[0]
        tot[1] += ts[1]
        print(f"{name:42s} f32 {ts[0] * 1e6:7.1f} us {fl / ts[0] / 1e12:6.1f} TF/s err {errs[0]:.1e} | x6 {ts[1] * 1e6:7.1f} us "
              f"{fl / ts[1] / 1e12:6.1f} TF/s err {errs[1]:.1e} | x{ts[0] / ts[1]:.2f}", flush=True)
    print(f"sum over the four weight-gradient launches of a layer: f32 {tot[0] * 1e3:.3f} ms, x6 {tot[1] * 1e3:.3f} ms")
