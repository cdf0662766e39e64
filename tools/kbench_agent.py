"""AgentAttention module timings (B 2 = the BASELINE.md row, B 64 = the chip-filling case).

    python tools/kbench_agent.py [--iters 20] [--dim-head 32|64|128]
    python tools/kbench_agent.py --autocast bf16 [--rounds 5] [--iters 20] [--dim-head 32|64|128 ...] [--parent-lib libamk.so]

The core's forward and backward are also given as a fraction of the 8 TB/s HBM peak, with bench.py's agent_block
byte count (16 * B*h*T*d forward, 28 * B*h*T*d backward: scales with the head dim).

--autocast bf16: the bf16-element kernels (ops.AGENT_BF16 on) against the cast path (off: qkv upcast, the f32 kernels, o
and the gradients cast back) under torch.autocast(bfloat16), in one process: the two arms alternate within each of
--rounds rounds, every (arm, workload) is warmed before it is timed, and each arm reports min / median / spread
((max - min) / median) over the rounds; a difference counts when the arms' ranges do not overlap.  Workloads: core forward, core forward + backward, module forward + backward,
at B 2, 8 and 64 for each --dim-head.  Algorithmic bytes count 2 bytes for q, k, v, o (forward: 8 * B*h*T*d) and for q,
k, v, dO, dq, dk, dv (backward: 14 * B*h*T*d) in both arms -- what the values need -- so the off arm's share of the HBM
peak shows what its 4-byte kernels and four casts cost.  The outputs of the two arms are compared bit for bit first.
--parent-lib: the f32 entry points of this build against those of another build of libamk.so (the parent commit's) on
the same f32 tensors at the same three shapes (and at 16 agents per head): every output bit for bit, then alternating timings of forward + backward.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "attention-models_amd"))
sys.path.insert(0, ROOT)
from tools.kbench_moe import time_launches  # noqa: E402

HBM_PEAK_GBS = 8000.0
H, T = 6, 1024


def f32_rows(d, iters):
    from amk import ops
    from amk.models import AgentAttention

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ag = AgentAttention(384, 6, d).to(dev)
    for B in (2, 8, 64):
        x = torch.randn(B, 1024, 384, device=dev, requires_grad=True)
        cot = torch.randn(B, 1024, 384, device=dev)
        qkv = ag.qkv(x).detach().requires_grad_(True)
        cw, cb = ag.dwc[1].weight, ag.dwc[1].bias
        core = lambda: ops.agent_attention(qkv, cw, cb, 6, d, ag.pool_size, ag.scale)
        co = torch.randn(B, 1024, 6 * d, device=dev)

        def core_fb():
            core().backward(co)

        def fb():
            ag(x).backward(cot)
        t_c = time_launches(core, iters)
        t_cfb = time_launches(core_fb, iters)
        t_f = time_launches(lambda: ag(x), iters)
        t_fb = time_launches(fb, iters)
        unit = float(B * 6 * 1024 * d)
        byt_f, byt_b, t_cb = 16.0 * unit, 28.0 * unit, t_cfb - t_c   # q, k, v read + o written; q, k, v, dO read + dq, dk, dv written
        print(f"d {d:3d} B {B:3d}: core fwd {t_c*1e3:7.3f} ms ({byt_f/t_c/1e9:7.1f} GB/s algorithmic, {byt_f/t_c/1e9/HBM_PEAK_GBS:.3f} of HBM peak)"
              f"  core bwd {t_cb*1e3:7.3f} ms ({byt_b/t_cb/1e9/HBM_PEAK_GBS:.3f} of HBM peak)  core fwd+bwd {t_cfb*1e3:7.3f} ms"
              f" | module fwd {t_f*1e3:7.3f} ms  fwd+bwd {t_fb*1e3:7.3f} ms")


def _stats(ts):
    med = statistics.median(ts)
    return min(ts), med, (max(ts) - min(ts)) / med


def _bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def bf16_rows(d, iters, rounds):
    """Returns {B: (the slowest round of the on arm is faster than the fastest of the off arm, off / on of the medians)} of
    core forward + backward: the shipping rule of ops.AGENT_BF16."""
    from amk import ops
    from amk.models import AgentAttention

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ag = AgentAttention(384, H, d).to(dev)
    cw, cb = ag.dwc[1].weight, ag.dwc[1].bias
    verdict = {}
    for B in (2, 8, 64):
        x = torch.randn(B, T, 384, device=dev, requires_grad=True)
        cot = torch.randn(B, T, 384, device=dev)
        with torch.autocast("cuda", torch.bfloat16):
            qkv = ag.qkv(x).detach().requires_grad_(True)
        assert qkv.dtype == torch.bfloat16
        co = torch.randn(B, T, H * d, device=dev).to(torch.bfloat16)

        def core():
            with torch.autocast("cuda", torch.bfloat16):
                return ops.agent_attention(qkv, cw, cb, H, d, ag.pool_size, ag.scale)

        def core_fb():
            o = core()
            o.backward(co.to(o.dtype))

        def mod_fb():
            with torch.autocast("cuda", torch.bfloat16):
                y = ag(x)
            y.backward(cot.to(y.dtype))

        # the two arms compute the same bits (the cast path's o is rounded where W_o would round it)
        res = {}
        for on in (True, False):
            ops.AGENT_BF16 = on
            qkv.grad = cw.grad = cb.grad = None
            o = core()
            o.backward(co.to(o.dtype))
            res[on] = (o.detach().to(torch.bfloat16), qkv.grad.clone(), cw.grad.clone(), cb.grad.clone())
        same = all(_bits(a, b) for a, b in zip(res[True], res[False]))
        work = {"core fwd": core, "core fwd+bwd": core_fb, "module fwd+bwd": mod_fb}
        times = {(on, w): [] for on in (True, False) for w in work}
        for r in range(rounds):
            for on in ((True, False) if r % 2 == 0 else (False, True)):      # alternate, and alternate who goes first
                ops.AGENT_BF16 = on
                for w, fn in work.items():
                    times[(on, w)].append(time_launches(fn, iters, warm=max(3, iters // 2)))
        ops.AGENT_BF16 = True
        unit = float(B * H * T * d)
        nbytes = {"core fwd": 8.0 * unit, "core fwd+bwd": 22.0 * unit}
        print(f"d {d:3d} B {B:3d}: outputs of the two arms bitwise equal: {same}")
        for w in work:
            line = f"    {w:15s}"
            for on in (True, False):
                lo, med, spread = _stats(times[(on, w)])
                frac = f" {nbytes[w]/med/1e9/HBM_PEAK_GBS:.3f} of HBM peak" if w in nbytes else ""
                line += f" | {'bf16 kernels' if on else 'cast + f32  '} min {lo*1e3:7.3f} median {med*1e3:7.3f} ms spread {spread*100:4.1f} %{frac}"
            m1, m0 = _stats(times[(True, w)])[1], _stats(times[(False, w)])[1]
            apart = max(times[(True, w)]) < min(times[(False, w)])       # every round of the on arm beats every round of the off arm
            print(line + f" | off / on {m0/m1:.2f}x{'' if apart else ' (the arms overlap)'}")
            if w == "core fwd+bwd":
                verdict[B] = (apart, m0 / m1)
    return verdict


PARENT_SIGS = ("amk_agent_attn_fwd", "amk_agent_attn_bwd", "amk_agent_conv_grad_reduce", "amk_agent_ws_floats_dh",
               "amk_agent_num_chunks_dh")


def vs_parent(path, d, iters, rounds):
    """The f32 kernels against another build's: bits of every output, then alternating timings."""
    from amk import lib as L_

    dev = torch.device("cuda:0")
    libs = {"this": L_.load(), "parent": ctypes.CDLL(path)}
    for name in PARENT_SIGS:
        fn = getattr(libs["parent"], name)
        fn.restype, fn.argtypes = L_.SIGNATURES[name]
    scale = d ** -0.5
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(d)
    for B, P in ((2, H), (8, H), (64, H), (8, 16)):          # (the last row: the instantiations for more than 8 agents)
        qkv = torch.randn(B, T, 3, H, d, device=dev, generator=g)
        q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
        g_o = torch.randn(B, T, H, d, device=dev, generator=g).permute(0, 2, 1, 3)
        cw, cb = torch.randn(d, 1, 3, 3, device=dev, generator=g) / 3, torch.randn(d, device=dev, generator=g)
        s4 = lambda t: (t.stride(0), t.stride(2), t.stride(1))
        outs, calls = {}, {}
        for tag, L in libs.items():
            NC = L.amk_agent_num_chunks_dh(T, d)
            cells, rows = B * H * NC, B * H * P
            o = torch.empty(B, T, H, d, device=dev).permute(0, 2, 1, 3)
            dqkv = torch.empty_like(qkv)
            dq, dk, dv = (dqkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
            agents, vagent = torch.empty(rows * d, device=dev), torch.empty(rows * d, device=dev)
            stats1 = torch.empty(rows * 2, device=dev)
            wsf = torch.empty(L.amk_agent_ws_floats_dh(B, H, T, P, d, 0), device=dev)
            wsb = torch.empty(L.amk_agent_ws_floats_dh(B, H, T, P, d, 1), device=dev)
            dwp, dbp = torch.empty(cells * 9 * d, device=dev), torch.empty(cells * d, device=dev)
            dw, db = torch.empty(d * 9, device=dev), torch.empty(d, device=dev)

            def call(L=L, o=o, dq=dq, dk=dk, dv=dv, agents=agents, vagent=vagent, stats1=stats1, wsf=wsf, wsb=wsb, dwp=dwp,
                     dbp=dbp, dw=dw, db=db, cells=cells):
                rc = L.amk_agent_attn_fwd(ptr(q), ptr(k), ptr(v), ptr(cw), ptr(cb), ptr(o), ptr(agents), ptr(vagent), ptr(stats1),
                                          ptr(wsf), B, H, T, d, P, *s4(q), *s4(k), *s4(v), *s4(o), scale, st)
                rc |= L.amk_agent_attn_bwd(ptr(q), ptr(k), ptr(v), ptr(cw), ptr(g_o), ptr(agents), ptr(vagent), ptr(stats1),
                                           ptr(dq), ptr(dk), ptr(dv), ptr(wsb), ptr(dwp), ptr(dbp), B, H, T, d, P, *s4(q), *s4(k),
                                           *s4(v), *s4(g_o), *s4(dq), *s4(dk), *s4(dv), scale, st)
                rc |= L.amk_agent_conv_grad_reduce(ptr(dwp), ptr(dbp), cells, d, ptr(dw), ptr(db), st)
                assert rc == 0, rc
            call()
            torch.cuda.synchronize()
            outs[tag] = (o, dqkv, agents, vagent, stats1, dwp, dbp, dw, db)
            calls[tag] = call
        same = all(_bits(a, b) for a, b in zip(outs["this"], outs["parent"]))
        times = {tag: [] for tag in libs}
        for r in range(rounds):
            for tag in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
                times[tag].append(time_launches(calls[tag], iters, warm=max(3, iters // 2)))
        line = f"d {d:3d} B {B:3d} P {P:2d}: f32 fwd+bwd outputs bitwise equal to the parent build's: {same}"
        for tag in libs:
            lo, med, spread = _stats(times[tag])
            line += f" | {tag:6s} min {lo*1e3:7.3f} median {med*1e3:7.3f} ms spread {spread*100:4.1f} %"
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dim-head", type=int, nargs="+", default=[64], choices=[32, 64, 128])
    ap.add_argument("--autocast", choices=["bf16"], default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.autocast is None:
        for d in a.dim_head:
            f32_rows(d, a.iters)
        return
    print(f"AgentAttention(384, 6, d) at T 1024 under torch.autocast(bfloat16): ops.AGENT_BF16 on (bf16-element kernels) against "
          f"off (casts + f32 kernels); {a.rounds} rounds x {a.iters} calls per arm and workload, arms alternating")
    verdicts = {d: bf16_rows(d, a.iters, a.rounds) for d in a.dim_head}
    ok = all(v[B][0] for v in verdicts.values() for B in (8, 64))
    print("core fwd+bwd, off / on: " + "  ".join(f"d{d} B{B} {v[B][1]:.2f}x{'' if v[B][0] else ' (the arms overlap)'}"
                                                  for d, v in verdicts.items() for B in (2, 8, 64)))
    print(f"faster than the cast path by more than the arms' spreads (no round of one arm inside the other's range) at B 8 and "
          f"B 64 at every head dim measured: {ok}")
    if a.parent_lib:
        for d in a.dim_head:
            vs_parent(a.parent_lib, d, a.iters, a.rounds)


if __name__ == "__main__":
    main()
