"""tests/agent_ref.py without a GPU: the fp64 reference is pinned to the CPU oracle the fixtures came from; the f32
emulation of the kernels' chain stays inside the hard bound of every element over every family and defines the tight
tier's Q_EMU (not too tight); planted kernel-style faults of that emulation are all flagged on diffuse inputs a few
chunks long (sensitive enough); the GPU sweep's case list reaches every kernel instantiation and every edge; the host
code refuses what it documents before any launch and sizes its workspaces as the restatement does."""
import ctypes

import pytest
import torch

import agent_ref as ref
import test_agent_bounds_gpu as sweep          # imports without a GPU: the case list is plain data
from amk import lib as amk_lib
from oracle import ref_cpu

EINVAL, EUNSUPPORTED = -1, -2
# (D, B, H, T, P): a few chunks with overlapping bins; nine agents over three heads; MAXP with short bins
SHAPES = [(64, 2, 2, 300, 6), (32, 2, 3, 140, 9), (128, 1, 2, 130, 16)]


@pytest.mark.parametrize("D", [32, 64, 128])
def test_reference_pinned_to_oracle(D):
    """At H == P the reference is the core of oracle.ref_cpu.agent_attention (identity projections, zero biases), in
    fp64 on both sides: o and every gradient, to 1e-12 (the oracle pools and multiplies in another order)."""
    B, h, T = 2, 3, 151
    q, k, v, g, cw, cb = ref.make_inputs("diffuse", B, h, T, D, h, D ** -0.5, 5)
    R = ref.reference(q, k, v, g, cw, cb, h, D ** -0.5)
    bthd = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, h * D)
    x = torch.cat([bthd(q), bthd(k), bthd(v)], -1).double().requires_grad_(True)
    w = {"qkv.weight": torch.eye(3 * h * D, dtype=torch.float64), "W_o.weight": torch.eye(h * D, dtype=torch.float64),
         "W_o.bias": torch.zeros(h * D, dtype=torch.float64), "bias1": torch.zeros(1, dtype=torch.float64),
         "bias2": torch.zeros(1, dtype=torch.float64), "dwc.1.weight": cw.double().requires_grad_(True),
         "dwc.1.bias": cb.double().requires_grad_(True)}
    out = ref_cpu.agent_attention(x, w, h, D, h * h)
    gx, gw, gb = torch.autograd.grad(out, [x, w["dwc.1.weight"], w["dwc.1.bias"]], bthd(g).double())
    close = lambda a, b: bool(((a - b).abs() <= 1e-12 * (1 + b.abs())).all())
    assert close(out, bthd(R["o"]))
    assert close(gx, torch.cat([bthd(R["dq"]), bthd(R["dk"]), bthd(R["dv"])], -1))
    assert close(gw, R["dconv_w"]) and close(gb, R["dconv_b"])


def _emulation_cases():
    for c in sweep.CASES:
        yield c["id"], sweep.case_inputs(c), c["P"], c["D"] ** -0.5
    for (D, B, H, T, P) in SHAPES:
        for fam in ref.FAMILIES:
            yield f"{fam} d{D} T{T} P{P}", ref.make_inputs(fam, B, H, T, D, P, D ** -0.5, 9), P, D ** -0.5


def test_emulation_defines_q(capsys):
    """Over the inputs of every case of the GPU sweep and every family at SHAPES: the reference is finite, the f32
    emulation is inside the hard bound of every element, and Q_EMU is its worst q per output, rounded up by at most a
    quarter: the tight tier's measure is this emulation, never the kernel."""
    worst = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)               # the f32 sums of the emulation in one order, whatever the machine
    try:
        for what, inp, P, scale in _emulation_cases():
            R = ref.reference(*inp, P, scale)
            E = ref.emulate(*inp, P, scale)
            for n in ref.OUTPUTS:
                assert bool(torch.isfinite(R[n]).all()), f"{what}: the reference's {n} is not finite"
                nbad, ratio, q, _ = ref.measures(E[n], R, n)
                assert nbad == 0, f"{what} {n}: the emulation misses the hard bound ({ratio:.3g}x)"
                worst[n] = max(worst.get(n, 0.0), q)
    finally:
        torch.set_num_threads(threads)
    with capsys.disabled():
        print("\nemulation worst q:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    for n, q in worst.items():
        assert q <= ref.Q_EMU[n] <= 1.25 * q, f"Q_EMU[{n}] = {ref.Q_EMU[n]} against the emulation's {q:.4g}"


@pytest.mark.parametrize("mut", ref.MUTATIONS)
def test_mutations_flagged(mut):
    """Each planted fault is flagged by the per-element check on diffuse inputs three chunks long (the combine's
    second pass: 65 chunks, the last of one token -- one key in 4097 goes missing); the same inputs without a fault pass."""
    D, B, H, T, P = 64, 2, 3, 300, (16 if mut == "p16_last_ignored" else 7)
    if mut == "second_pass_dropped":
        D, B, H, T, P = 128, 1, 1, 4097, 16
    inp = ref.make_inputs("diffuse", B, H, T, D, P, D ** -0.5, 3)
    R = ref.reference(*inp, P, D ** -0.5)
    clean, bad = ref.emulate(*inp, P, D ** -0.5), ref.emulate(*inp, P, D ** -0.5, mut=mut)
    assert sum(ref.violations(clean[n], R, n) for n in ref.OUTPUTS) == 0
    hit = {n: ref.violations(bad[n], R, n) for n in ref.OUTPUTS}
    assert any(hit.values()), f"{mut} goes unseen"


def test_paths_cover_dispatch():
    """From expected_kernels and features: the GPU sweep reaches every instantiation and every edge at least once."""
    kernels, feats, per_d = set(), set(), {}
    for c in sweep.CASES:
        kernels |= sweep.case_kernels(c)
        f = ref.features(c)
        feats |= f
        per_d.setdefault(c["D"], set()).update(f)
    assert not ref.all_instantiations() - kernels, sorted(ref.all_instantiations() - kernels)
    named = {f"{k}<{D},{pm}>" for D in (32, 64, 128) for pm in (8, 16)
             for k in ("agent_s1_partial_kernel", "agent_s2_kernel", "agent_s2_bwd_kernel", "agent_s1_bwd_kernel")}
    named |= {f"agent_s{s}_bwd_stream_kernel<{w}>" for s in (1, 2) for w in (4, 6, 8)}
    assert named <= kernels and named <= ref.all_instantiations()
    assert not set(ref.FEATURES) - feats, sorted(set(ref.FEATURES) - feats)
    for D, f in per_d.items():       # the edges of the chunking at every head dim
        assert {"NC > 64", "last chunk of one token", "exactly full last chunk", "T < chunk", "P == 16", "P == T",
                "bin crosses a 64-token block"} <= f, (D, sorted(f))
    assert any(c["D"] == 64 and c["P"] == 5 and "agent_s2_bwd_stream_kernel<6>" in sweep.case_kernels(c) for c in sweep.CASES)
    # the restatement itself: the width of the streaming forms, the <8 | 16> split, the environment switch
    assert "agent_s1_bwd_stream_kernel<4>" in ref.expected_kernels(64, 4) and "agent_s1_bwd_stream_kernel<6>" in ref.expected_kernels(64, 5)
    assert "agent_s1_bwd_stream_kernel<8>" in ref.expected_kernels(64, 7) and "agent_s1_bwd_kernel<64,16>" in ref.expected_kernels(64, 9)
    assert "agent_s2_bwd_kernel<64,8>" in ref.expected_kernels(64, 8, "0") and "agent_s2_bwd_stream_kernel<8>" in ref.expected_kernels(64, 8, "1")
    assert "agent_s2_bwd_kernel<64,8>" in ref.expected_kernels(64, 8, "") and "agent_s2_bwd_kernel<32,8>" in ref.expected_kernels(32, 3)
    assert ref.kernel_id("void amk_agent::agent_s2_kernel<64, 8>(amk_agent::Params)") == "agent_s2_kernel<64,8>"
    assert ref.kernel_id("_ZN9amk_agent26agent_s1_bwd_stream_kernelILi6EEEvNS_9BwdParamsE") == "agent_s1_bwd_stream_kernel<6>"
    assert ref.kernel_id("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float> >") is None


def test_size_queries_match_restatement():
    L = amk_lib.load()
    for c in sweep.CASES:
        B, H, T, D, P = (c[k] for k in "BHTDP")
        assert L.amk_agent_num_chunks_dh(T, D) == ref.num_chunks(T, D)
        for backward in (0, 1):
            assert L.amk_agent_ws_floats_dh(B, H, T, P, D, backward) == ref.ws_floats(B, H, T, P, D, backward)


# ---------------------------------------------------------------------------------------------- refusals before any launch
def _fake():
    """A 16-byte-aligned non-null host address: it passes the argument checks and is never dereferenced."""
    buf = (ctypes.c_float * 128)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _call(which, addr, B=1, H=2, T=32, D=64, P=2, strides=None, first=None, bad_tensor=0):
    """amk_agent_attn_fwd / _bwd with fake pointers; `strides` replaces the (sb, st, sh) of tensor `bad_tensor`,
    `first` the first pointer."""
    L = amk_lib.load()
    nptr, nten = (10, 4) if which == "fwd" else (14, 7)
    ptrs = [ctypes.c_void_p(addr)] * nptr
    if first is not None:
        ptrs[0] = ctypes.c_void_p(first)
    st = [[H * T * D, D, T * D] for _ in range(nten)]
    if strides is not None:
        st[bad_tensor] = list(strides)
    fn = L.amk_agent_attn_fwd if which == "fwd" else L.amk_agent_attn_bwd
    return fn(*ptrs, B, H, T, D, P, *[x for s in st for x in s], 0.125, ctypes.c_void_p(0))


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_refusals_before_any_launch(which):
    buf, addr = _fake()
    T, D, H = 32, 64, 2
    assert _call(which, addr, P=17) == EUNSUPPORTED
    assert _call(which, addr, T=4, P=5) == EUNSUPPORTED
    assert _call(which, addr, D=48) == EUNSUPPORTED
    last = 3 if which == "fwd" else 6
    for t in (0, last):
        assert _call(which, addr, strides=[H * T * D + 2, D, T * D], bad_tensor=t) == EINVAL       # a stride not a multiple of 4
        assert _call(which, addr, strides=[H * T * D, D + 1, T * D], bad_tensor=t) == EINVAL
        assert _call(which, addr, strides=[H * T * D, -D, T * D], bad_tensor=t) == EUNSUPPORTED     # a negative stride
        assert _call(which, addr, strides=[H * T * D, D, -T * D], bad_tensor=t) == EUNSUPPORTED
        assert _call(which, addr, strides=[1 << 40, 1 << 25, D], bad_tensor=t) == EUNSUPPORTED      # a batch entry of 2 GiB or more
    assert _call(which, addr, first=addr + 4) == EINVAL                                             # not 16-byte aligned
    assert _call(which, addr, first=0) == EINVAL
    assert _call(which, addr, B=0) == EINVAL
    assert b"amk_agent_attn_" + which.encode() in amk_lib.load().amk_last_error()


def test_conv_grad_reduce_refusals():
    L = amk_lib.load()
    buf, addr = _fake()
    p, null = ctypes.c_void_p(addr), ctypes.c_void_p(0)
    assert L.amk_agent_conv_grad_reduce(p, p, 0, 64, p, p, null) == EINVAL
    assert L.amk_agent_conv_grad_reduce(p, p, -3, 64, p, p, null) == EINVAL
    assert L.amk_agent_conv_grad_reduce(p, p, 4, 48, p, p, null) == EUNSUPPORTED
    assert L.amk_agent_conv_grad_reduce(ctypes.c_void_p(addr + 4), p, 4, 64, p, p, null) == EINVAL
    assert L.amk_agent_conv_grad_reduce(null, p, 4, 64, p, p, null) == EINVAL
