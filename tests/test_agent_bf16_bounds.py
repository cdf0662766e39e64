"""tests/agent_bf16_ref.py without a GPU: the f32 emulation of the kernels' chain on bf16-valued inputs, its bf16
outputs rounded once, meets agent_ref's two tiers and the interval condition on every case of the grid, and its q stays
at or below agent_ref.Q_EMU (the 4 x limit keeps its meaning); each defect a bf16 path can have leaves the interval;
the size query equals its restatement; the two entry points refuse what include/amk.h documents before any launch."""
import ctypes

import pytest
import torch

import agent_bf16_ref as bref
import agent_ref as ref
from amk import lib as amk_lib

EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def one_thread():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)               # the f32 sums of the emulation in one order, whatever the machine
    yield
    torch.set_num_threads(threads)


def test_rne_is_torch_rne():
    """The exact fp64 rounding agrees with torch's f32 -> bf16 conversion on ties, binade edges and subnormals."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-130, 120, (4096,), generator=g).float())
    ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, 1.99609375, 2.0 ** -126 * 1.00390625, 2.0 ** -133 * 1.5, 0.0])
    x = torch.cat([x, ties])
    assert torch.equal(bref.bf16_round(x), x.to(torch.bfloat16).float())
    assert torch.equal(bref.bf16_trunc(ties).float(), (ties.view(torch.int32) & -65536).view(torch.float32))


def test_emulation(one_thread, capsys):
    """agent_ref.emulate on the bf16-valued inputs of every grid case, o / dq / dk / dv rounded once: the f32 outputs
    meet both tiers, every output's q is at most agent_ref.Q_EMU (or the value bref carries, which is then this
    emulation's), every rounded output lies in its interval."""
    worst = {}
    for c in bref.CASES:
        inp = bref.case_inputs(c)
        P, scale = c["P"], c["D"] ** -0.5
        for x in inp[:4]:
            assert torch.equal(x, x.to(torch.bfloat16).float())
        R = bref.reference(*inp, P, scale)
        E = ref.emulate(*inp, P, scale)
        for n in ref.OUTPUTS:
            assert bool(torch.isfinite(R[n]).all()), f"{c['id']}: the reference's {n} is not finite"
            nbad, ratio, q, _ = ref.measures(E[n], R, n)
            assert nbad == 0, f"{c['id']} {n}: the emulation misses the hard bound ({ratio:.3g}x)"
            worst[n] = max(worst.get(n, 0.0), q)
        for n in bref.F32_OUT:
            assert ref.violations(E[n], R, n) == 0, f"{c['id']} {n}"
        for n in bref.ROUNDED:
            nbad, pos = bref.outside(bref.bf16_round(E[n]), R, n)
            assert nbad == 0, f"{c['id']} {n}: {nbad} rounded elements of the emulation leave the interval"
    with capsys.disabled():
        print("\nemulation worst q on bf16-valued inputs:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    for n, q in worst.items():
        assert q <= bref.q_emu(n), f"{n}: the emulation's q {q:.4g} on bf16-valued inputs exceeds {bref.q_emu(n)}"
        assert (n in bref.Q_EMU_BF16) == (q > ref.Q_EMU[n]), f"{n}: q {q:.4g}, Q_EMU {ref.Q_EMU[n]}: an own value where it is needed, only there"
        if n in bref.Q_EMU_BF16:
            assert bref.Q_EMU_BF16[n] <= 1.25 * q, f"Q_EMU_BF16[{n}] = {bref.Q_EMU_BF16[n]} against the emulation's {q:.4g}"


# the grid's cases of up to three chunks: every head dim, both sides of P = 8, every family
SMALL = [c for c in bref.CASES if c["T"] <= 3 * ref.chunk_len(c["D"])]


def test_defect_emulation_is_the_emulation(one_thread):
    for c in SMALL[::5]:
        inp = bref.case_inputs(c)
        a, b = bref.emulate(*inp, c["P"], c["D"] ** -0.5), bref.emulate_defect(*inp, c["P"], c["D"] ** -0.5)
        for n in ref.OUTPUTS:
            assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), f"{c['id']} {n}"


@pytest.mark.parametrize("defect", bref.DEFECTS)
def test_planted_defects(one_thread, defect):
    """Each defect puts elements of a rounded output outside the interval on at least one case; without a defect the
    same cases pass (test_emulation)."""
    hit = {}
    for c in SMALL:
        inp = bref.case_inputs(c)
        P, scale = c["P"], c["D"] ** -0.5
        R = bref.reference(*inp, P, scale)
        E = bref.emulate_defect(*inp, P, scale, defect)
        n = sum(bref.outside(E[name], R, name)[0] for name in bref.ROUNDED)
        if n:
            hit[c["id"]] = n
    assert hit, f"{defect} goes unseen"
    print(defect, "seen on", len(hit), "of", len(SMALL), "cases")


def test_size_query_matches_restatement():
    L = amk_lib.load()
    for c in bref.CASES:
        B, H, T, D, P = (c[k] for k in "BHTDP")
        for backward in (0, 1):
            assert L.amk_agent_bf16_ws_floats(B, H, T, P, D, backward) == bref.ws_floats(B, H, T, P, D, backward)
        assert L.amk_agent_bf16_ws_floats(B, H, T, P, D, 0) == L.amk_agent_ws_floats_dh(B, H, T, P, D, 0)
        assert L.amk_agent_bf16_ws_floats(B, H, T, P, D, 1) == L.amk_agent_ws_floats_dh(B, H, T, P, D, 1) + B * H * T * D
    assert L.amk_agent_bf16_ws_floats(2, 2, 32, 2, 48, 1) == 0 and L.amk_agent_bf16_ws_floats(0, 2, 32, 2, 64, 1) == 0


def test_kernel_names_restated():
    assert bref.expected_kernels(64, 5) == {
        "agent_pool_bf16_kernel<64>", "agent_s1_partial_bf16_kernel<64,8>", "agent_s1_combine_kernel<64>", "agent_s2_bf16_kernel<64,8>",
        "agent_s2_bwd_stream_bf16_kernel<6>", "agent_mid_kernel<64>", "agent_s1_bwd_stream_bf16_kernel<6>",
        "agent_pool_bwd_bf16_kernel<64>", "agent_conv_reduce_kernel<64>"}
    assert "agent_s2_bwd_bf16_kernel<64,8>" in bref.expected_kernels(64, 5, "0")
    assert ref.kernel_id("void amk_agent::agent_s2_bwd_stream_bf16_kernel<6>(amk_agent::BwdParams)") == "agent_s2_bwd_stream_bf16_kernel<6>"


# ---------------------------------------------------------------------------------------------- refusals before any launch
def _fake():
    """A 16-byte-aligned non-null host address: it passes the argument checks and is never dereferenced."""
    buf = (ctypes.c_float * 128)()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def _call(which, addr, B=1, H=2, T=32, D=64, P=2, strides=None, bad_tensor=0, ptr=None, bad_ptr=0):
    """amk_agent_attn_bf16_fwd / _bwd with fake pointers; `strides` replaces the (sb, st, sh) of tensor `bad_tensor`,
    `ptr` pointer number `bad_ptr`.  (code, amk_last_error)."""
    L = amk_lib.load()
    nptr, nten = (10, 4) if which == "fwd" else (14, 7)
    ptrs = [ctypes.c_void_p(addr)] * nptr
    if ptr is not None:
        ptrs[bad_ptr] = ctypes.c_void_p(ptr)
    st = [[H * T * D, D, T * D] for _ in range(nten)]
    if strides is not None:
        st[bad_tensor] = list(strides)
    fn = L.amk_agent_attn_bf16_fwd if which == "fwd" else L.amk_agent_attn_bf16_bwd
    rc = fn(*ptrs, B, H, T, D, P, *[x for s in st for x in s], 0.125, ctypes.c_void_p(0))
    return rc, L.amk_last_error()


# the pointers of the bf16 tensors in the argument lists: q, k, v, o | q, k, v, d_o, dq, dk, dv
BF16_PTRS = {"fwd": (0, 1, 2, 5), "bwd": (0, 1, 2, 4, 8, 9, 10)}


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_refusals_before_any_launch(which):
    buf, addr = _fake()
    T, D, H = 32, 64, 2
    name = b"amk_agent_attn_bf16_" + which.encode()

    def refused(code, fragment, **kw):
        rc, msg = _call(which, addr, **kw)
        assert rc == code, (kw, rc, msg)
        assert name in msg and fragment in msg, (kw, msg)

    nptr, nten = (10, 4) if which == "fwd" else (14, 7)
    for i in range(nptr):
        refused(EINVAL, b"null pointer", ptr=0, bad_ptr=i)
    for kw in (dict(B=0), dict(H=0), dict(T=0), dict(P=0), dict(B=-1)):
        refused(EINVAL, b"non-positive size", **kw)
    for i in BF16_PTRS[which]:
        refused(EINVAL, b"16-byte aligned", ptr=addr + 8, bad_ptr=i)      # 8 bytes: what the f32 path's 4 floats need
        refused(EINVAL, b"16-byte aligned", ptr=addr + 2, bad_ptr=i)
    for t in range(nten):
        refused(EINVAL, b"multiples of 8", strides=[H * T * D + 4, D, T * D], bad_tensor=t)   # a multiple of 4 is not enough
        refused(EINVAL, b"multiples of 8", strides=[H * T * D, D + 4, T * D], bad_tensor=t)
        refused(EINVAL, b"multiples of 8", strides=[H * T * D, D, T * D + 1], bad_tensor=t)
        refused(EUNSUPPORTED, b"non-negative strides", strides=[H * T * D, -D, T * D], bad_tensor=t)
        refused(EUNSUPPORTED, b"non-negative strides", strides=[H * T * D, D, -T * D], bad_tensor=t)
        # a batch entry of 2 GiB or more, counted with 2-byte elements: from 2^30 elements on
        refused(EUNSUPPORTED, b"less than 2 GiB", strides=[1 << 40, ((1 << 30) // (T - 1) + 8) & ~7, D], bad_tensor=t)
        refused(EUNSUPPORTED, b"less than 2 GiB", strides=[1 << 40, 1 << 26, D], bad_tensor=t)
    for d in (48, 16, 256, 0):
        refused(EUNSUPPORTED, b"32, 64 or 128", D=d)
    refused(EUNSUPPORTED, b"17", P=17)
    refused(EUNSUPPORTED, b"5", T=4, P=5)
    big = dict(B=1 << 15, H=1 << 15, T=1 << 10) if which == "bwd" else dict(B=1 << 15, H=1 << 15, T=1 << 8, P=16)
    refused(EUNSUPPORTED, b"grid limit", **big)
