"""The bf16 attention kernels (csrc/attn_bf16.hip) held element by element to the error bound of
tests/bf16_attention_ref.py: o, dq, dk and dv against the fp64 reference on the bf16 values, at the tile edges (128
queries per forward workgroup over 64-key tiles, 256 keys per backward workgroup over 32-query tiles), under every mask
kind, on diffuse, peaked, needle, large-score and climbing-maximum inputs, at three scales.  Plus what a tolerance cannot
see: batch and head invariance and run-to-run reproducibility (bitwise), the C ABI with separate tensors, padded strides
and views into wider buffers (bitwise against the ops path), its argument refusals, and which kernels autocast picks.

AMK_BF16_BOUND_REPORT=<file>: write the worst |got - ref| / bound per tensor over this module to that JSON file."""
import ctypes
import json
import os
import random

import pytest
import torch

import bf16_attention_ref as ref
from oracle import ref_cpu
from util import assert_close

pytestmark = pytest.mark.gpu
D = 64
SC = D ** -0.5
AMK_EINVAL, AMK_EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AMK_BF16_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(ref.WORST, f, indent=1)


def _fused(q, k, v):
    """(B,H,T,64) -> q2 (B,I,H*64), kv2 (B,J,2*H*64) as the projections lay them out."""
    B, H, I, _ = q.shape
    J = k.shape[2]
    q2 = q.permute(0, 2, 1, 3).reshape(B, I, H * D)
    kv2 = torch.stack([k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)], dim=2).reshape(B, J, 2 * H * D)
    return q2, kv2


def _run_ops(device, q, k, v, d_o, scale, km=None, cm=None):
    """ops.attention_fused_kv forward + backward on bf16 copies; asserts the bf16 kernels ran.  -> {name: (B,H,T,64)}"""
    from amk import ops

    B, H, I, _ = q.shape
    J = k.shape[2]
    q2, kv2 = (t.bfloat16().to(device).requires_grad_(True) for t in _fused(q, k, v))
    cot = d_o.permute(0, 2, 1, 3).reshape(B, I, H * D).bfloat16().to(device)
    ops.KERNEL_EVENTS = {}
    try:
        o2 = ops.attention_fused_kv(q2, kv2, H, D, scale, key_mask=None if km is None else km.to(device),
                                    causal_mask=None if cm is None else cm.to(device))
        dq2, dkv2 = torch.autograd.grad((o2.float() * cot.float()).sum(), [q2, kv2])
        torch.cuda.synchronize()
        names = set(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    sfx = "<masked>" if km is not None or cm is not None else ""
    assert names == {"attn_bf16_fwd_kernel" + sfx, "attn_bf16_bwd_kernel" + sfx}, names
    assert o2.dtype == dq2.dtype == dkv2.dtype == torch.bfloat16
    dkv = dkv2.view(B, J, 2, H, D)
    return {"o": o2.view(B, I, H, D).permute(0, 2, 1, 3), "dq": dq2.view(B, I, H, D).permute(0, 2, 1, 3),
            "dk": dkv[:, :, 0].permute(0, 2, 1, 3), "dv": dkv[:, :, 1].permute(0, 2, 1, 3)}


def _check(device, family, mask, B, H, I, J, scale, seed):
    q, k, v, d_o = ref.make_inputs(family, B, H, I, J, scale, seed)
    km, cm = ref.make_masks(mask, B, I, J, seed)
    got = _run_ops(device, q, k, v, d_o, scale, km, cm)
    R = ref.reference(q, k, v, d_o, scale, km, cm)
    ref.assert_within(got, R, f"{family}/{mask}/B{B}H{H}I{I}J{J}/scale {scale:g}")
    return q, k, v, d_o, km, cm, got, R


# ---------------------------------------------------------------------------------------------- shape sweep
SWEEP_I = (1, 31, 32, 33, 127, 128, 129, 257)
SWEEP_J = (1, 63, 64, 65, 255, 256, 257, 513, 1024)


def _sweep_cases():
    """Every I and every J of the tile edges at least once (18 cases), each with a seeded head count, batch, input
    family, mask and scale."""
    rng = random.Random(20261016)
    Is, Js = list(SWEEP_I) * 3, list(SWEEP_J) * 2
    rng.shuffle(Is)
    rng.shuffle(Js)
    out = []
    for n in range(18):
        I, J = Is[n], Js[n]
        H = rng.choice([1, 3, 8, 16])
        B = rng.choice([1, 2, 3])
        while B * H * I * J > 3 * 2 ** 20 and (H > 1 or B > 1):   # (the fp64 reference of one case stays ~1 s)
            H, B = (H // 2, B) if H > 1 else (H, B - 1)
        fam = ref.FAMILIES[n % len(ref.FAMILIES)]
        mask = ("none", "key", "causal", "both", "triu", "dead_rows")[n % 6]
        scale = (SC, 1.0, 0.05)[n % 3]
        out.append((n, B, H, I, J, fam, mask, scale))
    assert {c[3] for c in out} == set(SWEEP_I) and {c[4] for c in out} == set(SWEEP_J)
    return out


@pytest.mark.parametrize("case", _sweep_cases(), ids=lambda c: f"{c[0]}-B{c[1]}H{c[2]}I{c[3]}J{c[4]}-{c[5]}-{c[6]}-s{c[7]:.3g}")
def test_bf16_bounds_shape_sweep(device, case):
    n, B, H, I, J, fam, mask, scale = case
    _check(device, fam, mask, B, H, I, J, scale, 100 + n)


# ---------------------------------------------------------------------------------------------- masks
MASK_SHAPES = {"none": (2, 3, 129, 300), "key": (2, 3, 129, 300), "triu": (1, 3, 257, 257), "causal": (2, 2, 100, 300),
               "both": (2, 2, 129, 513), "dead_rows": (1, 4, 129, 129), "dead_batch": (3, 2, 64, 200),
               "j1_masked": (2, 3, 33, 1)}


@pytest.mark.parametrize("family", ["peaked", "needles"])
@pytest.mark.parametrize("mask", ref.MASKS)
def test_bf16_bounds_masks(device, mask, family):
    B, H, I, J = MASK_SHAPES[mask]
    _, _, v, d_o, km, cm, got, R = _check(device, family, mask, B, H, I, J, SC, 7)
    if mask == "dead_batch":   # the dead batch element: exactly the mean of v over all keys, no gradient through the scores
        assert float(got["dq"][0].float().abs().max()) == 0.0 and float(got["dk"][0].float().abs().max()) == 0.0
    if mask == "j1_masked":    # one key, masked: o is that key's v row, dq = dk = 0, dv collects every dO row
        assert torch.equal(got["o"].float().cpu(), v.expand(B, H, I, D))
        assert float(got["dq"].float().abs().max()) == 0.0 and float(got["dk"].float().abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- input families, scales
@pytest.mark.parametrize("mask", ["none", "both"])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_bf16_bounds_families(device, family, mask):
    """climb with "both": the running maximum moves in every 64-key tile of the masked loop as well."""
    _check(device, family, mask, 2, 4, 257, 513, SC, 21)


def test_bf16_bounds_needles_largest(device):
    """(2, 8, 1024, 1024), needles at 0, 31, 32, 63, 64, 255, 256 and 1023: o is the needle's v row, and dv of a needle
    key collects exactly the dO rows that point at it (both within the bound)."""
    B, H, I, J = 2, 8, 1024, 1024
    q, k, v, d_o, _, _, got, R = _check(device, "needles", "none", B, H, I, J, SC, 5)
    nd = ref.needle_of(B, H, I, J).unsqueeze(-1).expand(B, H, I, D)
    vn = torch.gather(v.double(), 2, nd)
    assert bool(((got["o"].double().cpu() - vn).abs() <= R["bound_o"]).all())
    dvn = torch.zeros(B, H, J, D, dtype=torch.float64).scatter_add_(2, nd, d_o.double())
    assert bool(((got["dv"].double().cpu() - dvn).abs() <= R["bound_dv"]).all())


@pytest.mark.parametrize("mask", ["none", "both"])
@pytest.mark.parametrize("scale", [SC, 1.0, 0.05], ids=["rsqrtD", "1", "0.05"])
def test_bf16_bounds_scales(device, scale, mask):
    """Scales other than D^-0.5: the masked kernels hold the fill as -1e9 / scale."""
    for fam in ("peaked", "needles"):
        _check(device, fam, mask, 2, 3, 129, 300, scale, 31)


# ---------------------------------------------------------------------------------------------- invariance, reproducibility
def _equal(a, b, what):
    for n in ref.NAMES:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs"


@pytest.mark.parametrize("mask", ["none", "both"])
def test_bf16_batch_element_alone_is_bitwise_equal(device, mask):
    B, H, I, J = 3, 4, 129, 300
    q, k, v, d_o = ref.make_inputs("peaked", B, H, I, J, SC, 41)
    km, cm = ref.make_masks(mask, B, I, J, 41)
    full = _run_ops(device, q, k, v, d_o, SC, km, cm)
    one = _run_ops(device, q[1:2], k[1:2], v[1:2], d_o[1:2], SC, None if km is None else km[1:2], cm)
    _equal({n: t[1:2] for n, t in full.items()}, one, "batch element 1 alone")


@pytest.mark.parametrize("mask", ["key", "both", "dead_rows"])
def test_bf16_reproducible_with_masks(device, mask):
    B, H, I, J = 2, 3, 129, 300
    q, k, v, d_o = ref.make_inputs("diffuse", B, H, I, J, SC, 43)
    km, cm = ref.make_masks(mask, B, I, J, 43)
    _equal(_run_ops(device, q, k, v, d_o, SC, km, cm), _run_ops(device, q, k, v, d_o, SC, km, cm), "second run")


# ---------------------------------------------------------------------------------------------- C ABI
def _P(t, elem_offset=0):
    return ctypes.c_void_p(t.data_ptr() + 2 * elem_offset) if t is not None else ctypes.c_void_p(0)


def _st(view):
    """(sb, st, sh) of a (B, H, T, 64) view."""
    return (view.stride(0), view.stride(2), view.stride(1))


def _abi(device, t, km, cm, scale, offsets=None):
    """amk_attn_bf16_fwd + _bwd on (B,H,T,64) bf16 views t["q"], ...; the outputs t["o"], t["dq"], ... are written in
    place.  offsets: per-tensor element offsets added to the pointers (a misaligned pointer)."""
    from amk import lib

    L = lib.load()
    q, k, v = t["q"], t["k"], t["v"]
    B, H, I, _ = q.shape
    J = k.shape[2]
    off = offsets or {}
    ptr = lambda n: _P(t[n], off.get(n, 0))
    stats = torch.empty((B, H, I, 2), device=device, dtype=torch.float32)
    kmu = None if km is None else km.to(device, torch.uint8).contiguous()
    cmu = None if cm is None else cm.to(device, torch.uint8).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    st = {n: t.get("st_" + n, _st(t[n])) for n in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv")}
    rc = L.amk_attn_bf16_fwd(ptr("q"), ptr("k"), ptr("v"), ptr("o"), _P(stats), _P(kmu), _P(cmu), B, H, I, J, t.get("Dh", D),
                             *st["q"], *st["k"], *st["v"], *st["o"], float(scale), stream)
    if rc != 0:
        return rc, None
    ws = torch.empty((L.amk_attn_bf16_bwd_ws_floats(B, H, I, J),), device=device, dtype=torch.float32)
    rc = L.amk_attn_bf16_bwd(ptr("q"), ptr("k"), ptr("v"), ptr("o"), _P(stats), ptr("d_o"), ptr("dq"), ptr("dk"), ptr("dv"), _P(ws),
                             _P(kmu), _P(cmu), B, H, I, J, t.get("Dh", D),
                             *st["q"], *st["k"], *st["v"], *st["o"], *st["d_o"], *st["dq"], *st["dk"], *st["dv"],
                             float(scale), stream)
    torch.cuda.synchronize()
    return rc, stats


SENTINEL = -7.0   # (bf16-exact) what the output buffers hold where nothing may be written


def _layout(kind, device, B, H, T, x=None):
    """A (B, H, T, 64) bf16 view in the given layout (holding x, or the sentinel), and its backing buffer.
    separate: contiguous (B, H, T, 64).  padded: rows of 88 elements (B, H, T, 88)[..., :64].
    wide: the middle third of a (B, T, 3, H, 64) buffer, i.e. a view with token stride 3 * H * 64."""
    if kind == "separate":
        buf = torch.full((B, H, T, D), SENTINEL, device=device, dtype=torch.bfloat16)
        view = buf
    elif kind == "padded":
        buf = torch.full((B, H, T, 88), SENTINEL, device=device, dtype=torch.bfloat16)
        view = buf[..., :D]
    elif kind == "wide":
        buf = torch.full((B, T, 3, H, D), SENTINEL, device=device, dtype=torch.bfloat16)
        view = buf[:, :, 1].permute(0, 2, 1, 3)
    else:
        raise ValueError(kind)
    if x is not None:
        view.copy_(x)
    return view, buf


@pytest.mark.parametrize("layout", ["separate", "padded", "wide"])
@pytest.mark.parametrize("mask", ["none", "both"])
def test_bf16_c_abi_layouts_match_ops(device, layout, mask):
    """Separate q / k / v / o / dO / dq / dk / dv tensors in (B, H, T, D) layout, rows padded to 88 elements, and views
    into wider buffers: bitwise the ops path's results, and nothing written outside the output views."""
    B, H, I, J = 2, 3, 129, 300
    q, k, v, d_o = ref.make_inputs("peaked", B, H, I, J, SC, 51)
    km, cm = ref.make_masks(mask, B, I, J, 51)
    want = _run_ops(device, q, k, v, d_o, SC, km, cm)
    t, bufs = {}, {}
    for n, x, T in (("q", q, I), ("k", k, J), ("v", v, J), ("d_o", d_o, I)):
        t[n], _ = _layout(layout, device, B, H, T, x.to(device, torch.bfloat16))
    for n, T in (("o", I), ("dq", I), ("dk", J), ("dv", J)):
        t[n], bufs[n] = _layout(layout, device, B, H, T)
    rc, _ = _abi(device, t, km, cm, SC)
    assert rc == 0
    _equal({n: t[n] for n in ref.NAMES}, want, f"C ABI, {layout} layout")
    for n, buf in bufs.items():   # everything outside the view still holds the sentinel
        outside = torch.ones_like(buf, dtype=torch.bool)
        if layout == "separate":
            outside[:] = False
        elif layout == "padded":
            outside[..., :D] = False
        else:
            outside[:, :, 1] = False
        assert bool((buf[outside] == SENTINEL).all()), f"{n}: written outside its view"


def test_bf16_c_abi_one_head_of_eight_is_bitwise_equal(device):
    """Head 5 of an H = 8 call, run alone through the C ABI with the H = 8 strides (pointers moved by 5 * 64 elements):
    bitwise the same o, dq, dk, dv as inside the full call."""
    B, H, I, J, h = 2, 8, 129, 300, 5
    q, k, v, d_o = ref.make_inputs("needles", B, H, I, J, SC, 61)
    km, cm = ref.make_masks("both", B, I, J, 61)
    full = _run_ops(device, q, k, v, d_o, SC, km, cm)
    t = {}
    for n, x, T in (("q", q, I), ("k", k, J), ("v", v, J), ("d_o", d_o, I)):
        view, _ = _layout("separate", device, B, H, T, x.to(device, torch.bfloat16))
        t[n] = view[:, h:h + 1]
    for n, T in (("o", I), ("dq", I), ("dk", J), ("dv", J)):
        view, _ = _layout("separate", device, B, H, T)
        t[n] = view[:, h:h + 1]
    rc, _ = _abi(device, t, km, cm, SC)
    assert rc == 0
    _equal({n: t[n] for n in ref.NAMES}, {n: x[:, h:h + 1] for n, x in full.items()}, f"head {h} alone")


@pytest.mark.parametrize("bad", ["misaligned_q", "misaligned_dq", "q_row_stride_68", "dk_head_stride_4", "head_dim_32"])
def test_bf16_c_abi_refuses_bad_arguments(device, bad):
    """Host-side refusals: a pointer off 16-byte alignment or a stride that is not a multiple of 8 elements is AMK_EINVAL,
    a head dim other than 64 AMK_EUNSUPPORTED, with the library's message -- and nothing launched (the outputs keep
    their sentinels).  The buffers are large enough for every stride given, so nothing could fault either way."""
    from amk import lib

    B, H, I, J = 1, 2, 40, 70
    q, k, v, d_o = ref.make_inputs("diffuse", B, H, I, J, SC, 71)
    t = {}
    for n, x, T in (("q", q, I), ("k", k, J), ("v", v, J), ("d_o", d_o, I)):
        t[n], _ = _layout("padded", device, B, H, T, x.to(device, torch.bfloat16))
    for n, T in (("o", I), ("dq", I), ("dk", J), ("dv", J)):
        t[n], _ = _layout("padded", device, B, H, T)
    offsets = {}
    if bad == "misaligned_q":
        offsets["q"] = 1
    elif bad == "misaligned_dq":
        offsets["dq"] = 1
    elif bad == "q_row_stride_68":
        t["st_q"] = (H * I * 88, 68, I * 88)
    elif bad == "dk_head_stride_4":
        t["st_dk"] = (H * J * 88, 88, 4)
    else:
        t["Dh"] = 32
    fwd_refuses = bad in ("misaligned_q", "q_row_stride_68", "head_dim_32")
    rc, _ = _abi(device, t, None, None, SC, offsets=offsets)
    torch.cuda.synchronize()
    msg = lib.load().amk_last_error().decode()
    if bad == "head_dim_32":
        assert rc == AMK_EUNSUPPORTED and "head dim 32" in msg, (rc, msg)
    else:
        assert rc == AMK_EINVAL and "16-byte aligned" in msg and "multiples of 8" in msg, (rc, msg)
    outs = ("o", "dq", "dk", "dv") if fwd_refuses else ("dq", "dk", "dv")
    for n in outs:
        assert bool((t[n] == SENTINEL).all()), f"{bad}: {n} was written"


# ---------------------------------------------------------------------------------------------- dispatch under autocast
def _fp64_ref(q2, kv2, H, Dh, scale):
    """fp64 attention_core on the (B,I,H*Dh) / (B,J,2*H*Dh) values as given; -> o2, dq2, dkv2 for the cotangent 1."""
    B, I, _ = q2.shape
    J = kv2.shape[1]
    qr, kvr = q2.detach().cpu().double().requires_grad_(True), kv2.detach().cpu().double().requires_grad_(True)
    kv = kvr.view(B, J, 2, H, Dh)
    o = ref_cpu.attention_core(qr.view(B, I, H, Dh).permute(0, 2, 1, 3), kv[:, :, 0].permute(0, 2, 1, 3),
                               kv[:, :, 1].permute(0, 2, 1, 3), scale)
    o2 = o.permute(0, 2, 1, 3).reshape(B, I, H * Dh)
    cot = torch.cos(torch.arange(o2.numel(), dtype=torch.float64)).view_as(o2)
    dq2, dkv2 = torch.autograd.grad((o2 * cot).sum(), [qr, kvr])
    return o2.detach(), dq2, dkv2, cot


def _autocast_run(device, q2, kv2, H, Dh, scale, cot):
    from amk import ops

    qd, kvd = q2.to(device).requires_grad_(True), kv2.to(device).requires_grad_(True)
    ops.KERNEL_EVENTS = {}
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            o2 = ops.attention_fused_kv(qd, kvd, H, Dh, scale)
        dq2, dkv2 = torch.autograd.grad((o2.float() * cot.to(device, torch.float32)).sum(), [qd, kvd])
        torch.cuda.synchronize()
        names = {n for n in ops.KERNEL_EVENTS if n.startswith("attn")}
    finally:
        ops.KERNEL_EVENTS = None
    return o2, dq2, dkv2, names


def _assert_f32_path(names, o2, dq2, dkv2, want):
    o_ref, dq_ref, dkv_ref, _ = want
    assert names and all(n.startswith("attn_fwd") or n.startswith("attn_bwd") for n in names), names
    assert any(n.startswith("attn_fwd") for n in names), names
    assert o2.dtype == torch.float32
    assert_close(o2, o_ref, 2e-5, "o")
    for n, g, r in (("dq", dq2, dq_ref), ("dkv", dkv2, dkv_ref)):
        # the f32 kernels' gradient, handed back in the input's dtype: a bf16 input gets one rounding of a value good to 2e-5
        one_rounding = ref.U if g.dtype == torch.bfloat16 else 0.0
        g, r = g.detach().cpu().double(), r.double()
        lim = one_rounding * r.abs() + 2e-5 * float(r.abs().max())
        assert bool(((g - r).abs() <= lim).all()), f"{n}: worst {float(((g - r).abs() / lim).max()):.3g}x the limit"


@pytest.mark.parametrize("Dh", [32, 128])
def test_bf16_autocast_other_head_dims_take_f32_kernels(device, Dh):
    """Under autocast, bf16 projections with head dims 32 and 128 run on the exact-f32 kernels (there is no bf16 kernel
    for them) and match fp64 on the bf16 values at the f32 suite's 2e-5."""
    B, H, I, J = 2, 3, 100, 140
    q2 = ref.bf16_round(torch.randn(B, I, H * Dh, generator=torch.Generator().manual_seed(81))).bfloat16()
    kv2 = ref.bf16_round(torch.randn(B, J, 2 * H * Dh, generator=torch.Generator().manual_seed(82))).bfloat16()
    want = _fp64_ref(q2, kv2, H, Dh, Dh ** -0.5)
    o2, dq2, dkv2, names = _autocast_run(device, q2, kv2, H, Dh, Dh ** -0.5, want[3])
    assert dq2.dtype == dkv2.dtype == torch.bfloat16
    _assert_f32_path(names, o2, dq2, dkv2, want)


def test_bf16_autocast_switched_off_takes_f32_kernels(device, monkeypatch):
    """ops.ATTENTION_BF16 = False: head dim 64 under autocast runs on the f32 kernels too."""
    from amk import ops

    monkeypatch.setattr(ops, "ATTENTION_BF16", False)
    B, H, I, J = 2, 3, 100, 140
    q2 = torch.randn(B, I, H * D, generator=torch.Generator().manual_seed(83)).bfloat16()
    kv2 = torch.randn(B, J, 2 * H * D, generator=torch.Generator().manual_seed(84)).bfloat16()
    want = _fp64_ref(q2, kv2, H, D, SC)
    o2, dq2, dkv2, names = _autocast_run(device, q2, kv2, H, D, SC, want[3])
    _assert_f32_path(names, o2, dq2, dkv2, want)


def test_bf16_q_with_f32_kv_under_autocast_takes_f32_kernels(device):
    """bf16 q with f32 kv under autocast is handled, not refused: the bf16 kernels want both in bf16, so the call takes
    the f32 kernels on q upcast (exact) and kv as given, and matches fp64 on those values at 2e-5."""
    B, H, I, J = 2, 3, 100, 140
    q2 = torch.randn(B, I, H * D, generator=torch.Generator().manual_seed(85)).bfloat16()
    kv2 = torch.randn(B, J, 2 * H * D, generator=torch.Generator().manual_seed(86))
    want = _fp64_ref(q2, kv2, H, D, SC)
    o2, dq2, dkv2, names = _autocast_run(device, q2, kv2, H, D, SC, want[3])
    assert dq2.dtype == torch.bfloat16 and dkv2.dtype == torch.float32
    _assert_f32_path(names, o2, dq2, dkv2, want)
