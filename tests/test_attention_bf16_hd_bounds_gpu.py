"""The bf16 attention kernels for head dims 32 and 128 (csrc/attn_bf16_hd.hip) held element by element to the error bound
of tests/bf16_attention_hd_ref.py: o, dq, dk and dv against the fp64 reference on the bf16 values, at the tile edges (128
queries per forward workgroup over 64-key tiles, KEY_BLOCK[D] keys per backward workgroup over 32-query tiles), under
every mask kind, on every input family, at three scales.  Plus what a tolerance cannot see: batch and head invariance and
run-to-run reproducibility (bitwise), the C ABI with separate tensors, padded strides and views into wider buffers
(bitwise against the ops path), its refusals, independence of stale memory in the internal buffers, and which kernels
ops.ATTENTION_BF16_DIMS picks.

AMK_BF16_BOUND_REPORT=<file>: write the worst |got - ref| / bound per tensor over this module to that JSON file."""
import ctypes
import json
import os
import random

import pytest
import torch

import bf16_attention_hd_ref as ref
from poison import assert_fill_independent, run_both_fills

pytestmark = pytest.mark.gpu
DIMS = ref.HEAD_DIMS
AMK_EINVAL, AMK_EUNSUPPORTED = -1, -2


WORST = {}   # "D<head dim>/<tensor>": the worst |got - ref| / bound over this module


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AMK_BF16_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(WORST, f, indent=1)


@pytest.fixture(autouse=True)
def _dims(monkeypatch):
    """Every test of this module runs with the two head dims enabled, unless it sets the switch itself."""
    from amk import ops

    monkeypatch.setattr(ops, "ATTENTION_BF16_DIMS", frozenset((32, 64, 128)))


def _fused(q, k, v):
    """(B,H,T,D) -> q2 (B,I,H*D), kv2 (B,J,2*H*D) as the projections lay them out."""
    B, H, I, D = q.shape
    J = k.shape[2]
    q2 = q.permute(0, 2, 1, 3).reshape(B, I, H * D)
    kv2 = torch.stack([k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)], dim=2).reshape(B, J, 2 * H * D)
    return q2, kv2


def _run_ops(device, q, k, v, d_o, scale, km=None, cm=None):
    """ops.attention_fused_kv forward + backward on bf16 copies; asserts the head-dim kernels ran.  -> {name: (B,H,T,D)}"""
    from amk import ops

    B, H, I, D = q.shape
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
    assert names == {"attn_bf16_hd_fwd_kernel" + sfx, "attn_bf16_hd_bwd_kernel" + sfx}, names
    assert o2.dtype == dq2.dtype == dkv2.dtype == torch.bfloat16
    dkv = dkv2.view(B, J, 2, H, D)
    return {"o": o2.view(B, I, H, D).permute(0, 2, 1, 3), "dq": dq2.view(B, I, H, D).permute(0, 2, 1, 3),
            "dk": dkv[:, :, 0].permute(0, 2, 1, 3), "dv": dkv[:, :, 1].permute(0, 2, 1, 3)}


_CASES = {}   # inputs, masks and the fp64 reference of a case, computed once and left unchanged


def _case(family, mask, B, H, I, J, D, scale, seed):
    key = (family, mask, B, H, I, J, D, scale, seed)
    if key not in _CASES:
        q, k, v, d_o = ref.make_inputs(family, B, H, I, J, D, scale, seed)
        km, cm = ref.make_masks(mask, B, I, J, seed)
        _CASES[key] = (q, k, v, d_o, km, cm, ref.reference(q, k, v, d_o, scale, km, cm))
    return _CASES[key]


def _check(device, family, mask, B, H, I, J, D, scale, seed):
    q, k, v, d_o, km, cm, R = _case(family, mask, B, H, I, J, D, scale, seed)
    got = _run_ops(device, q, k, v, d_o, scale, km, cm)
    res = ref.ratios(got, R)
    print("worst ratios", {n: round(w, 3) for n, (_, w) in res.items()})
    for n, (nbad, worst) in res.items():
        WORST[f"D{D}/{n}"] = max(WORST.get(f"D{D}/{n}", 0.0), worst)
        assert nbad == 0, f"D{D}/{family}/{mask}/B{B}H{H}I{I}J{J}/scale {scale:g} {n}: {nbad} elements outside the bound (worst {worst:.3g}x the bound)"
    return q, k, v, d_o, km, cm, got, R


# ---------------------------------------------------------------------------------------------- shape sweep
SWEEP_I = (1, 31, 32, 33, 127, 128, 129, 257)


def _sweep_j(D):
    KB = ref.KEY_BLOCK[D]
    return (1, 63, 64, 65, KB - 1, KB, KB + 1, 2 * KB + 1, 1024)


def _sweep_cases():
    """Per head dim: every I and every J of the tile edges at least once (18 cases), each with a seeded head count,
    batch, input family, mask and scale, drawn as the D = 64 module draws them."""
    out = []
    for D in DIMS:
        rng = random.Random(20261016)      # (the D = 64 module's seed: its draw covers every I)
        Is, Js = list(SWEEP_I) * 3, list(_sweep_j(D)) * 2
        rng.shuffle(Is)
        rng.shuffle(Js)
        mine = []
        for n in range(18):
            I, J = Is[n], Js[n]
            H = rng.choice([1, 3, 8, 16])
            B = rng.choice([1, 2, 3])
            while B * H * I * J > 3 * 2 ** 20 and (H > 1 or B > 1):   # (the fp64 reference of one case stays ~1 s)
                H, B = (H // 2, B) if H > 1 else (H, B - 1)
            fam = ref.FAMILIES[n % len(ref.FAMILIES)]
            mask = ("none", "key", "causal", "both", "triu", "dead_rows")[n % 6]
            scale = (D ** -0.5, 1.0, 0.05)[n % 3]
            mine.append((D, n, B, H, I, J, fam, mask, scale))
        assert {c[4] for c in mine} == set(SWEEP_I) and {c[5] for c in mine} == set(_sweep_j(D))
        out += mine
    return out


@pytest.mark.parametrize("case", _sweep_cases(), ids=lambda c: f"D{c[0]}-{c[1]}-B{c[2]}H{c[3]}I{c[4]}J{c[5]}-{c[6]}-{c[7]}-s{c[8]:.3g}")
def test_bf16_hd_bounds_shape_sweep(device, case):
    D, n, B, H, I, J, fam, mask, scale = case
    _check(device, fam, mask, B, H, I, J, D, scale, 100 + n)


# ---------------------------------------------------------------------------------------------- masks
MASK_SHAPES = {"none": (2, 3, 129, 300), "key": (2, 3, 129, 300), "triu": (1, 3, 257, 257), "causal": (2, 2, 100, 300),
               "both": (2, 2, 129, 513), "dead_rows": (1, 4, 129, 129), "dead_batch": (3, 2, 64, 200),
               "j1_masked": (2, 3, 33, 1)}


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("family", ["peaked", "needles"])
@pytest.mark.parametrize("mask", ref.MASKS)
def test_bf16_hd_bounds_masks(device, mask, family, D):
    B, H, I, J = MASK_SHAPES[mask]
    _, _, v, d_o, km, cm, got, R = _check(device, family, mask, B, H, I, J, D, D ** -0.5, 7)
    if mask == "dead_batch":   # the dead batch element: exactly the mean of v over all keys, no gradient through the scores
        assert float(got["dq"][0].float().abs().max()) == 0.0 and float(got["dk"][0].float().abs().max()) == 0.0
    if mask == "j1_masked":    # one key, masked: o is that key's v row, dq = dk = 0, dv collects every dO row
        assert torch.equal(got["o"].float().cpu(), v.expand(B, H, I, D))
        assert float(got["dq"].float().abs().max()) == 0.0 and float(got["dk"].float().abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- input families, scales
@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("mask", ["none", "both"])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_bf16_hd_bounds_families(device, family, mask, D):
    """climb with "both": the running maximum moves in every 64-key tile of the masked loop as well."""
    _check(device, family, mask, 2, 4, 257, 513, D, D ** -0.5, 21)


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("mask", ["none", "both"])
@pytest.mark.parametrize("scale", ["rsqrtD", 1.0, 0.05], ids=["rsqrtD", "1", "0.05"])
def test_bf16_hd_bounds_scales(device, scale, mask, D):
    """Scales other than D^-0.5: the masked kernels hold the fill as -1e9 / scale."""
    scale = D ** -0.5 if scale == "rsqrtD" else scale
    for fam in ("peaked", "needles"):
        _check(device, fam, mask, 2, 3, 129, 300, D, scale, 31)


# ---------------------------------------------------------------------------------------------- invariance, reproducibility
def _equal(a, b, what):
    for n in ref.NAMES:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs"


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("mask", ["none", "both"])
def test_bf16_hd_batch_element_alone_is_bitwise_equal(device, mask, D):
    B, H, I, J = 3, 4, 129, 300
    q, k, v, d_o = ref.make_inputs("peaked", B, H, I, J, D, D ** -0.5, 41)
    km, cm = ref.make_masks(mask, B, I, J, 41)
    full = _run_ops(device, q, k, v, d_o, D ** -0.5, km, cm)
    one = _run_ops(device, q[1:2], k[1:2], v[1:2], d_o[1:2], D ** -0.5, None if km is None else km[1:2], cm)
    _equal({n: t[1:2] for n, t in full.items()}, one, "batch element 1 alone")


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("mask", ["none", "key", "both", "dead_rows"])
def test_bf16_hd_reproducible(device, mask, D):
    B, H, I, J = 2, 3, 129, 300
    q, k, v, d_o = ref.make_inputs("diffuse", B, H, I, J, D, D ** -0.5, 43)
    km, cm = ref.make_masks(mask, B, I, J, 43)
    _equal(_run_ops(device, q, k, v, d_o, D ** -0.5, km, cm), _run_ops(device, q, k, v, d_o, D ** -0.5, km, cm), "second run")


# ---------------------------------------------------------------------------------------------- stale memory
# (B, H, I, J, mask): whole tiles; one past a tile edge with masks; the smallest
STALE_SHAPES = [(1, 2, 128, 128, "none"), (2, 2, 129, 257, "both"), (1, 2, 33, 65, "key"), (1, 1, 1, 1, "none")]


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("shape", STALE_SHAPES, ids=lambda s: f"B{s[0]}H{s[1]}I{s[2]}J{s[3]}-{s[4]}")
def test_bf16_hd_results_do_not_depend_on_stale_memory(device, shape, D):
    """Forward + backward with every torch.empty of the ops path (o, the statistics, dq, dkv, the workspace of row
    constants and dQ partials) pre-filled with NaN bytes and with 0x7F bytes: finite, and the bits of the plain run."""
    B, H, I, J, mask = shape
    q, k, v, d_o = ref.make_inputs("diffuse", B, H, I, J, D, D ** -0.5, 47)
    km, cm = ref.make_masks(mask, B, I, J, 47)
    case = lambda: _run_ops(device, q, k, v, d_o, D ** -0.5, km, cm)
    plain = {n: t.detach().clone() for n, t in case().items()}
    nan_run, big_run = run_both_fills(case)
    assert_fill_independent(nan_run, big_run, f"D{D} {shape}")
    _equal(nan_run, plain, "poisoned against plain")


# ---------------------------------------------------------------------------------------------- C ABI
def _P(t, elem_offset=0):
    return ctypes.c_void_p(t.data_ptr() + 2 * elem_offset) if t is not None else ctypes.c_void_p(0)


def _st(view):
    """(sb, st, sh) of a (B, H, T, D) view."""
    return (view.stride(0), view.stride(2), view.stride(1))


def _abi(device, t, km, cm, scale, D, offsets=None):
    """amk_attn_bf16_hd_fwd + _bwd on (B,H,T,D) bf16 views t["q"], ...; the outputs t["o"], t["dq"], ... are written in
    place.  offsets: per-tensor element offsets added to the pointers (a misaligned pointer); t["Dh"]: the head dim
    passed, if not D.  -> [(rc, message)] of the calls made: the forward, and the backward unless the forward refused
    (t["bwd_after_refusal"]: the backward is asked all the same)."""
    from amk import lib

    L = lib.load()
    q, k = t["q"], t["k"]
    B, H, I, _ = q.shape
    J = k.shape[2]
    off = offsets or {}
    ptr = lambda n: _P(t[n], off.get(n, 0))
    stats = torch.zeros((B, H, I, 2), device=device, dtype=torch.float32)
    kmu = None if km is None else km.to(device, torch.uint8).contiguous()
    cmu = None if cm is None else cm.to(device, torch.uint8).contiguous()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    st = {n: t.get("st_" + n, _st(t[n])) for n in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv")}
    Dh = t.get("Dh", D)
    rc_f = L.amk_attn_bf16_hd_fwd(ptr("q"), ptr("k"), ptr("v"), ptr("o"), _P(stats), _P(kmu), _P(cmu), B, H, I, J, Dh,
                                  *st["q"], *st["k"], *st["v"], *st["o"], float(scale), stream)
    msg_f = L.amk_last_error().decode()
    if rc_f != 0 and not t.get("bwd_after_refusal"):
        return [(rc_f, msg_f)]
    ws = torch.zeros((max(16, L.amk_attn_bf16_hd_bwd_ws_floats(B, H, I, J, D)),), device=device, dtype=torch.float32)
    rc = L.amk_attn_bf16_hd_bwd(ptr("q"), ptr("k"), ptr("v"), ptr("o"), _P(stats), ptr("d_o"), ptr("dq"), ptr("dk"), ptr("dv"), _P(ws),
                                _P(kmu), _P(cmu), B, H, I, J, Dh,
                                *st["q"], *st["k"], *st["v"], *st["o"], *st["d_o"], *st["dq"], *st["dk"], *st["dv"],
                                float(scale), stream)
    msg = L.amk_last_error().decode()
    torch.cuda.synchronize()
    return [(rc_f, msg_f), (rc, msg)]


SENTINEL = -7.0   # (bf16-exact) what the output buffers hold where nothing may be written


def _layout(kind, device, B, H, T, D, x=None):
    """A (B, H, T, D) bf16 view in the given layout (holding x, or the sentinel), and its backing buffer.
    separate: contiguous (B, H, T, D).  padded: rows of D + 24 elements.
    wide: the middle third of a (B, T, 3, H, D) buffer, i.e. a view with token stride 3 * H * D."""
    if kind == "separate":
        buf = torch.full((B, H, T, D), SENTINEL, device=device, dtype=torch.bfloat16)
        view = buf
    elif kind == "padded":
        buf = torch.full((B, H, T, D + 24), SENTINEL, device=device, dtype=torch.bfloat16)
        view = buf[..., :D]
    elif kind == "wide":
        buf = torch.full((B, T, 3, H, D), SENTINEL, device=device, dtype=torch.bfloat16)
        view = buf[:, :, 1].permute(0, 2, 1, 3)
    else:
        raise ValueError(kind)
    if x is not None:
        view.copy_(x)
    return view, buf


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("layout", ["separate", "padded", "wide"])
@pytest.mark.parametrize("mask", ["none", "both"])
def test_bf16_hd_c_abi_layouts_match_ops(device, layout, mask, D):
    """Separate q / k / v / o / dO / dq / dk / dv tensors in (B, H, T, D) layout, rows padded by 24 elements, and views
    into wider buffers: bitwise the ops path's results, and nothing written outside the output views."""
    B, H, I, J = 2, 3, 129, 300
    SC = D ** -0.5
    q, k, v, d_o = ref.make_inputs("peaked", B, H, I, J, D, SC, 51)
    km, cm = ref.make_masks(mask, B, I, J, 51)
    want = _run_ops(device, q, k, v, d_o, SC, km, cm)
    t, bufs = {}, {}
    for n, x, T in (("q", q, I), ("k", k, J), ("v", v, J), ("d_o", d_o, I)):
        t[n], _ = _layout(layout, device, B, H, T, D, x.to(device, torch.bfloat16))
    for n, T in (("o", I), ("dq", I), ("dk", J), ("dv", J)):
        t[n], bufs[n] = _layout(layout, device, B, H, T, D)
    calls = _abi(device, t, km, cm, SC, D)
    assert [rc for rc, _ in calls] == [0, 0], calls
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


@pytest.mark.parametrize("D", DIMS)
def test_bf16_hd_c_abi_one_head_of_eight_is_bitwise_equal(device, D):
    """Head 5 of an H = 8 call, run alone through the C ABI with the H = 8 strides (pointers moved by 5 * D elements):
    bitwise the same o, dq, dk, dv as inside the full call."""
    B, H, I, J, h = 2, 8, 129, 300, 5
    SC = D ** -0.5
    q, k, v, d_o = ref.make_inputs("needles", B, H, I, J, D, SC, 61)
    km, cm = ref.make_masks("both", B, I, J, 61)
    full = _run_ops(device, q, k, v, d_o, SC, km, cm)
    t = {}
    for n, x, T in (("q", q, I), ("k", k, J), ("v", v, J), ("d_o", d_o, I)):
        view, _ = _layout("separate", device, B, H, T, D, x.to(device, torch.bfloat16))
        t[n] = view[:, h:h + 1]
    for n, T in (("o", I), ("dq", I), ("dk", J), ("dv", J)):
        view, _ = _layout("separate", device, B, H, T, D)
        t[n] = view[:, h:h + 1]
    calls = _abi(device, t, km, cm, SC, D)
    assert [rc for rc, _ in calls] == [0, 0], calls
    _equal({n: t[n] for n in ref.NAMES}, {n: x[:, h:h + 1] for n, x in full.items()}, f"head {h} alone")


@pytest.mark.parametrize("D", DIMS)
@pytest.mark.parametrize("bad", ["misaligned_q", "misaligned_dq", "q_row_stride_68", "dk_head_stride_4", "head_dim_64", "head_dim_96"])
def test_bf16_hd_c_abi_refusals_leave_outputs_untouched(device, bad, D):
    """Host-side refusals: a pointer off 16-byte alignment or a stride that is not a multiple of 8 elements is AMK_EINVAL,
    a head dim other than 32 / 128 AMK_EUNSUPPORTED with a message that names it and points head dim 64 to
    amk_attn_bf16_fwd -- and nothing launched: the outputs keep their sentinels.  The buffers are large enough for every
    stride given, so nothing could fault either way."""
    B, H, I, J = 1, 2, 40, 70
    SC = D ** -0.5
    q, k, v, d_o = ref.make_inputs("diffuse", B, H, I, J, D, SC, 71)
    t = {}
    for n, x, T in (("q", q, I), ("k", k, J), ("v", v, J), ("d_o", d_o, I)):
        t[n], _ = _layout("padded", device, B, H, T, D, x.to(device, torch.bfloat16))
    for n, T in (("o", I), ("dq", I), ("dk", J), ("dv", J)):
        t[n], _ = _layout("padded", device, B, H, T, D)
    offsets = {}
    if bad == "misaligned_q":
        offsets["q"] = 1
    elif bad == "misaligned_dq":
        offsets["dq"] = 1
    elif bad == "q_row_stride_68":
        t["st_q"] = (H * I * (D + 24), 68, I * (D + 24))
    elif bad == "dk_head_stride_4":
        t["st_dk"] = (H * J * (D + 24), D + 24, 4)
    else:
        t["Dh"] = int(bad.rsplit("_", 1)[1])
        t["bwd_after_refusal"] = True      # the backward entry point is asked too: it must refuse by itself
    fwd_refuses = bad in ("misaligned_q", "q_row_stride_68", "head_dim_64", "head_dim_96")
    calls = _abi(device, t, None, None, SC, D, offsets=offsets)
    torch.cuda.synchronize()
    if bad.startswith("head_dim"):
        assert len(calls) == 2
        for rc, msg in calls:
            assert rc == AMK_EUNSUPPORTED and f"head dim {t['Dh']}" in msg and "amk_attn_bf16_fwd" in msg, calls
    else:
        assert len(calls) == (1 if fwd_refuses else 2) and (fwd_refuses or calls[0][0] == 0), calls
        rc, msg = calls[-1]
        assert rc == AMK_EINVAL and "16-byte aligned" in msg and "multiples of 8" in msg, calls
    outs = ("o", "dq", "dk", "dv") if fwd_refuses else ("dq", "dk", "dv")
    for n in outs:
        assert bool((t[n] == SENTINEL).all()), f"{bad}: {n} was written"


# ---------------------------------------------------------------------------------------------- dispatch under autocast
def _autocast_run(device, H, D):
    from amk import ops

    B, I, J = 2, 100, 140
    q2 = torch.randn(B, I, H * D, generator=torch.Generator().manual_seed(81)).bfloat16().to(device).requires_grad_(True)
    kv2 = torch.randn(B, J, 2 * H * D, generator=torch.Generator().manual_seed(82)).bfloat16().to(device).requires_grad_(True)
    ops.KERNEL_EVENTS = {}
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            o2 = ops.attention_fused_kv(q2, kv2, H, D, D ** -0.5)
        dq2, dkv2 = torch.autograd.grad(o2.float().sum(), [q2, kv2])
        torch.cuda.synchronize()
        names = {n for n in ops.KERNEL_EVENTS if n.startswith("attn")}
    finally:
        ops.KERNEL_EVENTS = None
    return o2, dq2, dkv2, names


@pytest.mark.parametrize("D", DIMS)
def test_bf16_hd_dispatch_follows_the_switch(device, monkeypatch, D):
    """With the head dim in ops.ATTENTION_BF16_DIMS the call launches exactly the attn_bf16_hd_* kernels and o, dq, dkv
    are bf16; with the default set the same call launches the f32 kernels and returns an f32 o, as before the switch."""
    from amk import ops

    o2, dq2, dkv2, names = _autocast_run(device, 3, D)
    assert names == {"attn_bf16_hd_fwd_kernel", "attn_bf16_hd_bwd_kernel"}, names
    assert o2.dtype == dq2.dtype == dkv2.dtype == torch.bfloat16
    monkeypatch.setattr(ops, "ATTENTION_BF16_DIMS", ops._parse_bf16_dims("64"))
    o32, dq32, dkv32, names = _autocast_run(device, 3, D)
    assert names and all(n.startswith("attn_fwd") or n.startswith("attn_bwd") for n in names), names
    assert o32.dtype == torch.float32 and dq32.dtype == dkv32.dtype == torch.bfloat16


def test_bf16_hd_switch_leaves_head_dim_64_on_its_kernels(device):
    """Head dim 64 with all three dims enabled: the existing kernels, under their existing names."""
    _, _, _, names = _autocast_run(device, 3, 64)
    assert names == {"attn_bf16_fwd_kernel", "attn_bf16_bwd_kernel"}, names
