"""The checker of tests/test_ce_head_bf16_gpu.py checks itself, without a GPU.

* The fp64 reference of tests/ce_head_bf16_ref.py equals F.cross_entropy(F.linear(x, w), target, ignore_index) and its
  autograd in fp64 on bf16-valued inputs.
* A CPU emulation of csrc/ce_head_bf16.hip in the kernels' own order stays under half of every hard bound on every
  family and shape class and defines the constants Q_EMU of the tight tier.
* The bounds reject, on at least one tensor in every family at (129, 1000, 264): the mean taken over M instead of over
  count, ignore_index not honoured, a target column off by one, and operands (x, w and G) rounded to 7 instead of 8 significant bits.
* The library path's semantics -- the logits rounded to bf16 before the softmax -- are rejected at least on `large` and
  `needle-30`.
* The library exports the four entry points, and every argument error returns its code with a message before any
  device work (no GPU is needed).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ce_head_bf16_ref as ref

SHAPES = [(1, 1, 8), (127, 8, 40), (128, 127, 64), (129, 129, 8), (300, 128, 40), (129, 1000, 264), (300, 1000, 264),
          (300, 8192, 40)]   # (the last: four tiles per slice, sixteen slices, the longest dx chain of the GPU cases)
REJECT_SHAPE = (129, 1000, 264)
D_LOSS = 0.7
NAMES = ("loss", "dx", "dw")
_CACHE = {}


def case(family, shape, mut=None, pattern=None):
    key = (family, shape, mut, pattern)
    if key not in _CACHE:
        M, V, K = shape
        pattern = pattern or ("all" if M == 1 else "random64")
        target = ref.make_target(M, V, pattern, seed=M + V)
        x, w = ref.make_inputs(family, M, V, K, target, seed=K)
        rkey = (family, shape, "ref", pattern)
        if rkey not in _CACHE:
            _CACHE[rkey] = ref.reference(x, w, target, -1, D_LOSS)
        _CACHE[key] = (ref.emulate(x, w, target, -1, D_LOSS, mut), _CACHE[rkey], (x, w, target))
    return _CACHE[key]


@pytest.mark.parametrize("family", ref.CPU_FAMILIES)
def test_reference_equals_torch_fp64(family):
    for shape in ((129, 1000, 264), (127, 8, 40)):
        _, R, (x, w, target) = case(family, shape)
        assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16
        xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
        loss = F.cross_entropy(F.linear(xd, wd), target, ignore_index=-1)
        (loss * D_LOSS).backward()
        for name, got in (("loss", loss.detach()), ("dx", xd.grad), ("dw", wd.grad)):
            assert torch.allclose(R[name], got, rtol=1e-11, atol=1e-11), (family, shape, name)


def test_reference_edge_semantics():
    """count == 0: NaN loss and zero gradients; an out-of-range target poisons the loss, takes no gradient, and is
    still counted in the mean's divisor."""
    M, V, K = 40, 12, 8
    t = ref.make_target(M, V, "all")
    x, w = ref.make_inputs("unit", M, V, K, t)
    R0 = ref.reference(x, w, torch.full((M,), -1), -1)
    assert torch.isnan(R0["loss"]) and not R0["dx"].any() and not R0["dw"].any()
    bad = t.clone()
    bad[3], bad[7] = V + 2, -5
    Rb = ref.reference(x, w, bad, -1)
    dropped = t.clone()
    dropped[3] = dropped[7] = -1
    Rd = ref.reference(x, w, dropped, -1)
    assert torch.isnan(Rb["loss"]) and Rb["count"] == M and Rd["count"] == M - 2
    assert not Rb["dx"][3].any() and not Rb["dx"][7].any()
    assert torch.allclose(Rb["dw"] * M, Rd["dw"] * (M - 2), rtol=1e-12, atol=1e-15)
    loss, dx, dw = ref.emulate(x, w, bad, -1)
    assert torch.isnan(loss) and not dx[3].any() and not dx[7].any() and dx.dtype == torch.bfloat16
    assert ref.measures(dw, Rb, "dw")[0] == 0 and ref.measures(dx, Rb, "dx")[0] == 0
    loss, dx, dw = ref.emulate(x, w, torch.full((M,), -1), -1)
    assert torch.isnan(loss) and not dx.any() and not dw.any()


@pytest.mark.parametrize("family", ref.CPU_FAMILIES)
def test_emulation_within_half_the_hard_bound(family):
    for shape in SHAPES:
        got, R, _ = case(family, shape)
        for name, g in zip(NAMES, got):
            nbad, ratio, q = ref.measures(g, R, name)
            assert nbad == 0 and ratio <= 0.5, f"{family} {shape} {name}: the emulation reaches {ratio:.3f} of the hard bound"
            assert q <= ref.Q_EMU[name], f"{family} {shape} {name}: q {q:.3f} above Q_EMU = {ref.Q_EMU[name]}"


def test_emulation_defines_q(capsys):
    """Q_EMU is the emulation's worst q per output over every family and shape class, rounded up by at most a tenth."""
    worst = {}
    for family in ref.CPU_FAMILIES:
        for shape in SHAPES:
            got, R, _ = case(family, shape)
            for name, g in zip(NAMES, got):
                worst[name] = max(worst.get(name, 0.0), ref.measures(g, R, name)[2])
    with capsys.disabled():
        print("\nbf16 head, emulation worst q:", {k: round(v, 4) for k, v in worst.items()})
    for name, q in worst.items():
        assert q <= ref.Q_EMU[name] <= 1.1 * q, f"Q_EMU[{name}] = {ref.Q_EMU[name]} against the emulation's {q:.4f}"


@pytest.mark.parametrize("family", ref.CPU_FAMILIES)
@pytest.mark.parametrize("fault", ["mean_over_M", "ignore_not_honoured", "target_off_by_one", "bits7"])
def test_planted_fault_is_rejected(fault, family):
    """Every fault leaves at least one of loss / dx / dw outside its hard bound, in every family.

    bits7 rounds every bf16 operand of the three products to 7 significant bits: x, w and G.  With x and w alone the
    `large` family is NOT rejected (measured, hard ratio: loss 0.004, dx 0.24, dw 0.96): a 7-bit rounding is at most
    2^-7 relative, which is what the bound grants the one bf16 rounding of G (2 U16, the project's factor 2), and the
    common offset of 3000 makes the loss bound 0.10 (gamma_289 x 3000 per logit) while the fault moves the loss by 4e-4.
    With G included, `large` is rejected through dw at 1.7 x (the f32 head's checker rejects its analogous fault there
    at 1.8 x)."""
    got, R, _ = case(family, REJECT_SHAPE)
    assert sum(ref.violations(g, R, n) for n, g in zip(NAMES, got)) == 0
    bad, R, _ = case(family, REJECT_SHAPE, fault)
    flagged = [n for n, g in zip(NAMES, bad) if ref.measures(g, R, n)[0] > 0]
    assert flagged, f"{fault} on {family} inputs stays inside every hard bound"


@pytest.mark.parametrize("family", ["large", "needle-30"])
@pytest.mark.parametrize("shape", [REJECT_SHAPE, (300, 8192, 40)])
def test_logits_rounded_to_bf16_are_rejected(family, shape):
    """What the library path computes under autocast -- bf16 logits, then the softmax -- is outside the bounds (on unit,
    climb and needle+30 inputs it stays inside the loss bound, so those are not asked for)."""
    bad, R, _ = case(family, shape, "bf16_logits")
    flagged = [n for n, g in zip(NAMES, bad) if ref.measures(g, R, n)[0] > 0]
    assert flagged, f"bf16 logits on {family} inputs at {shape} stay inside every hard bound"


def test_logit_chain_rule():
    assert [ref.logit_chain(K) for K in (8, 32, 40, 64, 264, 1024)] == [33, 33, 65, 65, 289, 1025]


# ---------------------------------------------------------------------------------------------- the ABI without a GPU
EXPORTS = ("amk_ce_head_bf16_fwd_ws_bytes", "amk_ce_head_bf16_bwd_ws_bytes", "amk_ce_head_bf16_fwd", "amk_ce_head_bf16_bwd")


def test_library_exports_the_bf16_loss_head():
    from amk import lib as amk_lib

    L = amk_lib.load()
    for name in EXPORTS:
        assert hasattr(L, name) and name in amk_lib.SIGNATURES
    M, V, K = 300, 8192, 1024
    ns, _ = ref.slices(M, V)
    assert L.amk_ce_head_bf16_fwd_ws_bytes(M, V, K) == 3 * M * ns * 4
    assert L.amk_ce_head_bf16_bwd_ws_bytes(M, V, K) == M * 8192 * 2           # half the f32 head's bytes
    assert L.amk_ce_head_bf16_bwd_ws_bytes(M, V, K) * 2 == L.amk_ce_head_bwd_ws_bytes(M, V, K)
    assert L.amk_ce_head_bf16_bwd_ws_bytes(129, 1000, 264) == 129 * 1024 * 2
    assert L.amk_ce_head_bf16_fwd_ws_bytes(0, V, K) == 0 and L.amk_ce_head_bf16_bwd_ws_bytes(M, -1, K) == 0


def _call(L, which, **over):
    """One entry point with plausible (never dereferenced) addresses; `over` replaces arguments by name."""
    P = ctypes.c_void_p
    a = dict(x=1 << 20, ldx=64, w=2 << 20, ldw=64, target=3 << 20, ignore_index=-1, M=128, V=100, K=64, loss=4 << 20,
             d_loss=4 << 20, lse=5 << 20, rows=6 << 20, count=7 << 20, dx=8 << 20, lddx=64, dw=9 << 20, lddw=64,
             ws=10 << 20, ws_bytes=1 << 30)
    a.update(over)
    p = {k: P(v) for k, v in a.items() if k in ("x", "w", "target", "loss", "d_loss", "lse", "rows", "count", "dx", "dw", "ws")}
    if which == "fwd":
        return L.amk_ce_head_bf16_fwd(p["x"], a["ldx"], p["w"], a["ldw"], p["target"], a["ignore_index"], a["M"], a["V"],
                                      a["K"], p["loss"], p["lse"], p["rows"], p["count"], p["ws"], a["ws_bytes"], P(0))
    return L.amk_ce_head_bf16_bwd(p["x"], a["ldx"], p["w"], a["ldw"], p["target"], a["ignore_index"], a["M"], a["V"], a["K"],
                                  p["d_loss"], p["lse"], p["rows"], p["count"], p["dx"], a["lddx"], p["dw"], a["lddw"],
                                  p["ws"], a["ws_bytes"], P(0))


EINVAL, EUNSUPPORTED = -1, -2
ERRORS = [
    ("fwd", dict(x=0), EINVAL, b"null"), ("fwd", dict(count=0), EINVAL, b"null"), ("bwd", dict(d_loss=0), EINVAL, b"null"),
    ("bwd", dict(dw=0), EINVAL, b"null"),
    ("fwd", dict(M=0), EINVAL, b"non-positive"), ("fwd", dict(V=-3), EINVAL, b"non-positive"),
    ("bwd", dict(K=0), EINVAL, b"non-positive"),
    ("fwd", dict(x=(1 << 20) + 8), EINVAL, b"misaligned"), ("fwd", dict(ws=(10 << 20) + 8), EINVAL, b"misaligned"),
    ("bwd", dict(dx=(8 << 20) + 8), EINVAL, b"misaligned"), ("bwd", dict(target=(3 << 20) + 4), EINVAL, b"misaligned"),
    ("fwd", dict(ws_bytes=16), EINVAL, b"workspace"), ("bwd", dict(ws_bytes=128 * 128 * 2 - 1), EINVAL, b"workspace"),
    ("fwd", dict(ldx=56), EINVAL, b"below K"), ("bwd", dict(lddw=56), EINVAL, b"below K"),
    ("fwd", dict(K=60, ldx=64), EUNSUPPORTED, b"multiple of 8"), ("fwd", dict(ldx=68), EUNSUPPORTED, b"multiples of 8"),
    ("bwd", dict(ldw=76), EUNSUPPORTED, b"multiples of 8"), ("bwd", dict(lddx=68), EUNSUPPORTED, b"multiples of 8"),
    ("bwd", dict(lddw=76), EUNSUPPORTED, b"multiples of 8"),
    ("fwd", dict(M=(1 << 24) + 1), EUNSUPPORTED, b"limits"), ("bwd", dict(V=(1 << 22) + 1), EUNSUPPORTED, b"limits"),
    ("fwd", dict(K=(1 << 16) + 8, ldx=1 << 17, ldw=1 << 17), EUNSUPPORTED, b"limits"),
]


@pytest.mark.parametrize("which,over,code,word", ERRORS)
def test_argument_errors_are_refused_on_the_host(which, over, code, word):
    from amk import lib as amk_lib

    L = amk_lib.load()
    assert _call(L, which, **over) == code
    assert word in L.amk_last_error(), L.amk_last_error()


def test_op_has_no_cpu_path_under_cpu_autocast():
    from amk import ops

    x, w, t = torch.randn(4, 8), torch.randn(5, 8), torch.zeros(4, dtype=torch.long)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.linear_cross_entropy(x, w, t, -1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.linear_cross_entropy(x.bfloat16(), w, t, -1)
        assert not ops.ce_head_ok(x, w)
