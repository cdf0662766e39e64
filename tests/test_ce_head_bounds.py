"""The checker of tests/test_ce_head_gpu.py checks itself, without a GPU.

* The fp64 reference of tests/ce_head_ref.py equals F.cross_entropy(F.linear(x, w), target, ignore_index) and its
  autograd in fp64.
* An f32 emulation of csrc/ce_head.hip in the kernels' own order stays under half of every hard bound on every family
  and shape class and defines the constants Q_EMU of the tight tier.
* The bounds reject, on at least one tensor in every family at (129, 1000, 260): operands rounded to bf16, the mean taken
  over M instead of over count, ignore_index not honoured, and a target column off by one.
* The library exports the four entry points, and every argument error returns its code with a message before any
  device work (no GPU is needed).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ce_head_ref as ref

SHAPES = [(1, 1, 4), (127, 4, 36), (128, 127, 64), (129, 129, 4), (300, 128, 36), (129, 1000, 260), (300, 1000, 260),
          (300, 8192, 36)]   # (the last: four tiles per slice, sixteen slices, the longest dx chain of the GPU cases)
REJECT_SHAPE = (129, 1000, 260)
D_LOSS = 0.7
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
    for shape in ((129, 1000, 260), (127, 4, 36)):
        _, R, (x, w, target) = case(family, shape)
        xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
        loss = F.cross_entropy(F.linear(xd, wd), target, ignore_index=-1)
        (loss * D_LOSS).backward()
        for name, got in (("loss", loss.detach()), ("dx", xd.grad), ("dw", wd.grad)):
            assert torch.allclose(R[name], got, rtol=1e-11, atol=1e-11), (family, shape, name)  # (large: dx[:, 0] = 100 sum_v g cancels)


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
    assert torch.isnan(loss) and not dx[3].any() and not dx[7].any()
    assert ref.measures(dw, Rb, "dw")[0] == 0 and ref.measures(dx, Rb, "dx")[0] == 0
    loss, dx, dw = ref.emulate(x, w, torch.full((M,), -1), -1)
    assert torch.isnan(loss) and not dx.any() and not dw.any()


@pytest.mark.parametrize("family", ref.CPU_FAMILIES)
def test_emulation_within_half_the_hard_bound(family):
    for shape in SHAPES:
        got, R, _ = case(family, shape)
        for name, g in zip(("loss", "dx", "dw"), got):
            nbad, ratio, q = ref.measures(g, R, name)
            assert nbad == 0 and ratio <= 0.5, f"{family} {shape} {name}: the emulation reaches {ratio:.3f} of the hard bound"
            assert q <= ref.Q_EMU[name], f"{family} {shape} {name}: q {q:.3f} above Q_EMU = {ref.Q_EMU[name]}"


def test_emulation_defines_q(capsys):
    """Q_EMU is the emulation's worst q per output over every family and shape class, rounded up by at most a tenth."""
    worst = {}
    for family in ref.CPU_FAMILIES:
        for shape in SHAPES:
            got, R, _ = case(family, shape)
            for name, g in zip(("loss", "dx", "dw"), got):
                worst[name] = max(worst.get(name, 0.0), ref.measures(g, R, name)[2])
    with capsys.disabled():
        print("\nemulation worst q:", {k: round(v, 4) for k, v in worst.items()})
    for name, q in worst.items():
        assert q <= ref.Q_EMU[name] <= 1.1 * q, f"Q_EMU[{name}] = {ref.Q_EMU[name]} against the emulation's {q:.4f}"


@pytest.mark.parametrize("family", ref.CPU_FAMILIES)
@pytest.mark.parametrize("fault", ["bf16", "mean_over_M", "ignore_not_honoured", "target_off_by_one"])
def test_planted_fault_is_rejected(fault, family):
    got, R, _ = case(family, REJECT_SHAPE)
    assert sum(ref.violations(g, R, n) for n, g in zip(("loss", "dx", "dw"), got)) == 0
    bad, R, _ = case(family, REJECT_SHAPE, fault)
    flagged = [n for n, g in zip(("loss", "dx", "dw"), bad) if ref.measures(g, R, n)[0] > 0]
    assert flagged, f"{fault} on {family} inputs stays inside every hard bound"


def test_slices_cover_the_vocabulary():
    for M, V in ((1, 1), (300, 8192), (8192, 8192), (129, 1000), (127, 129), (100000, 50000), (5, 2049)):
        ns, vper = ref.slices(M, V)
        assert vper % ref.TILE == 0 and 1 <= ns <= 16 and (ns - 1) * vper < V <= ns * vper


# ---------------------------------------------------------------------------------------------- the ABI without a GPU
def test_library_exports_the_loss_head():
    from amk import lib as amk_lib

    L = amk_lib.load()
    for name in ("amk_ce_head_fwd_ws_bytes", "amk_ce_head_bwd_ws_bytes", "amk_ce_head_fwd", "amk_ce_head_bwd"):
        assert hasattr(L, name) and name in amk_lib.SIGNATURES
    M, V, K = 300, 8192, 1024
    ns, _ = ref.slices(M, V)
    assert L.amk_ce_head_fwd_ws_bytes(M, V, K) == 3 * M * ns * 4
    assert L.amk_ce_head_bwd_ws_bytes(M, V, K) == M * 8192 * 4
    assert L.amk_ce_head_bwd_ws_bytes(129, 1000, 260) == 129 * 1024 * 4
    assert L.amk_ce_head_fwd_ws_bytes(0, V, K) == 0 and L.amk_ce_head_bwd_ws_bytes(M, -1, K) == 0


def _call(L, which, **over):
    """One entry point with plausible (never dereferenced) addresses; `over` replaces arguments by name."""
    P = ctypes.c_void_p
    a = dict(x=1 << 20, ldx=64, w=2 << 20, ldw=64, target=3 << 20, ignore_index=-1, M=128, V=100, K=64, loss=4 << 20,
             d_loss=4 << 20, lse=5 << 20, rows=6 << 20, count=7 << 20, dx=8 << 20, lddx=64, dw=9 << 20, lddw=64,
             ws=10 << 20, ws_bytes=1 << 30)
    a.update(over)
    p = {k: P(v) for k, v in a.items() if k in ("x", "w", "target", "loss", "d_loss", "lse", "rows", "count", "dx", "dw", "ws")}
    if which == "fwd":
        return L.amk_ce_head_fwd(p["x"], a["ldx"], p["w"], a["ldw"], p["target"], a["ignore_index"], a["M"], a["V"], a["K"],
                                 p["loss"], p["lse"], p["rows"], p["count"], p["ws"], a["ws_bytes"], P(0))
    return L.amk_ce_head_bwd(p["x"], a["ldx"], p["w"], a["ldw"], p["target"], a["ignore_index"], a["M"], a["V"], a["K"],
                             p["d_loss"], p["lse"], p["rows"], p["count"], p["dx"], a["lddx"], p["dw"], a["lddw"], p["ws"],
                             a["ws_bytes"], P(0))


EINVAL, EUNSUPPORTED = -1, -2
ERRORS = [
    ("fwd", dict(x=0), EINVAL, b"null"), ("fwd", dict(count=0), EINVAL, b"null"), ("bwd", dict(d_loss=0), EINVAL, b"null"),
    ("bwd", dict(dw=0), EINVAL, b"null"),
    ("fwd", dict(M=0), EINVAL, b"non-positive"), ("fwd", dict(V=-3), EINVAL, b"non-positive"),
    ("bwd", dict(K=0), EINVAL, b"non-positive"),
    ("fwd", dict(x=(1 << 20) + 4), EINVAL, b"misaligned"), ("fwd", dict(ws=(10 << 20) + 8), EINVAL, b"misaligned"),
    ("bwd", dict(dx=(8 << 20) + 4), EINVAL, b"misaligned"), ("bwd", dict(target=(3 << 20) + 4), EINVAL, b"misaligned"),
    ("fwd", dict(ws_bytes=16), EINVAL, b"workspace"), ("bwd", dict(ws_bytes=128 * 128 * 4 - 1), EINVAL, b"workspace"),
    ("fwd", dict(ldx=60), EINVAL, b"below K"), ("bwd", dict(lddw=60), EINVAL, b"below K"),
    ("fwd", dict(K=62, ldx=64), EUNSUPPORTED, b"multiple of 4"), ("fwd", dict(ldx=66), EUNSUPPORTED, b"multiples of 4"),
    ("bwd", dict(ldw=70), EUNSUPPORTED, b"multiples of 4"), ("bwd", dict(lddx=66), EUNSUPPORTED, b"multiples of 4"),
    ("bwd", dict(lddw=70), EUNSUPPORTED, b"multiples of 4"),
    ("fwd", dict(M=(1 << 24) + 1), EUNSUPPORTED, b"limits"), ("bwd", dict(V=(1 << 22) + 1), EUNSUPPORTED, b"limits"),
    ("fwd", dict(K=(1 << 16) + 4, ldx=1 << 17, ldw=1 << 17), EUNSUPPORTED, b"limits"),
]


@pytest.mark.parametrize("which,over,code,word", ERRORS)
def test_argument_errors_are_refused_on_the_host(which, over, code, word):
    from amk import lib as amk_lib

    L = amk_lib.load()
    assert _call(L, which, **over) == code
    assert word in L.amk_last_error(), L.amk_last_error()


def test_op_has_no_cpu_path():
    from amk import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_cross_entropy(torch.randn(4, 8), torch.randn(5, 8), torch.zeros(4, dtype=torch.long), -1)
