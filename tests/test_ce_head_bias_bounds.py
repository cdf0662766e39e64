"""The checker of tests/test_ce_head_bias_gpu.py and tests/test_ce_head_bias_bf16_gpu.py checks itself, without a GPU.

* The fp64 reference of tests/ce_head_bias_ref.py equals F.cross_entropy(F.linear(x, w, b), target, ignore_index) and its
  autograd in fp64 -- loss, dx, dw and db -- on every input family x bias family, with one row valid, no row valid and
  out-of-range targets.
* The emulation of the kernels' own order (bias preloaded into the logits' chain, the db chain of ce_bwd_db) stays under
  half of every hard bound and defines the constants Q_EMU of the tight tier, for the f32 and the bf16 head.
* Every planted fault is rejected on every input family x bias family at (129, 1000, 260) -- except that on the `zero`
  bias family bias_dropped, bias_shifted_by_one and bias_on_forward_only change nothing and so cannot show (no others),
  and that db_mean_over_M cannot show on needle+90 inputs under the needle bias, where db itself is below 2^-100.
* The library exports the four new entry points, the workspace sizes are the biasless ones (the header says so), and
  every argument error returns its code with a message before any device work; the op takes the keyword.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ce_head_bias_ref as ref

SHAPES = [(1, 1, 4), (127, 4, 36), (128, 127, 64), (129, 129, 4), (300, 128, 36), (129, 1000, 260), (300, 1000, 260),
          (300, 8192, 36)]
SHAPES16 = [(1, 1, 8), (127, 4, 40), (128, 127, 64), (129, 129, 8), (300, 128, 40), (129, 1000, 264), (300, 1000, 264),
            (300, 8192, 40)]
REJECT = {False: (129, 1000, 260), True: (129, 1000, 264)}
SMALL = {False: (127, 4, 36), True: (127, 4, 40)}
D_LOSS = 0.7
MODES = [False, True]
IDS = ["f32", "bf16"]
_CACHE = {}


def case(family, bfam, shape, bf16, mut=None, pattern=None):
    key = (family, bfam, shape, bf16, mut, pattern)
    if key not in _CACHE:
        M, V, K = shape
        pattern = pattern or ("all" if M == 1 else "random64")
        target = ref.make_target(M, V, pattern, seed=M + V)
        x, w = ref.make_inputs(family, M, V, K, target, seed=K, bf16=bf16)
        b = ref.make_bias(bfam, x, w, target, seed=V)
        rkey = (family, bfam, shape, bf16, "ref", pattern)
        if rkey not in _CACHE:
            _CACHE[rkey] = ref.reference(x, w, b, target, -1, D_LOSS, bf16=bf16)
        _CACHE[key] = (ref.emulate(x, w, b, target, -1, D_LOSS, mut, bf16=bf16), _CACHE[rkey], (x, w, b, target))
    return _CACHE[key]


def crossed(bf16):
    """Every input family x bias family at the reject shape and a small one; every shape class with the families
    rotating against each other."""
    out = [(f, bf, s) for f in ref.CPU_FAMILIES for bf in ref.BIAS_FAMILIES for s in (REJECT[bf16], SMALL[bf16])]
    shapes = SHAPES16 if bf16 else SHAPES
    for i, s in enumerate(shapes):
        for j, bf in enumerate(ref.BIAS_FAMILIES):
            c = (ref.CPU_FAMILIES[(i + 2 * j) % len(ref.CPU_FAMILIES)], bf, s)
            if c not in out:
                out.append(c)
    return out


def _torch_fp64(x, w, b, target):
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    loss = F.cross_entropy(F.linear(xd, wd, bd), target, ignore_index=-1)
    (loss * D_LOSS).backward()
    return loss.detach(), xd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("bf16", MODES, ids=IDS)
@pytest.mark.parametrize("bfam", ref.BIAS_FAMILIES)
def test_reference_equals_torch_fp64(bfam, bf16):
    for family in ref.CPU_FAMILIES:
        for shape in (REJECT[bf16], SMALL[bf16]):
            _, R, (x, w, b, target) = case(family, bfam, shape, bf16)
            for name, got in zip(ref.NAMES, _torch_fp64(x, w, b, target)):
                assert torch.allclose(R[name], got, rtol=1e-10, atol=1e-10), (family, bfam, shape, name)


@pytest.mark.parametrize("bfam", ref.BIAS_FAMILIES)
def test_reference_edge_semantics(bfam):
    """One row valid; no row valid (NaN loss, zero gradients, db included); an out-of-range target poisons the loss,
    takes and gives no gradient -- db included -- and is still counted in the mean's divisor."""
    M, V, K = 40, 12, 8
    t = ref.make_target(M, V, "all")
    x, w = ref.make_inputs("unit", M, V, K, t)
    b = ref.make_bias(bfam, x, w, t)
    one = ref.make_target(M, V, "first")
    R1 = ref.reference(x, w, b, one, -1, D_LOSS)
    for name, got in zip(ref.NAMES, _torch_fp64(x, w, b, one)):
        assert torch.allclose(R1[name], got, rtol=1e-11, atol=1e-12), name
    got = ref.emulate(x, w, b, one, -1, D_LOSS)
    assert all(ref.measures(g, R1, n)[0] == 0 for n, g in zip(ref.NAMES, got))
    none = torch.full((M,), -1)
    R0 = ref.reference(x, w, b, none, -1)
    assert torch.isnan(R0["loss"]) and not R0["dx"].any() and not R0["dw"].any() and not R0["db"].any()
    loss, dx, dw, db = ref.emulate(x, w, b, none, -1)
    assert torch.isnan(loss) and not dx.any() and not dw.any() and not db.any()
    bad = t.clone()
    bad[3], bad[7] = V + 2, -5
    Rb = ref.reference(x, w, b, bad, -1)
    dropped = t.clone()
    dropped[3] = dropped[7] = -1
    Rd = ref.reference(x, w, b, dropped, -1)
    assert torch.isnan(Rb["loss"]) and Rb["count"] == M and Rd["count"] == M - 2
    assert not Rb["dx"][3].any() and not Rb["dx"][7].any()
    assert torch.allclose(Rb["dw"] * M, Rd["dw"] * (M - 2), rtol=1e-12, atol=1e-15)
    assert torch.allclose(Rb["db"] * M, Rd["db"] * (M - 2), rtol=1e-12, atol=1e-15)
    loss, dx, dw, db = ref.emulate(x, w, b, bad, -1)
    assert torch.isnan(loss) and not dx[3].any() and not dx[7].any()
    assert all(ref.measures(g, Rb, n)[0] == 0 for n, g in (("dx", dx), ("dw", dw), ("db", db)))


@pytest.mark.parametrize("bf16", MODES, ids=IDS)
def test_emulation_within_half_the_hard_bound(bf16):
    for family, bfam, shape in crossed(bf16):
        got, R, _ = case(family, bfam, shape, bf16)
        for name, g in zip(ref.NAMES, got):
            nbad, ratio, q = ref.measures(g, R, name)
            what = f"{family} x {bfam} {shape} {name}"
            assert nbad == 0 and ratio <= 0.5, f"{what}: the emulation reaches {ratio:.3f} of the hard bound"
            assert q <= ref.Q_EMU[bf16][name], f"{what}: q {q:.3f} above Q_EMU = {ref.Q_EMU[bf16][name]}"


@pytest.mark.parametrize("bf16", MODES, ids=IDS)
def test_emulation_defines_q(capsys, bf16):
    """Q_EMU is the emulation's worst q per output over every case of crossed(), rounded up by at most a tenth."""
    worst = {}
    for family, bfam, shape in crossed(bf16):
        got, R, _ = case(family, bfam, shape, bf16)
        for name, g in zip(ref.NAMES, got):
            worst[name] = max(worst.get(name, 0.0), ref.measures(g, R, name)[2])
    with capsys.disabled():
        print(f"\nemulation worst q ({'bf16' if bf16 else 'f32'}):", {k: round(v, 4) for k, v in worst.items()})
    for name, q in worst.items():
        have = ref.Q_EMU[bf16][name]
        assert q <= have <= 1.1 * q, f"Q_EMU[{name}] = {have} against the emulation's {q:.4f}"


@pytest.mark.parametrize("bf16", MODES, ids=IDS)
@pytest.mark.parametrize("bfam", ref.BIAS_FAMILIES)
@pytest.mark.parametrize("fault", ref.FAULTS)
def test_planted_fault_is_rejected(fault, bfam, bf16):
    for family in ref.CPU_FAMILIES:
        got, R, _ = case(family, bfam, REJECT[bf16], bf16)
        assert sum(ref.violations(g, R, n, bf16) for n, g in zip(ref.NAMES, got)) == 0
        bad, R, _ = case(family, bfam, REJECT[bf16], bf16, fault)
        flagged = [n for n, g in zip(ref.NAMES, bad) if ref.measures(g, R, n)[0] > 0]
        if bfam == "zero" and fault in ref.NEED_A_BIAS:
            assert all(torch.equal(a, b) or (bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()))
                       for a, b in zip(got, bad)), f"{fault} changes a result on a zero bias"
            continue
        if fault == "db_mean_over_M" and not flagged:
            # a scaling of db cannot show where db itself vanishes: needle+90 inputs under the needle bias put every
            # target at least 120 ahead of every word that is nobody's target, and the whole of the fp64 db lies under
            # 2^-100, where the bound is the allowance for weights flushed to zero.  Nowhere else.
            assert (family, bfam) == ("needle+90", "needle") and float(R["db"].abs().max()) < 2.0 ** -100
            continue
        assert flagged, f"{fault} on {family} x {bfam} stays inside every hard bound"


def test_the_faults_excused_on_a_zero_bias():
    assert set(ref.NEED_A_BIAS) == {"bias_dropped", "bias_shifted_by_one", "bias_on_forward_only"}
    assert set(ref.FAULTS) - set(ref.NEED_A_BIAS) == {"db_over_all_rows", "db_mean_over_M"}


def test_db_chain_length():
    assert [ref.n_db(c) for c in (1, 32, 33, 129)] == [6, 6, 7, 10]


# ---------------------------------------------------------------------------------------------- the ABI without a GPU
NEW = ("amk_ce_head_bias_fwd", "amk_ce_head_bias_bwd", "amk_ce_head_bias_bf16_fwd", "amk_ce_head_bias_bf16_bwd")


def test_library_exports_the_biased_loss_head():
    from amk import lib as amk_lib

    L = amk_lib.load()
    declared = amk_lib.declared_symbols()
    for name in NEW:
        assert hasattr(L, name) and name in amk_lib.SIGNATURES and name in declared
    # the header: db needs no workspace of its own, the biasless sizes apply (and are what they were)
    assert not any("bias" in n and "ws_bytes" in n for n in declared)
    M, V, K = 300, 8192, 1024
    ns, _ = ref.slices(M, V)
    assert L.amk_ce_head_fwd_ws_bytes(M, V, K) == L.amk_ce_head_bf16_fwd_ws_bytes(M, V, K) == 3 * M * ns * 4
    assert L.amk_ce_head_bwd_ws_bytes(M, V, K) == M * 8192 * 4 and L.amk_ce_head_bf16_bwd_ws_bytes(M, V, K) == M * 8192 * 2
    assert L.amk_ce_head_bwd_ws_bytes(129, 1000, 260) == 129 * 1024 * 4


def _call(L, which, bf16, **over):
    """One entry point with plausible (never dereferenced) addresses; `over` replaces arguments by name."""
    P = ctypes.c_void_p
    a = dict(x=1 << 20, ldx=64, w=2 << 20, ldw=64, bias=11 << 20, target=3 << 20, ignore_index=-1, M=128, V=100, K=64,
             loss=4 << 20, d_loss=4 << 20, lse=5 << 20, rows=6 << 20, count=7 << 20, dx=8 << 20, lddx=64, dw=9 << 20, lddw=64,
             dbias=12 << 20, ws=10 << 20, ws_bytes=1 << 30)
    a.update(over)
    p = {k: P(v) for k, v in a.items() if isinstance(v, int) and k in ("x", "w", "bias", "target", "loss", "d_loss", "lse", "rows",
                                                                      "count", "dx", "dw", "dbias", "ws")}
    if which == "fwd":
        fn = L.amk_ce_head_bias_bf16_fwd if bf16 else L.amk_ce_head_bias_fwd
        return fn(p["x"], a["ldx"], p["w"], a["ldw"], p["bias"], p["target"], a["ignore_index"], a["M"], a["V"], a["K"], p["loss"],
                  p["lse"], p["rows"], p["count"], p["ws"], a["ws_bytes"], P(0))
    fn = L.amk_ce_head_bias_bf16_bwd if bf16 else L.amk_ce_head_bias_bwd
    return fn(p["x"], a["ldx"], p["w"], a["ldw"], p["bias"], p["target"], a["ignore_index"], a["M"], a["V"], a["K"], p["d_loss"],
              p["lse"], p["rows"], p["count"], p["dx"], a["lddx"], p["dw"], a["lddw"], p["dbias"], p["ws"], a["ws_bytes"], P(0))


EINVAL, EUNSUPPORTED = -1, -2
ERRORS = [
    ("fwd", dict(bias=0), EINVAL, b"null"), ("bwd", dict(bias=0), EINVAL, b"null"), ("bwd", dict(dbias=0), EINVAL, b"null"),
    ("fwd", dict(bias=(11 << 20) + 4), EINVAL, b"misaligned"), ("bwd", dict(bias=(11 << 20) + 8), EINVAL, b"misaligned"),
    ("bwd", dict(dbias=(12 << 20) + 4), EINVAL, b"misaligned"),
    ("fwd", dict(x=0), EINVAL, b"null"), ("bwd", dict(dw=0), EINVAL, b"null"),
    ("fwd", dict(M=0), EINVAL, b"non-positive"), ("bwd", dict(K=0), EINVAL, b"non-positive"),
    ("fwd", dict(x=(1 << 20) + 4), EINVAL, b"misaligned"), ("bwd", dict(dx=(8 << 20) + 4), EINVAL, b"misaligned"),
    ("fwd", dict(ws_bytes=16), EINVAL, b"workspace"), ("bwd", dict(ws_bytes=128 * 128 * 2 - 1), EINVAL, b"workspace"),
    ("fwd", dict(ldx=56), EINVAL, b"below K"), ("bwd", dict(lddw=56), EINVAL, b"below K"),
    ("fwd", dict(K=62, ldx=64), EUNSUPPORTED, b"multiple of"), ("bwd", dict(lddx=66), EUNSUPPORTED, b"multiples of"),
    ("fwd", dict(M=(1 << 24) + 1), EUNSUPPORTED, b"limits"), ("bwd", dict(V=(1 << 22) + 1), EUNSUPPORTED, b"limits"),
    ("fwd", dict(K=(1 << 16) + 8, ldx=1 << 17, ldw=1 << 17), EUNSUPPORTED, b"limits"),
]


@pytest.mark.parametrize("bf16", MODES, ids=IDS)
@pytest.mark.parametrize("which,over,code,word", ERRORS)
def test_argument_errors_are_refused_on_the_host(which, over, code, word, bf16):
    from amk import lib as amk_lib

    L = amk_lib.load()
    assert _call(L, which, bf16, **over) == code
    msg = L.amk_last_error()
    assert word in msg and (b"amk_ce_head_bias_bf16_" if bf16 else b"amk_ce_head_bias_") + which.encode() in msg, msg


def test_op_takes_a_bias_and_has_no_cpu_path():
    from amk import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_cross_entropy(torch.randn(4, 8), torch.randn(5, 8), torch.zeros(4, dtype=torch.long), -1,
                                 bias=torch.randn(5))
    assert not ops.ce_head_ok(torch.randn(4, 8), torch.randn(5, 8), torch.randn(5))
    assert not ops.ce_head_ok(torch.randn(4, 8), torch.randn(5, 8), bias=None)
