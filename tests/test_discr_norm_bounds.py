"""The per-element bounds of tests/discr_norm_ref.py, checked without a GPU: the CPU emulation of csrc/discr_norm.hip stays
under half of every bound on every family and shape, the reference alone keeps the kink set within its cap on every case of
this file and of tests/test_discr_norm_bounds_gpu.py, planted defects fall outside, the exact cases are exact, and the
geometry restatement agrees with the library's workspace size."""
import pytest
import torch

import discr_norm_ref as ref

CAP = 0.5

RAGGED, PIECES, LONG = (5, 4, 31, 31), (2, 3, 65, 65), (300, 2, 3, 683)
KEPT = [sh for sh in ref.CPU_SHAPES if sh != LONG]      # the shapes several tests share; a reference holds 25 arrays like x
_CACHE = {}
_LAST = [None, None]
EMULATION_WORST = {}


def _case(family, shape):
    """(inputs, reference), never modified: kept for the module on the small shapes the tests share, one at a time otherwise
    (the six families at LONG would hold 0.8 GB)."""
    key = (family, shape)
    if key in _CACHE:
        return _CACHE[key]
    if _LAST[0] != key:
        inp = ref.make_inputs(family, shape)
        _LAST[:] = [key, (inp, ref.reference(inp, family))]
    if shape in KEPT:
        _CACHE[key] = _LAST[1]
    return _LAST[1]


def _ch(t):
    return t.view(1, -1, 1, 1)


@pytest.mark.parametrize("shape", ref.CPU_SHAPES)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_emulation_stays_under_half_of_every_bound(family, shape):
    inp, R = _case(family, shape)
    q = ref.ratios(ref.emulate(inp), R, record=False)
    print(family, shape, {k: round(v, 4) for k, v in q.items()})
    for name, v in q.items():
        EMULATION_WORST[(family, name)] = max(EMULATION_WORST.get((family, name), 0.0), v)
    for name in ref.TENSORS:
        assert torch.isfinite(R["bound_" + name]).all(), name      # delta < 0.9 on every family: no bound is inf
        assert q[name] <= CAP, (name, q[name])
    for name in ref.TWO_BRANCH:
        assert torch.isfinite(R["bound_alt_" + name]).all(), name


@pytest.mark.parametrize("shape", ref.CPU_SHAPES + ref.GPU_SHAPES)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_reference_alone_keeps_the_kink_set_within_its_cap(family, shape):
    inp, R = _case(family, shape)             # reference() asserts the cap
    cap = ref.KINK_CAP.get(family, ref.KINK_CAP_DEFAULT)
    print(family, shape, "kink", R["kink"], "of", inp["x"].numel())
    assert R["kink"] <= cap * inp["x"].numel()
    assert ref.KINK_CAP_DEFAULT == 1e-4 and set(ref.KINK_CAP) == {"offset"}


@pytest.mark.parametrize("mut,family,shape,tensors", [
    ("tail_dropped", "diffuse", RAGGED, ("mean", "z", "dbeta")),
    ("tail_dropped", "mean_heavy", PIECES, ("mean", "g_gamma")),
    ("chan_no_cross_term", "sparse_cotangent", LONG, ("rstd", "z", "run_var")),
    ("chan_no_cross_term", "diffuse", PIECES, ("rstd",)),
    ("biased_running_var", "diffuse", RAGGED, ("run_var",)),
    ("biased_running_var", "diffuse", (2, 3, 1, 1), ("run_var",)),
    ("uncentred_variance", "offset", RAGGED, ("rstd", "z", "gx")),
    ("uncentred_variance", "offset", LONG, ("rstd", "z")),
    ("sign_from_xhat", "diffuse", RAGGED, ("gx", "dbeta", "g_gz", "g_x")),
    ("sign_from_xhat", "dead_channel", (2, 3, 1, 1), ("dbeta", "g_gz")),
    ("g_gz_without_slope", "diffuse", RAGGED, ("g_gz",)),
    ("g_gz_without_slope", "mean_heavy", LONG, ("g_gz",)),
    ("k1_with_2BD", "diffuse", RAGGED, ("g_x",)),
    ("k1_with_2BD", "mean_heavy", PIECES, ("g_x",)),
    ("fold_first_256_only", "diffuse", LONG, ("mean", "rstd", "dgamma", "dbeta", "g_gamma")),
    ("fold_first_256_only", "mean_heavy", LONG, ("mean", "dbeta", "g_gamma")),
    ("last_segment_dropped", "diffuse", RAGGED, ("mean", "rstd", "run_var", "z")),
    ("last_segment_dropped", "offset", RAGGED, ("rstd", "z")),
])
def test_planted_defects_fall_outside_the_bound(mut, family, shape, tensors):
    inp, R = _case(family, shape)
    N, C, H, W = shape
    if mut == "fold_first_256_only":
        assert ref.make_geo(N, C, H * W)["S"] > ref.BLOCK
    if mut == "last_segment_dropped":
        assert ref.is_ragged(N, C, H * W)
    if mut == "tail_dropped":
        assert any(tail for c in range(C) for s in range(ref.make_geo(N, C, H * W)["S"])
                   for _, _, _, tail in ref.plane_walk(ref.make_geo(N, C, H * W), c, s))
    q = ref.ratios(ref.emulate(inp, mut=mut), R, record=False)
    clean = ref.ratios(ref.emulate(inp), R, record=False)
    print(mut, family, shape, {k: round(v, 3) for k, v in q.items()})
    for name in tensors:
        assert clean[name] <= CAP
        assert q[name] > 1.0, (mut, name, q[name])


def _leaky(b):
    b = torch.as_tensor(b, dtype=torch.float32)
    return torch.where(b > 0, b, torch.tensor(ref.SLOPE, dtype=torch.float32) * b)


@pytest.mark.parametrize("shape", ref.CPU_SHAPES)
def test_dead_channels_are_exact_in_the_emulation(shape):
    inp, _ = _case("dead_channel", shape)
    got = ref.emulate(inp)
    dead = ref.dead_channels("dead_channel", shape[1], shape[2] * shape[3])
    assert dead
    xh = (inp["x"] - _ch(got["mean"])) * _ch(got["rstd"])
    t = _ch(inp["gg_gamma"]) * xh + _ch(inp["gg_beta"])
    for c, b in dead.items():
        assert float(inp["gamma"][c]) == 0.0 and float(inp["beta"][c]) == torch.tensor(b, dtype=torch.float32)
        assert torch.equal(got["z"][:, c], _leaky(b).expand_as(got["z"][:, c])), c
        assert not bool(got["gx"][:, c].any()), c
        want = t[:, c] if b > 0 else torch.tensor(ref.SLOPE, dtype=torch.float32) * t[:, c]
        assert torch.equal(got["g_gz"][:, c], want), c


@pytest.mark.parametrize("shape", ref.CPU_SHAPES)
def test_flat_channels_are_exact_in_the_emulation(shape):
    """mean == the constant for every flat channel; z == leaky_relu(beta) to the bit where the constant is 0 (for another
    constant shift rounds at |c gamma| eps^-1/2 and z is held to its bound: see the module docstring of discr_norm_ref)."""
    inp, R = _case("flat_channel", shape)
    got = ref.emulate(inp)
    flat = ref.flat_channels("flat_channel", shape[1])
    assert flat
    for c, v in flat.items():
        assert bool((inp["x"][:, c] == v).all())
        assert float(got["mean"][c]) == v, c
        assert float(got["rstd"][c]) == float(torch.rsqrt(torch.tensor(ref.EPS, dtype=torch.float32))), c
        if v == 0.0:
            assert torch.equal(got["z"][:, c], _leaky(inp["beta"][c]).expand_as(got["z"][:, c])), c


@pytest.mark.parametrize("shape", ref.CPU_SHAPES + ref.GPU_SHAPES)
def test_geometry_restatement_gives_the_library_workspace(shape):
    from amk import lib

    N, C, H, W = shape
    g = ref.make_geo(N, C, H * W)
    assert C * g["S"] * 3 == ref.ws_floats(N, C, H * W) == lib.load().amk_bnact_ws_floats(N, C, H * W)
    # every element of a channel belongs to exactly one segment, and the walks cover it once
    segid, cnt = ref._segmap(N, C, H * W)
    assert int(cnt.sum()) == N * H * W and segid.numel() == N * H * W
    idx = ref._plan(N, C, H * W)
    seen = idx[idx < N * C * H * W]
    assert seen.numel() == N * C * H * W and seen.unique().numel() == N * C * H * W


def test_geometry_of_the_named_shapes():
    geo = lambda N, C, H, W: ref.make_geo(N, C, H * W)  # noqa: E731
    g = geo(5, 4, 31, 31)
    assert (g["PP"], g["S"]) == (4, 2) and ref.seg_of(g, 1)[:2] == (4, 5) and ref.is_ragged(5, 4, 961)
    g = geo(2, 3, 65, 65)
    assert (g["Q"], g["S"]) == (2, 4) and g["HW"] % 2 == 1
    assert len({ref.plane_walk(g, 1, s)[0][1] for s in range(4)}) > 1          # the head changes from piece to piece
    g = geo(300, 2, 3, 683)
    assert (g["HW"], g["PP"], g["S"]) == (2049, 1, 300) and g["S"] > ref.BLOCK
    g = geo(9, 3, 33, 31)
    assert (g["HW"], g["PP"], g["S"]) == (1023, 4, 3) and [ref.seg_count(g, s) // 1023 for s in range(3)] == [4, 4, 1]
    assert len({h for s in range(3) for _, h, _, _ in ref.plane_walk(g, 0, s)}) == 4
    assert (geo(2, 5, 64, 64)["Q"], geo(2, 5, 64, 64)["S"]) == (1, 2) and geo(2, 3, 64, 65)["Q"] == 2
    assert ref.depths(3, 7, 1)[0] == 3 + 9                                    # HW == 1: thread 0 adds every plane


def test_zz_report_emulation_worst_ratios(capsys):
    """The figures of the "Measured" block of discr_norm_ref's docstring: per family, and over all of them."""
    with capsys.disabled():
        for family in ref.FAMILIES:
            print("\ndiscr_norm emulation worst,", family, {n: round(EMULATION_WORST.get((family, n), 0.0), 4) for n in ref.TENSORS},
                  end="")
        print()
    assert all(v <= CAP for v in EMULATION_WORST.values())
