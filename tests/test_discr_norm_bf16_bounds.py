"""tests/discr_norm_bf16_ref.py without a GPU: the CPU emulation of the bf16 BatchNorm + LeakyReLU kernels (f32 torch ops in
the kernels' order on the bf16 walk, z, gx, g_gz and g_x rounded to bf16 once) keeps its f32 values under HALF of every f32
bound and its rounded outputs inside RNE's image of the bound; the fp64 reference alone keeps the kink set within its cap on
every case of this file and of tests/test_discr_norm_bf16_gpu.py; defects planted in the walk, in the rounding or in the
fp64 spec land outside; the geometry restatement; and the refusals of amk_bnact_bf16_*, which need no device memory."""
import ctypes

import pytest
import torch

import discr_norm_bf16_ref as bref
import discr_norm_ref as ref
from bf16_dense_ref import bf16_round

F32, F64 = torch.float32, torch.float64
CAP = 0.5
RAGGED, PIECES, LONG, EDGES, ODD_PIECES = (5, 4, 31, 31), (2, 3, 65, 65), (300, 2, 3, 683), (3, 5, 3, 5), (1, 2, 67, 67)
KEPT = [sh for sh in bref.SHAPES if sh != LONG]
_CACHE = {}
_LAST = [None, None]
EMU_WORST = {}


def _case(family, shape):
    """(inputs, reference), never modified: kept for the module on the small shapes, one at a time at LONG."""
    key = (family, shape)
    if key in _CACHE:
        return _CACHE[key]
    if _LAST[0] != key:
        inp = bref.make_inputs(family, shape)
        _LAST[:] = [key, (inp, bref.reference(inp, family))]
    if shape in KEPT:
        _CACHE[key] = _LAST[1]
    return _LAST[1]


def _rounded(f32):
    return dict(f32, **{name: bf16_round(f32[name]) for name in bref.ROUNDED})


# ---------------------------------------------------------------------------------------------- geometry
def test_geometry_of_the_bf16_walk():
    geo = lambda N, C, H, W: bref.make_geo(N, C, H * W)  # noqa: E731
    g = geo(*ODD_PIECES)
    assert (g["Q"], g["L"], g["S"]) == (2, 2248, 2) and g["L"] % 8 == 0
    assert [ref.seg_of(g, s)[3] - ref.seg_of(g, s)[2] for s in range(2)] == [2248, 2241]
    g = geo(*PIECES)
    assert (g["Q"], g["S"]) == (2, 4) and g["L"] == 2120 and ref.make_geo(2, 3, 4225)["L"] == 2116
    # HW = 15: the plane bases fall on every residue mod 8, so heads of 0 to 7 all occur
    g = geo(*EDGES)
    walks = [w for c in range(5) for s in range(g["S"]) for w in bref.plane_walk(g, c, s)]
    assert {h for _, h, _, _ in walks} == set(range(8)) and {b % 8 for b, _, _, _ in walks} == set(range(8))
    # HW = 7: no body at all
    g = geo(2, 3, 7, 1)
    assert all(nv == 0 for c in range(3) for s in range(g["S"]) for _, _, nv, _ in bref.plane_walk(g, c, s))
    # a full one-plane segment is two body trips of eight adds and one edge add
    assert bref.depths(2, 5, 4096)[0] == 17 + 9 and ref.depths(2, 5, 4096)[0] == 17 + 9
    assert bref.depths(3, 7, 1)[0] == 3 + 9


@pytest.mark.parametrize("shape", bref.SHAPES)
def test_geometry_restatement_gives_the_library_workspace(shape):
    from amk import lib

    N, C, H, W = shape
    g = bref.make_geo(N, C, H * W)
    assert g["S"] == ref.make_geo(N, C, H * W)["S"] and g["Q"] == ref.make_geo(N, C, H * W)["Q"]
    assert C * g["S"] * 3 == bref.ws_floats(N, C, H * W) == lib.load().amk_bnact_ws_floats(N, C, H * W)
    segid, cnt = bref._segmap(N, C, H * W)
    assert int(cnt.sum()) == N * H * W and segid.numel() == N * H * W
    idx = bref._plan(N, C, H * W)
    seen = idx[idx < N * C * H * W]
    assert seen.numel() == N * C * H * W and seen.unique().numel() == N * C * H * W


# ---------------------------------------------------------------------------------------------- inputs and the kink cap
@pytest.mark.parametrize("shape", bref.SHAPES)
@pytest.mark.parametrize("family", bref.FAMILIES)
def test_reference_alone_keeps_the_kink_set_within_its_cap(family, shape):
    inp, R = _case(family, shape)             # reference() asserts the cap
    for k in bref.BF16_INPUTS:
        assert torch.equal(inp[k], bf16_round(inp[k])), k
    for k in ("gamma", "beta", "gg_gamma", "gg_beta"):
        assert inp[k].dtype == F32
    cap = bref.KINK_CAP.get(family, bref.KINK_CAP_DEFAULT)
    print(family, shape, "kink", R["kink"], "of", inp["x"].numel())
    assert R["kink"] <= cap * inp["x"].numel()
    assert bref.KINK_CAP_DEFAULT == 1e-4 and bref.KINK_CAP == {"offset": 4e-3}


def test_offset_keeps_a_distribution_on_the_bf16_grid():
    """x = RNE(100 + 2 N(0, 1)): |mu| r about 50 and far more than the one or two distinct values per channel that rounding
    discr_norm_ref's 100 + 0.1 N(0, 1) leaves."""
    inp, R = _case("offset", RAGGED)
    for c in range(RAGGED[1]):
        assert inp["x"][:, c].unique().numel() >= 12
        assert 30 < abs(float(R["mean"][c] * R["rstd"][c])) < 80
    plain = bf16_round(ref.make_inputs("offset", RAGGED)["x"])
    assert max(plain[:, c].unique().numel() for c in range(RAGGED[1])) <= 3


# ---------------------------------------------------------------------------------------------- the emulation
@pytest.mark.parametrize("shape", bref.CPU_SHAPES)
@pytest.mark.parametrize("family", bref.FAMILIES)
def test_emulation_stays_under_half_of_every_bound(family, shape):
    inp, R = _case(family, shape)
    f32 = bref.emulate_f32(inp)
    q32 = ref.ratios(f32, R, record=False)                      # every tensor before the store, against b32
    q = bref.ratios(_rounded(f32), R, record=False)
    print(family, shape, {k: round(v, 4) for k, v in q32.items()}, {k: round(q[k], 4) for k in bref.ROUNDED})
    for name in bref.TENSORS:
        assert bool(torch.isfinite(R["bound_" + name]).all()), f"{name} has no bound somewhere"
        assert q32[name] <= CAP, f"{family} {shape}: the emulation's f32 {name} at {q32[name]:.3f} of its bound"
        EMU_WORST[name] = max(EMU_WORST.get(name, 0.0), q32[name] if name not in bref.ROUNDED else q[name])
    assert not bref.outside(_rounded(f32), R)
    for name in bref.ROUNDED:
        assert bool((R["lo_" + name] <= R["hi_" + name]).all())


def test_zz_report_emulation_worst(capsys):
    with capsys.disabled():
        print("\ndiscr_norm_bf16 emulation worst ratios:", {k: round(v, 4) for k, v in sorted(EMU_WORST.items())})
    assert all(v <= 1.0 for v in EMU_WORST.values())


# ---------------------------------------------------------------------------------------------- the bounds are not vacuous
def _truncate(v):
    """f32 -> bf16 by dropping the low 16 bits."""
    return (v.to(F32).contiguous().view(torch.int32) & -65536).view(F32)


def _c(v):
    return v.view(1, -1, 1, 1)


def _spec(inp, mut=None):
    """What a kernel with one defect would compute, in fp64 from the formulas of tests/discr_norm_spec.py (every tensor of
    bref.TENSORS, before the store).  mut:
      "stats_of_bf16_centred"  the statistics' second pass squares a centred value rounded to bf16;
      "sums_of_bf16_y"         the channel sums take xh back from a y rounded to bf16, xh = (RNE(y) - beta) / gamma;
      "s_from_rounded_z"       s is taken from the rounded z as RNE(z) / y (its SIGN alone is the sign of the f32 y wherever that
                               is determined, which no test could tell apart and none needs to; the defect is the value);
      "g_x_D_B_swapped"        g_x with D and B exchanged."""
    x, gz, ggx, gam, bet, ggg, ggb = (inp[k].to(F64) for k in ("x", "gz", "ggx", "gamma", "beta", "gg_gamma", "gg_beta"))
    n = x.numel() // x.shape[1]
    sm = lambda t: t.sum((0, 2, 3))  # noqa: E731
    mu = sm(x) / n
    d = x - _c(mu)
    if mut == "stats_of_bf16_centred":
        d = bf16_round(d)
    m2 = sm(d * d)
    r = (m2 / n + bref.EPS).rsqrt()
    xh = (x - _c(mu)) * _c(r)
    y = _c(gam) * xh + _c(bet)
    z = torch.where(y > 0, y, bref.SLOPE * y)
    s = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, bref.SLOPE))
    if mut == "s_from_rounded_z":
        s = torch.where(y != 0, bf16_round(z) / torch.where(y != 0, y, torch.ones_like(y)), s)
    xs = xh
    if mut == "sums_of_bf16_y":
        live = _c(gam) != 0
        xs = torch.where(live, (bf16_round(y) - _c(bet)) / torch.where(live, _c(gam), torch.ones_like(_c(gam))), xh)
    gy = s * gz
    sgy, sgyx = sm(gy), sm(gy * xs)
    A, B = sgy / n, sgyx / n
    C, D, E = sm(ggx) / n, sm(ggx * xs) / n, sm(ggx * gy) / n
    gx = _c(gam * r) * (gy - _c(A) - xh * _c(B))
    g_gz = s * (_c(gam * r) * (ggx - _c(C) - xh * _c(D)) + _c(ggg) * xh + _c(ggb))
    B2, D2 = (D, B) if mut == "g_x_D_B_swapped" else (B, D)
    g_x = (-_c(gam * r * r) * (xh * _c(E - A * C - 3 * B * D) + _c(B2) * (ggx - _c(C)) + _c(D2) * (gy - _c(A)))
           + _c(ggg * r) * (gy - _c(A) - xh * _c(B)))
    mom = bref.MOMENTUM
    return dict(z=z, mean=mu, rstd=r, gx=gx, dgamma=sgyx, dbeta=sgy, g_gz=g_gz, g_x=g_x, g_gamma=n * r * (E - A * C - B * D),
                run_mean=(1 - mom) * inp["run_mean"].to(F64) + mom * mu,
                run_var=(1 - mom) * inp["run_var"].to(F64) + mom * m2 / (n - 1))


def _planted(inp, mut):
    """What a kernel with one defect would write."""
    if mut in ("head_short", "tail_twice", "tail_dropped"):
        return bref.emulate(inp, walk=mut)
    f32 ={k: v.to(F32) for k, v in _spec(inp, mut if mut != "z_truncated" else None).items()}
    if mut == "z_truncated":
        return dict(_rounded(f32), z=_truncate(f32["z"]))
    if mut == "gx_truncated":
        return dict(_rounded(f32), gx=_truncate(f32["gx"]))
    return _rounded(f32)


@pytest.mark.parametrize("mut,family,shape", [
    ("z_truncated", "diffuse", RAGGED),
    ("gx_truncated", "diffuse", RAGGED),
    ("head_short", "diffuse", EDGES),
    ("head_short", "diffuse", ODD_PIECES),
    ("tail_twice", "diffuse", EDGES),
    ("tail_twice", "mean_heavy", ODD_PIECES),
    ("tail_dropped", "diffuse", RAGGED),
    ("s_from_rounded_z", "diffuse", RAGGED),
    ("stats_of_bf16_centred", "diffuse", RAGGED),
    ("sums_of_bf16_y", "diffuse", RAGGED),
    ("g_x_D_B_swapped", "diffuse", RAGGED),
    ("g_x_D_B_swapped", "mean_heavy", PIECES),
])
def test_planted_defects_fall_outside(mut, family, shape):
    """Each defect puts at least one element outside; the fp64 spec and the emulation, rounded once, are inside."""
    inp, R = _case(family, shape)
    assert not bref.outside(_planted(inp, None), R)
    assert not bref.outside(bref.emulate(inp), R)
    N, C, H, W = shape
    g = bref.make_geo(N, C, H * W)
    walks = [w for c in range(C) for s in range(g["S"]) for w in bref.plane_walk(g, c, s)]
    if mut == "head_short":
        assert any(h for _, h, _, _ in walks)
    if mut in ("tail_twice", "tail_dropped"):
        assert any(t for _, _, _, t in walks)
    hit = bref.outside(_planted(inp, mut), R)
    print(mut, family, shape, hit)
    assert hit, f"{mut}: inside every bound"


# ---------------------------------------------------------------------------------------------- refusals of the C ABI
def test_abi_refusals():
    from amk import lib

    L = lib.load()
    null, p, off = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4104)   # off: 8-byte aligned only
    err = lambda: L.amk_last_error().decode()  # noqa: E731

    def fwd(x=p, N=2, C=4, HW=9, z=p, ws=p):
        return L.amk_bnact_bf16_fwd(x, p, p, N, C, HW, 1e-5, 0.1, 0.2, z, p, p, null, null, ws, null)

    def bwd(gz=p, x=p, N=2, C=4, HW=9, gx=p, sums=p):
        return L.amk_bnact_bf16_bwd(gz, x, p, p, p, p, N, C, HW, 0.2, gx, sums, null, null, p, null)

    def bwd_bwd(ggx=p, gz=p, x=p, N=2, C=4, HW=9, g_gz=p, g_x=p, sums=p):
        return L.amk_bnact_bf16_bwd_bwd(ggx, null, null, gz, x, p, p, p, p, sums, N, C, HW, 0.2, g_gz, g_x, null, p, null)

    for call, name in ((fwd, "amk_bnact_bf16_fwd"), (bwd, "amk_bnact_bf16_bwd"), (bwd_bwd, "amk_bnact_bf16_bwd_bwd")):
        for kw in (dict(N=0), dict(C=0), dict(HW=0), dict(N=-1)):
            assert call(**kw) == -1 and name in err() and "non-positive" in err(), kw
        assert call(C=65536) == -2 and "not supported" in err()
        assert call(N=1 << 16, HW=1 << 16) == -2 and "not supported" in err()
        assert call(x=null) == -1 and "null" in err()
        assert call(x=off) == -1 and "16-byte" in err()
    assert fwd(N=1, HW=1) == -1 and "more than one value" in err()
    assert fwd(ws=null) == -1 and fwd(z=null) == -1 and "null" in err()
    assert fwd(z=off) == -1 and "16-byte" in err()
    assert bwd(gz=null) == -1 and bwd(sums=null) == -1 and "null" in err()
    assert bwd(gz=off) == -1 and bwd(gx=off) == -1 and "16-byte" in err()
    assert bwd_bwd(ggx=null) == -1 and bwd_bwd(sums=null) == -1 and "null" in err()
    for kw in (dict(ggx=off), dict(gz=off), dict(g_gz=off), dict(g_x=off)):
        assert bwd_bwd(**kw) == -1 and "16-byte" in err(), kw
    with pytest.raises(RuntimeError, match="amk_bnact_bf16_fwd"):
        lib.check(fwd(N=0), "amk_bnact_bf16_fwd")
