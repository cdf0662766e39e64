"""tests/gn_act_bf16_ref.py without a GPU: the CPU emulation of the bf16 GroupNorm + Swish kernels (f32 torch ops in the
kernels' order on the bf16 walk, z and gx rounded to bf16 once) keeps its f32 values under HALF of every f32 bound and its
rounded z and gx inside RNE's image of the bound; defects planted in the fp64 spec or in the rounding land outside; and the
refusals of amk_gnact_bf16_*, which need no device memory."""
import ctypes

import pytest
import torch

import gn_act_bf16_ref as bref
import gn_act_ref as ref
import gn_act_spec as spec
from bf16_dense_ref import bf16_round
from test_gn_act_bounds import _mutated

F32, F64 = torch.float32, torch.float64
_IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731
_CACHE = {}
EMU_WORST = {}


def _case(family, case, act):
    """(inputs, reference): the last few kept, never modified."""
    key = (family, case, act)
    if key not in _CACHE:
        if len(_CACHE) >= 4:
            _CACHE.pop(next(iter(_CACHE)))
        inp = bref.make_inputs(family, case)
        _CACHE[key] = (inp, bref.reference(inp, case[4], act))
    return _CACHE[key]


def test_bf16_grid_functions():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.00390625, -1.0 - 2.0 ** -8, 0.0, 3.1415926, -2.5e-7,
                      float("inf")], dtype=F64)
    rne = bref.bf16_rne(v)
    assert torch.equal(rne[:-1], v[:-1].to(torch.bfloat16).to(F64)) and rne[-1] == float("inf")
    assert rne[1] == 1.0 and rne[2] == 1.0 + 2.0 ** -6                 # ties go to the even neighbour
    dn, up = bref.bf16_down(v), bref.bf16_up(v)
    assert bool((dn <= v).all() and (v <= up).all() and (dn <= rne).all() and (rne <= up).all())
    assert torch.equal(dn[:-1], bf16_round(dn[:-1])) and torch.equal(up[:-1], bf16_round(up[:-1]))
    assert float(dn[1]) == 1.0 and float(up[1]) == 1.0 + 2.0 ** -7 and float(dn[0]) == float(up[0]) == 1.0


def test_geometry_of_the_new_case():
    """HW = 4489: two pieces of 2248 and 2241, every residue of the plane base mod 8, heads and tails of 1 to 7."""
    N, C, H, W, G = bref.NEW_CASE
    HW = H * W
    g = bref.make_geo(C, HW, G)
    assert (g["Q"], g["L"], g["S"]) == (2, 2248, 4) and g["L"] % 8 == 0
    heads, tails = set(), set()
    for pl in range(N * C):
        for q in range(g["Q"]):
            e0 = q * g["L"]
            ln = min(HW, e0 + g["L"]) - e0
            head = min((8 - (pl * HW + e0) % 8) % 8, ln)
            heads.add(head)
            tails.add((ln - head) % 8)
    assert heads == set(range(8)) and tails >= set(range(1, 8))
    # every element is visited exactly once by the walk
    seg, plane = bref._plans(N, C, HW, G)
    for plan in (seg, plane):
        idx = plan[plan < N * C * HW]
        assert idx.numel() == N * C * HW and idx.unique().numel() == N * C * HW


@pytest.mark.parametrize("act", [0, 1], ids=["identity", "swish"])
@pytest.mark.parametrize("family,case", bref.family_cases(), ids=_IDS)
def test_emulation_stays_under_half_of_every_bound(family, case, act):
    inp, R = _case(family, case, act)
    assert torch.equal(inp["x"], bf16_round(inp["x"])) and torch.equal(inp["gz"], bf16_round(inp["gz"]))
    f32 = bref.emulate_f32(inp, case[4], act)
    q32 = ref.ratios(f32, R, record=False)                       # every tensor before the store, against b32
    got = dict(f32, **{name: bf16_round(f32[name]) for name in bref.ROUNDED})
    q = bref.ratios(got, R, record=False)
    print(family, case, act, {k: round(v, 4) for k, v in q32.items()}, {k: round(q[k], 4) for k in bref.ROUNDED})
    for name, v in q32.items():
        assert v <= 0.5, f"{family} {case} act {act}: the emulation's f32 {name} at {v:.3f} of its bound"
    for name in bref.ROUNDED:
        assert q[name] <= 1.0, f"{family} {case} act {act}: the emulation's bf16 {name} outside RNE's image of its bound"
        assert bool((R["lo_" + name] <= R["hi_" + name]).all())
    for name in bref.TENSORS:
        assert bool(torch.isfinite(R["bound_" + name]).all()), f"{name} has no bound somewhere"
        EMU_WORST[name] = max(EMU_WORST.get(name, 0.0), q[name])


def test_zz_report_emulation_worst(capsys):
    with capsys.disabled():
        print("\ngn_act_bf16 emulation worst ratios:", {k: round(v, 4) for k, v in sorted(EMU_WORST.items())})
    assert all(v <= 1.0 for v in EMU_WORST.values())


# ---------------------------------------------------------------------------------------------- the bounds are not vacuous
def _truncate(v):
    """f32 -> bf16 by dropping the low 16 bits."""
    return (v.to(F32).contiguous().view(torch.int32) & -65536).view(F32)


def _planted(inp, G, act, mut):
    """What a kernel with one defect would write, from the fp64 spec: z and gx rounded to bf16 once unless the defect says
    otherwise."""
    x, gam, bet, gz = (inp[k].to(F64) for k in ("x", "gamma", "beta", "gz"))
    if mut in ("z_truncated", "z_rounded_twice", "stats_of_bf16_centred"):
        xr = x.reshape(x.shape[0], G, -1)
        mu = xr.mean(2)
        d = xr - mu.unsqueeze(2)
        if mut == "stats_of_bf16_centred":
            d = bf16_round(d)
        r = ((d ** 2).mean(2) + ref.EPS).rsqrt()
        y = spec._c(gam) * ((x - spec._per_elem(mu, x, G)) * spec._per_elem(r, x, G)) + spec._c(bet)
        if mut == "z_rounded_twice":
            y = bf16_round(y)
        z = spec.act_fwd(y, act)
        gx, dgamma, dbeta = spec.bwd(gz, x, gam, bet, mu, r, G, act)
        out = dict(z=z, mean=mu, rstd=r, gx=gx, dgamma=dgamma, dbeta=dbeta)
        if mut == "z_truncated":
            return dict(out, z=_truncate(z).to(F64), gx=bf16_round(gx))
    else:
        out = _mutated(inp, G, act, mut)
    return dict(out, z=bf16_round(out["z"]), gx=bf16_round(out["gx"]))


def _outside(got, R):
    """[(tensor, ratio)] of the tensors with at least one element outside its condition."""
    q = bref.ratios(got, R, record=False)
    bad = {n for n in bref.ROUNDED if not bool(bref.inside(got[n].to(F64), R, n).all())}
    return [(n, round(v, 2)) for n, v in q.items() if v > 1.0 or n in bad]


@pytest.mark.parametrize("mut", ["z_truncated", "z_rounded_twice", "stats_of_bf16_centred", "unbiased_variance",
                                 "swish_grad_without_y_term", "element_dropped"])
def test_planted_defects_fall_outside(mut):
    """On `diffuse` at CASES[3], each defect puts at least one element outside; the spec rounded once is inside."""
    case = ref.CASES[3]
    inp, R = _case("diffuse", case, 1)
    assert not _outside(_planted(inp, case[4], 1, None), R)
    hit = _outside(_planted(inp, case[4], 1, mut), R)
    print(mut, hit)
    assert hit, f"{mut}: inside every bound"


def test_planted_eps_falls_outside():
    """eps = 1e-5 for 1e-6 moves rstd by 4.5e-6 / var in relative terms: on `diffuse` at CASES[3] (var = 1) that is 0.36 of
    the f32 bound of rstd, which the bf16 kernels share with the f32 ones, and RNE(z) moves nowhere; as in
    tests/test_gn_act_bounds.py the defect is found over the families and cases instead (on the runs of 9 and of 2 values, whose
    variance is far below 1, and on `constant`, var = 0, where rstd changes by a factor 10^1/2)."""
    hit = []
    for family, case in bref.family_cases():
        if case[0] * case[1] * case[2] * case[3] > 1 << 20:
            continue
        inp, R = _case(family, case, 1)
        hit += [(family, case, n, v) for n, v in _outside(_planted(inp, case[4], 1, "eps_1e-5"), R)]
    print(hit[:6])
    assert hit, "eps_1e-5: inside every bound on every case"


# ---------------------------------------------------------------------------------------------- refusals of the C ABI
def test_abi_refusals():
    from amk import lib

    L = lib.load()
    null, p, off = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4104)   # off: 8-byte aligned only
    err = lambda: L.amk_last_error().decode()  # noqa: E731

    def fwd(x=p, N=2, C=64, HW=9, G=32, act=1, z=p, ws=p):
        return L.amk_gnact_bf16_fwd(x, p, p, N, C, HW, G, 1e-6, act, z, p, p, ws, null)

    def bwd(gz=p, x=p, N=2, C=64, HW=9, G=32, act=1, gx=p, dgamma=p):
        return L.amk_gnact_bf16_bwd(gz, x, p, p, p, p, N, C, HW, G, act, gx, dgamma, p, p, null)

    for call, name in ((fwd, "amk_gnact_bf16_fwd"), (bwd, "amk_gnact_bf16_bwd")):
        for kw in (dict(N=0), dict(C=0), dict(HW=0), dict(G=0), dict(N=-1), dict(act=2), dict(act=-1)):
            assert call(**kw) == -1 and name in err(), kw
        assert call(act=2) == -1 and "act" in err()
        assert call(N=0) == -1 and "non-positive" in err()
        assert call(C=48, G=32) == -2 and "does not divide" in err()
        assert call(N=1 << 20, C=4096, HW=1, G=4096) == -2 and "2^31" in err()
    assert fwd(x=null) == -1 and "null" in err()
    assert fwd(ws=null) == -1 and "null" in err()
    assert bwd(gz=null) == -1 and "null" in err()
    assert bwd(dgamma=null) == -1 and "null" in err()
    assert fwd(x=off) == -1 and "16-byte" in err()
    assert fwd(z=off) == -1 and "16-byte" in err()
    assert bwd(gz=off) == -1 and "16-byte" in err()
    assert bwd(x=off) == -1 and "16-byte" in err()
    assert bwd(gx=off) == -1 and "16-byte" in err()
    assert L.amk_gnact_bf16_ws_floats(0, 64, 9, 32) == 0 and L.amk_gnact_bf16_ws_floats(2, 48, 9, 32) == 0
    for N, C, H, W, G in bref.CASES:
        assert L.amk_gnact_bf16_ws_floats(N, C, H * W, G) == bref.ws_floats(N, C, H * W, G)
    with pytest.raises(RuntimeError, match="amk_gnact_bf16_fwd"):
        lib.check(fwd(act=2), "amk_gnact_bf16_fwd")
