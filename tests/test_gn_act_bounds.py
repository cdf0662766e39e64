"""tests/gn_act_ref.py without a GPU: the CPU emulation of csrc/gn_act.hip (f32, the kernels' summation order) stays under
HALF of every per-element bound on every family and case; defects planted in the fp64 spec land outside the bounds, so the
bounds are not vacuous; and the C ABI's refusals, which need no device memory."""
import ctypes
from unittest import mock

import pytest
import torch

import gn_act_ref as ref
import gn_act_spec as spec

F64 = torch.float64
_CACHE = {}


def _case(family, case, act):
    """(inputs, reference): the last few kept, never modified."""
    key = (family, case, act)
    if key not in _CACHE:
        if len(_CACHE) >= 4:
            _CACHE.pop(next(iter(_CACHE)))
        inp = ref.make_inputs(family, case)
        _CACHE[key] = (inp, ref.reference(inp, case[4], act))
    return _CACHE[key]


@pytest.mark.parametrize("act", [0, 1], ids=["identity", "swish"])
@pytest.mark.parametrize("family,case", ref.family_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_emulation_stays_under_half_of_every_bound(family, case, act):
    inp, R = _case(family, case, act)
    q = ref.ratios(ref.emulate(inp, case[4], act), R, record=False)
    print(family, case, act, {k: round(v, 4) for k, v in q.items()})
    for name, v in q.items():
        assert v <= 0.5, f"{family} {case} act {act}: the emulation's {name} at {v:.3f} of its bound"
    for name in ref.TENSORS:
        assert bool(torch.isfinite(R["bound_" + name]).all()), f"{name} has no bound somewhere"


def test_saturated_family_reaches_both_ends():
    """|y| reaches 150 on both sides in `saturated`, and the reference and the emulation stay finite there."""
    case = ref.ALL_FAMILY_CASES[1]
    inp, R = _case("saturated", case, 1)
    x, G = inp["x"].to(F64), case[4]
    y = spec.fwd(x, inp["gamma"].to(F64), inp["beta"].to(F64), G, ref.EPS, 0)[0]
    assert float(y.max()) > 150 and float(y.min()) < -150
    got = ref.emulate(inp, G, 1)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


def test_sigmoid_form_at_both_ends():
    """1 / (1 + exp2(-y log2 e)) and sigma (1 + y (1 - sigma)) in f32 at y = -200, 200 and in between: finite, 0 and 1 at the
    ends, within 1e-6 of fp64 elsewhere."""
    y = torch.tensor([-200.0, -104.0, -88.0, -20.0, -1.278, 0.0, 1.0, 20.0, 88.0, 104.0, 200.0])
    sg = ref._sigmoid(y)
    a1 = sg * (1.0 + y * (1.0 - sg))
    z = y * sg
    assert bool(torch.isfinite(sg).all() and torch.isfinite(a1).all() and torch.isfinite(z).all())
    assert float(sg[0]) == 0.0 and float(z[0]) == 0.0 and float(a1[0]) == 0.0
    assert float(sg[-1]) == 1.0 and float(z[-1]) == 200.0 and float(a1[-1]) == 1.0
    y64 = y.to(F64)
    assert float((sg.to(F64) - torch.sigmoid(y64)).abs().max()) < 1e-6
    assert float((a1.to(F64) - spec.act_grad(y64, 1)).abs().max()) < 1e-4      # 3 w |y| at y = 200: 3.6e-5


# ---------------------------------------------------------------------------------------------- the bounds are not vacuous
def _mutated(inp, G, act, mut):
    """The fp64 spec with one defect planted."""
    x, gam, bet, gz = (inp[k].to(F64) for k in ("x", "gamma", "beta", "gz"))
    N, C = x.shape[:2]
    xr = x.reshape(N, G, -1)
    m = xr.shape[2]
    st = xr[..., :-1] if mut == "element_dropped" else xr
    mu = st.mean(2)
    var = ((st - mu.unsqueeze(2)) ** 2).mean(2)
    if mut == "unbiased_variance":
        var = var * m / (m - 1)
    r = (var + (1e-5 if mut == "eps_1e-5" else ref.EPS)).rsqrt()
    y = spec._c(gam) * ((x - spec._per_elem(mu, x, G)) * spec._per_elem(r, x, G)) + spec._c(bet)
    z = spec.act_fwd(y, act)
    if mut == "swish_grad_without_y_term":
        with mock.patch.object(spec, "act_grad", lambda y, act: torch.sigmoid(y) if act == 1 else torch.ones_like(y)):
            gx, dgamma, dbeta = spec.bwd(gz, x, gam, bet, mu, r, G, act)
    else:
        gx, dgamma, dbeta = spec.bwd(gz, x, gam, bet, mu, r, G, act)
    return dict(z=z, mean=mu, rstd=r, gx=gx, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize("mut", ["unbiased_variance", "eps_1e-5", "swish_grad_without_y_term", "element_dropped"])
def test_planted_defects_fall_outside_the_bounds(mut):
    hit = []
    for family, case in ref.family_cases():
        if case[0] * case[1] * case[2] * case[3] > 1 << 20:
            continue                                  # the largest case adds nothing here
        inp, R = _case(family, case, 1)
        q = ref.ratios(_mutated(inp, case[4], 1, mut), R, record=False)
        # the unmutated spec is the reference itself
        assert max(ref.ratios(_mutated(inp, case[4], 1, None), R, record=False).values()) < 1e-6
        hit += [(family, case, n, v) for n, v in q.items() if v > 1.0]
    assert hit, f"{mut}: inside every bound on every case"
    print(mut, [(f, c, n, round(v, 1)) for f, c, n, v in hit[:6]])


# ---------------------------------------------------------------------------------------------- refusals of the C ABI
def test_abi_refusals():
    from amk import lib

    L = lib.load()
    null, p, off = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    err = lambda: L.amk_last_error().decode()  # noqa: E731

    def fwd(x=p, N=2, C=64, HW=9, G=32, act=1, z=p, ws=p):
        return L.amk_gnact_fwd(x, p, p, N, C, HW, G, 1e-6, act, z, p, p, ws, null)

    def bwd(gz=p, N=2, C=64, HW=9, G=32, act=1, gx=p, dgamma=p):
        return L.amk_gnact_bwd(gz, p, p, p, p, p, N, C, HW, G, act, gx, dgamma, p, p, null)

    for call, name in ((fwd, "amk_gnact_fwd"), (bwd, "amk_gnact_bwd")):
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
    assert bwd(gx=off) == -1 and "16-byte" in err()
    assert L.amk_gnact_ws_floats(0, 64, 9, 32) == 0 and L.amk_gnact_ws_floats(2, 48, 9, 32) == 0
    for N, C, H, W, G in ref.CASES:
        assert L.amk_gnact_ws_floats(N, C, H * W, G) == ref.ws_floats(N, C, H * W, G)
    with pytest.raises(RuntimeError, match="amk_gnact_fwd"):
        lib.check(fwd(act=2), "amk_gnact_fwd")
