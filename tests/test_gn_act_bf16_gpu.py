"""csrc/gn_act.hip on bf16 tensors (amk_gnact_bf16_fwd / _bwd) on the MI355X against the fp64 reference and the per-element
conditions of tests/gn_act_bf16_ref.py: mean, rstd, dgamma and dbeta within their f32 bounds and every element of z and gx
inside RNE's image of its bound, through the C ABI called the way ops._GNActBF16 calls it, for both activations on every case
and family; batch invariance and run-to-run reproducibility, bitwise; ops.group_norm_act under bf16 autocast (bf16 in, bf16
out, the bits of the direct call); the module path under autocast on the same input, whose f32 result rounds to bf16 inside
the same intervals (the two paths round in the same place); and the dispatch.

AMK_GN_ACT_BF16_BOUND_REPORT=<file>: write the worst ratio per tensor over this module to that JSON file."""
import json
import os

import pytest
import torch
import torch.nn as nn

import gn_act_bf16_ref as bref
import gn_act_ref as ref

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
_IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731
_CACHE = {}
OP_CASES = [ref.CASES[2], ref.CASES[3], bref.NEW_CASE]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AMK_GN_ACT_BF16_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(bref.WORST, f, indent=1, sort_keys=True)


def _inputs(family, case):
    key = (family, case)
    if key not in _CACHE:
        _CACHE[key] = bref.make_inputs(family, case)
    return _CACHE[key]


def _reference(family, case, act):
    """The last few references kept, never modified."""
    key = ("ref", family, case, act)
    if key not in _CACHE:
        for k in [k for k in _CACHE if k[0] == "ref"][:-3]:
            del _CACHE[k]
        _CACHE[key] = bref.reference(_inputs(family, case), case[4], act)
    return _CACHE[key]


def _abi(inp, G, act, device):
    """amk_gnact_bf16_fwd and _bwd as ops._GNActBF16 calls them: bf16 x and gz, the backward reads the forward's mean and rstd;
    a fresh workspace per call.  z and gx come back as bf16 CPU tensors."""
    from amk import lib, ops

    L, P = lib.load(), ops._ptr
    x, gz = (inp[k].to(device=device, dtype=BF16).contiguous() for k in ("x", "gz"))
    gamma, beta = (inp[k].to(device).contiguous() for k in ("gamma", "beta"))
    N, C, H, W = x.shape
    HW = H * W
    ws = lambda: torch.empty(int(L.amk_gnact_bf16_ws_floats(N, C, HW, G)), device=device, dtype=F32)  # noqa: E731
    z, gx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(N, G, device=device, dtype=F32), torch.empty(N, G, device=device, dtype=F32)
    dgamma, dbeta = torch.empty(C, device=device, dtype=F32), torch.empty(C, device=device, dtype=F32)
    lib.check(L.amk_gnact_bf16_fwd(P(x), P(gamma), P(beta), N, C, HW, G, ref.EPS, act, P(z), P(mean), P(rstd), P(ws()),
                                   ops._stream()), "amk_gnact_bf16_fwd")
    lib.check(L.amk_gnact_bf16_bwd(P(gz), P(x), P(gamma), P(beta), P(mean), P(rstd), N, C, HW, G, act, P(gx), P(dgamma),
                                   P(dbeta), P(ws()), ops._stream()), "amk_gnact_bf16_bwd")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(z=z, mean=mean, rstd=rstd, gx=gx, dgamma=dgamma, dbeta=dbeta).items()}


def _assert_inside(got, R, what, names=bref.TENSORS, record=True):
    q = bref.ratios(got, R, names=names, record=record)
    print(what, {k: round(v, 4) for k, v in q.items()})
    for name in names:
        v = got[name].detach().to(F64).cpu().reshape(R[name].shape)
        assert bool(torch.isfinite(v).all()), f"{what}: {name} is not finite"
        if name in bref.ROUNDED:
            bad = ~bref.inside(v, R, name)
            assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements of {name} outside RNE's image of their bound, "
                                         f"worst ratio {q[name]:.3f}")
        else:
            assert q[name] <= 1.0, f"{what}: {name} at {q[name]:.3f} of its bound"


@pytest.mark.parametrize("act", [0, 1], ids=["identity", "swish"])
@pytest.mark.parametrize("family,case", bref.family_cases(), ids=_IDS)
def test_kernels_within_bounds(device, family, case, act):
    inp = _inputs(family, case)
    got = _abi(inp, case[4], act, device)
    assert got["z"].dtype == BF16 and got["gx"].dtype == BF16 and got["mean"].dtype == F32
    _assert_inside(got, _reference(family, case, act), f"{family} {case} act {act}")
    if family == "gamma0":      # exact: y == beta to the bit where gamma == 0, and nothing flows back into x from there
        dead = inp["gamma"] == 0
        zd = got["z"][:, dead]
        if act == 0:
            assert torch.equal(zd, inp["beta"][dead].to(BF16).view(1, -1, 1, 1).expand_as(zd))
        else:
            assert torch.equal(zd, zd[:1, :, :1, :1].expand_as(zd))
        if case[1] == case[4]:
            assert not bool(got["gx"][:, dead].any())


@pytest.mark.parametrize("case", [ref.CASES[4], bref.NEW_CASE], ids=_IDS)
def test_a_sample_alone_equals_the_sample_in_its_batch_and_runs_repeat(device, case):
    """Bitwise.  z, mean, rstd and gx of a sample do not depend on the rest of the batch: the sample is run alone and as the
    last of a batch of two (C HW is a multiple of 8 in CASES[4]; in the new case C HW = 64 * 4489 is too, so the sample starts
    at the same alignment in both).  And two runs of the same call give the same bits in every tensor."""
    inp = _inputs("diffuse", case)
    if case[0] == 1:                                       # the new case has one sample: put another in front of it
        other = _inputs("offset", case)
        inp = dict(inp, x=torch.cat([other["x"], inp["x"]]), gz=torch.cat([other["gz"], inp["gz"]]))
    full = _abi(inp, case[4], 1, device)
    again = _abi(inp, case[4], 1, device)
    for name in bref.TENSORS:
        assert torch.equal(full[name], again[name]), name
    n = inp["x"].shape[0] - 1
    one = dict(inp, x=inp["x"][n:n + 1].clone(), gz=inp["gz"][n:n + 1].clone())
    got = _abi(one, case[4], 1, device)
    for name in ("z", "mean", "rstd", "gx"):
        assert torch.equal(got[name][0], full[name][n]), name


# ---------------------------------------------------------------------------------------------- the op
def _gn(inp, G, device=None):
    gn = nn.GroupNorm(G, inp["gamma"].numel(), eps=1e-6)
    with torch.no_grad():
        gn.weight.copy_(inp["gamma"])
        gn.bias.copy_(inp["beta"])
    return gn.to(device=device)


@pytest.mark.parametrize("act", [0, 1], ids=["identity", "swish"])
@pytest.mark.parametrize("case", OP_CASES, ids=_IDS)
def test_op_under_autocast(device, monkeypatch, case, act):
    """bf16 in, bf16 out on _GNActBF16, the bits of the direct ABI call, inside the intervals against the fp64 spec; and the
    module path under autocast on the same bf16 input returns f32 whose rounding to bf16 lies inside the same intervals."""
    from amk import ops

    monkeypatch.setattr(ops, "GN_ACT", True)
    monkeypatch.setattr(ops, "GN_ACT_BF16", True)
    inp, G = _inputs("diffuse", case), case[4]
    R = _reference("diffuse", case, act)
    gn = _gn(inp, G, device)
    x = inp["x"].to(device=device, dtype=BF16).requires_grad_()
    gz = inp["gz"].to(device=device, dtype=BF16)
    with torch.autocast("cuda", dtype=BF16):
        assert ops.group_norm_act_bf16_ok(gn, x) and not ops.group_norm_act_ok(gn, x)
        z = ops.group_norm_act(x, gn, act)
    assert z.dtype == BF16 and type(z.grad_fn).__name__ == "_GNActBF16Backward"
    gx, gw, gb = torch.autograd.grad(z, (x, gn.weight, gn.bias), gz)
    assert gx.dtype == BF16 and gw.dtype == F32 and gb.dtype == F32
    got = dict(z=z.detach(), gx=gx, dgamma=gw, dbeta=gb)
    direct = _abi(inp, G, act, device)
    for name in got:
        assert torch.equal(got[name].cpu(), direct[name]), name
    _assert_inside(got, R, f"op {case} act {act}", names=tuple(got), record=False)

    monkeypatch.setattr(ops, "GN_ACT_BF16", False)
    with torch.autocast("cuda", dtype=BF16):
        zm = ops.group_norm_act(x, gn, act)
    assert zm.dtype == F32 and type(zm.grad_fn).__name__ != "_GNActBF16Backward"
    _assert_inside(dict(z=zm.detach().to(BF16)), R, f"modules {case} act {act}", names=("z",), record=False)


def test_dispatch(device, monkeypatch):
    """With a bf16 x under bf16 autocast the fused bf16 kernels run and are timed under their names; nothing is saved under
    no_grad.  The bf16 switch off, AMK_GN_ACT off, a non-contiguous x, autocast to f16 and autocast disabled each keep the
    modules; an f32 x under autocast does as before."""
    from amk import ops

    case = ref.CASES[3]
    inp, G = _inputs("diffuse", case), case[4]
    gn = _gn(inp, G, device)
    x = inp["x"].to(device=device, dtype=BF16).requires_grad_()
    gz = inp["gz"].to(device=device, dtype=BF16)
    monkeypatch.setattr(ops, "GN_ACT", True)
    monkeypatch.setattr(ops, "GN_ACT_BF16", True)

    monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
    with torch.autocast("cuda", dtype=BF16):
        z = ops.group_norm_act(x, gn, 1)
    z.backward(gz)
    torch.cuda.synchronize()
    assert set(ops.KERNEL_EVENTS) == {"gnact_bf16_fwd", "gnact_bf16_bwd"}
    monkeypatch.setattr(ops, "KERNEL_EVENTS", None)
    assert x.grad.dtype == BF16 and gn.weight.grad.dtype == F32
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        z0 = ops.group_norm_act(x, gn, 1)
    assert z0.grad_fn is None and z0.dtype == BF16 and torch.equal(z0, z.detach())

    def modules_path(xin, dtype=BF16, enabled=True):
        with torch.autocast("cuda", dtype=dtype, enabled=enabled):
            assert not ops.group_norm_act_bf16_ok(gn, xin)
            out = ops.group_norm_act(xin, gn, 1)
        assert "GNAct" not in type(out.grad_fn).__name__
        return out

    zf = z.detach().float()
    close = lambda a, what: torch.testing.assert_close(a.float(), zf, rtol=2 ** -7, atol=2 ** -7, msg=what)  # noqa: E731
    xt = x.detach().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_()
    assert not xt.is_contiguous()
    close(modules_path(xt), "non-contiguous")
    close(modules_path(x, dtype=torch.float16), "autocast to f16")
    gnb = _gn(inp, G, device).to(BF16)                     # autocast disabled: a bf16 module on the bf16 x
    with torch.autocast("cuda", enabled=False):
        assert not ops.group_norm_act_bf16_ok(gn, x)
        out = ops.group_norm_act(x, gnb, 1)
    assert "GNAct" not in type(out.grad_fn).__name__
    x32 = x.detach().float().requires_grad_()              # an f32 x under autocast keeps the modules and an f32 result
    assert modules_path(x32).dtype == F32
    monkeypatch.setattr(ops, "GN_ACT_BF16", False)
    close(modules_path(x), "bf16 switch off")
    monkeypatch.setattr(ops, "GN_ACT_BF16", True)
    monkeypatch.setattr(ops, "GN_ACT", False)
    close(modules_path(x), "AMK_GN_ACT off")


def test_zz_report_worst_ratios(capsys):
    with capsys.disabled():
        print("\ngn_act_bf16 worst ratios:", {k: round(v, 4) for k, v in sorted(bref.WORST.items())})
    assert bref.WORST and all(v <= 1.0 for v in bref.WORST.values())
