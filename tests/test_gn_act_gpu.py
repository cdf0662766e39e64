"""csrc/gn_act.hip on the MI355X against the fp64 reference and per-element bounds of tests/gn_act_ref.py: every element of
z, mean, rstd, gx, dgamma and dbeta through the C ABI, called the way amk.ops calls it, for both activations on every case
and family; batch invariance and run-to-run reproducibility, bitwise; ops.group_norm_act against nn.GroupNorm + x sigmoid(x)
in fp64; and the dispatch (fused kernels with the switch on; the modules with it off, under autocast and for a
non-contiguous input).

AMK_GN_ACT_BOUND_REPORT=<file>: write the worst |got - ref| / bound per tensor over this module to that JSON file."""
import json
import os

import pytest
import torch
import torch.nn as nn

import gn_act_ref as ref
from util import assert_close

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
_IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AMK_GN_ACT_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(ref.WORST, f, indent=1, sort_keys=True)


def _inputs(family, case):
    key = (family, case)
    if key not in _CACHE:
        _CACHE[key] = ref.make_inputs(family, case)
    return _CACHE[key]


def _abi(inp, G, act, device):
    """amk_gnact_fwd and _bwd as ops._GNAct calls them: the backward reads the forward's mean and rstd; a fresh workspace
    per call."""
    from amk import lib, ops

    L, P = lib.load(), ops._ptr
    x, gz, gamma, beta = (inp[k].to(device).contiguous() for k in ("x", "gz", "gamma", "beta"))
    N, C, H, W = x.shape
    HW = H * W
    ws = lambda: torch.empty(int(L.amk_gnact_ws_floats(N, C, HW, G)), device=device, dtype=F32)  # noqa: E731
    z, gx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(N, G, device=device, dtype=F32), torch.empty(N, G, device=device, dtype=F32)
    dgamma, dbeta = torch.empty(C, device=device, dtype=F32), torch.empty(C, device=device, dtype=F32)
    lib.check(L.amk_gnact_fwd(P(x), P(gamma), P(beta), N, C, HW, G, ref.EPS, act, P(z), P(mean), P(rstd), P(ws()),
                              ops._stream()), "amk_gnact_fwd")
    lib.check(L.amk_gnact_bwd(P(gz), P(x), P(gamma), P(beta), P(mean), P(rstd), N, C, HW, G, act, P(gx), P(dgamma), P(dbeta),
                              P(ws()), ops._stream()), "amk_gnact_bwd")
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(z=z, mean=mean, rstd=rstd, gx=gx, dgamma=dgamma, dbeta=dbeta).items()}


@pytest.mark.parametrize("act", [0, 1], ids=["identity", "swish"])
@pytest.mark.parametrize("family,case", ref.family_cases(), ids=_IDS)
def test_kernels_within_bounds(device, family, case, act):
    inp = _inputs(family, case)
    R = ref.reference(inp, case[4], act)
    got = _abi(inp, case[4], act, device)
    q = ref.ratios(got, R)
    print(family, case, act, {k: round(v, 4) for k, v in q.items()})
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    for name, v in q.items():
        assert v <= 1.0, f"{family} {case} act {act}: {name} at {v:.3f} of its bound"
    if family == "gamma0":      # exact: y == beta to the bit where gamma == 0, and nothing flows back into x from there
        dead = inp["gamma"] == 0
        zd = got["z"][:, dead]
        if act == 0:
            assert torch.equal(zd, inp["beta"][dead].view(1, -1, 1, 1).expand_as(zd))
        else:                   # one value per channel, whatever x holds
            assert torch.equal(zd, zd[:1, :, :1, :1].expand_as(zd))
        if case[1] == case[4]:  # cpg == 1: the whole run has gamma == 0
            assert not bool(got["gx"][:, dead].any())


@pytest.mark.parametrize("case", [ref.CASES[2], ref.CASES[4]], ids=_IDS)
def test_a_sample_alone_equals_the_sample_in_its_batch(device, case):
    """Bitwise: z, mean, rstd and gx of sample n do not depend on the rest of the batch (C HW is a multiple of 4 in every
    case, so a sample starts at the same alignment alone and in the batch)."""
    inp = _inputs("diffuse", case)
    full = _abi(inp, case[4], 1, device)
    n = case[0] - 1
    one = dict(inp, x=inp["x"][n:n + 1].clone(), gz=inp["gz"][n:n + 1].clone())
    got = _abi(one, case[4], 1, device)
    for name in ("z", "mean", "rstd", "gx"):
        assert torch.equal(got[name][0], full[name][n]), name


@pytest.mark.parametrize("case", [ref.CASES[2], ref.CASES[5]], ids=_IDS)
def test_run_to_run_reproducible(device, case):
    inp = _inputs("diffuse", case)
    a, b = _abi(inp, case[4], 1, device), _abi(inp, case[4], 1, device)
    for name in ref.TENSORS:
        assert torch.equal(a[name], b[name]), name


# ---------------------------------------------------------------------------------------------- the op
def _gn(inp, G, device=None, dtype=F32):
    gn = nn.GroupNorm(G, inp["gamma"].numel(), eps=1e-6)
    with torch.no_grad():
        gn.weight.copy_(inp["gamma"])
        gn.bias.copy_(inp["beta"])
    return gn.to(device=device, dtype=dtype)


def _modules(inp, G, act, x, gz, gn):
    y = gn(x)
    z = y * torch.sigmoid(y) if act == 1 else y
    gx, gw, gb = torch.autograd.grad(z, (x, gn.weight, gn.bias), gz)
    return dict(z=z.detach(), gx=gx, dgamma=gw, dbeta=gb)


@pytest.mark.parametrize("act", [0, 1], ids=["identity", "swish"])
@pytest.mark.parametrize("case", [ref.CASES[2], ref.CASES[3], ref.CASES[5]], ids=_IDS)
def test_op_agrees_with_the_modules_in_fp64(device, monkeypatch, case, act):
    from amk import ops

    monkeypatch.setattr(ops, "GN_ACT", True)
    inp, G = _inputs("diffuse", case), case[4]
    want = _modules(inp, G, act, inp["x"].to(F64).requires_grad_(), inp["gz"].to(F64), _gn(inp, G, dtype=F64))
    gn = _gn(inp, G, device)
    x = inp["x"].to(device).requires_grad_()
    assert ops.group_norm_act_ok(gn, x)
    z = ops.group_norm_act(x, gn, act)
    assert type(z.grad_fn).__name__ == "_GNActBackward"
    gx, gw, gb = torch.autograd.grad(z, (x, gn.weight, gn.bias), inp["gz"].to(device))
    got = dict(z=z.detach(), gx=gx, dgamma=gw, dbeta=gb)
    for name in want:
        assert_close(got[name], want[name], 2e-5, f"{name} {case} act {act}")
    # the wrapper adds nothing to the kernels: the same bits as the C ABI called directly
    direct = _abi(inp, G, act, device)
    for name in got:
        assert torch.equal(got[name].cpu(), direct[name]), name


def test_dispatch(device, monkeypatch):
    """Switch on: the fused kernels run and are timed under their names; nothing is saved under no_grad.  Switch off, under
    autocast and for a non-contiguous input: the modules run, and the results agree with the fused ones."""
    from amk import ops

    case = ref.CASES[3]
    inp, G = _inputs("diffuse", case), case[4]
    gn = _gn(inp, G, device)
    x = inp["x"].to(device).requires_grad_()
    gz = inp["gz"].to(device)

    monkeypatch.setattr(ops, "GN_ACT", True)
    monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
    z = ops.group_norm_act(x, gn, 1)
    z.backward(gz)
    torch.cuda.synchronize()
    assert set(ops.KERNEL_EVENTS) == {"gnact_fwd", "gnact_bwd"}
    fused = dict(z=z.detach(), gx=x.grad.clone(), dgamma=gn.weight.grad.clone(), dbeta=gn.bias.grad.clone())
    with torch.no_grad():
        z0 = ops.group_norm_act(x, gn, 1)
    assert z0.grad_fn is None and torch.equal(z0, fused["z"])
    monkeypatch.setattr(ops, "KERNEL_EVENTS", None)

    def modules_path(xin):
        out = ops.group_norm_act(xin, gn, 1)
        assert type(out.grad_fn).__name__ != "_GNActBackward"
        return out

    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not ops.group_norm_act_ok(gn, x)
        za = modules_path(x)
    assert za.dtype == F32                                 # autocast runs group_norm in f32
    assert_close(za, fused["z"], 2e-5, "autocast z")
    xt = inp["x"].to(device).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not xt.is_contiguous() and not ops.group_norm_act_ok(gn, xt)
    assert_close(modules_path(xt), fused["z"], 2e-5, "non-contiguous z")
    monkeypatch.setattr(ops, "GN_ACT", False)
    assert not ops.group_norm_act_ok(gn, x)
    off = _modules(inp, G, 1, x.detach().requires_grad_(), gz, gn)
    zo = modules_path(x)
    assert torch.equal(zo, off["z"])
    for name in fused:
        assert_close(fused[name], off[name], 2e-5, f"switch off {name}")
    cpu_gn = _gn(inp, G)
    assert not ops.group_norm_act_ok(cpu_gn, inp["x"])
    assert ops.group_norm_act(inp["x"], cpu_gn, 0).shape == inp["x"].shape


def test_zz_report_worst_ratios(capsys):
    with capsys.disabled():
        print("\ngn_act worst |got - ref| / bound:", {k: round(v, 4) for k, v in sorted(ref.WORST.items())})
    assert ref.WORST and all(v <= 1.0 for v in ref.WORST.values())
