"""csrc/discr_norm.hip on the MI355X against the fp64 reference and per-element bounds of tests/discr_norm_ref.py: every
output of the three entry points through the C ABI, called the way amk.ops calls it, on every input family and every
segment geometry (ragged last segment, pieces of odd planes, more than 256 segments, HW == 1); the exact cases; the optional
pointers; and ops.bn_leaky_relu through torch.autograd.grad with and without input_grad_only().  Every element of every
tensor is held to its own bound: no global-maximum criterion, no comparison with another f32 implementation.

AMK_DISCR_NORM_BOUND_REPORT=<file>: write the worst |got - ref| / bound per tensor over this module, over all families and
per family, to that JSON file."""
import json
import os

import pytest
import torch
import torch.nn as nn

import discr_norm_ref as ref

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AMK_DISCR_NORM_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            by_family = {fam: {n: v for (f2, n), v in ref.WORST_BY_FAMILY.items() if f2 == fam} for fam in ref.FAMILIES}
            json.dump({"all": ref.WORST, "by_family": by_family}, f, indent=1, sort_keys=True)


KEPT = [(5, 4, 31, 31), (2, 3, 65, 65)]     # the shapes several tests share; a reference holds 25 arrays like x
_CACHE = {}


def _case(family, shape, gg=True):
    """(inputs on the CPU, reference), never modified; kept for the module only on the shapes that several tests share.
    gg=False: gg_gamma = gg_beta = 0."""
    key = (family, shape, gg)
    if key in _CACHE:
        return _CACHE[key]
    inp = ref.make_inputs(family, shape)
    if not gg:
        inp["gg_gamma"], inp["gg_beta"] = torch.zeros_like(inp["gamma"]), torch.zeros_like(inp["beta"])
    case = (inp, ref.reference(inp, family))
    if shape in KEPT:
        _CACHE[key] = case
    return case


def _abi(inp, device, param_grads=True, running=True, gg="given", g_gamma=True):
    """amk_bnact_fwd, _bwd and _bwd_bwd as ops._BNAct / _BNActGrad call them: the backward reads the forward's mean and
    rstd, the double backward the backward's sums; a fresh workspace per call.  Outputs not asked for are None."""
    from amk import lib, ops

    L, P = lib.load(), ops._ptr
    t = {k: v.to(device).contiguous() for k, v in inp.items()}
    x, gz, ggx, gamma, beta = t["x"], t["gz"], t["ggx"], t["gamma"], t["beta"]
    N, C, H, W = x.shape
    HW = H * W
    ws = lambda: torch.empty(int(L.amk_bnact_ws_floats(N, C, HW)), device=device, dtype=F32)  # noqa: E731
    vec = lambda: torch.empty(C, device=device, dtype=F32)  # noqa: E731
    z, mean, rstd = torch.empty_like(x), vec(), vec()
    rm, rv = (t["run_mean"].clone(), t["run_var"].clone()) if running else (None, None)
    lib.check(L.amk_bnact_fwd(P(x), P(gamma), P(beta), N, C, HW, ref.EPS, ref.MOMENTUM, ref.SLOPE, P(z), P(mean), P(rstd),
                              P(rm), P(rv), P(ws()), ops._stream()), "amk_bnact_fwd")
    gx, sums = torch.empty_like(x), torch.empty(2, C, device=device, dtype=F32)
    dgamma, dbeta = (vec(), vec()) if param_grads else (None, None)
    lib.check(L.amk_bnact_bwd(P(gz), P(x), P(gamma), P(beta), P(mean), P(rstd), N, C, HW, ref.SLOPE, P(gx), P(sums),
                              P(dgamma), P(dbeta), P(ws()), ops._stream()), "amk_bnact_bwd")
    ggg, ggb = {"given": (t["gg_gamma"], t["gg_beta"]), "null": (None, None),
                "zeros": (torch.zeros_like(gamma), torch.zeros_like(beta))}[gg]
    g_gz, g_x = torch.empty_like(x), torch.empty_like(x)
    g_g = vec() if g_gamma else None
    lib.check(L.amk_bnact_bwd_bwd(P(ggx), P(ggg), P(ggb), P(gz), P(x), P(gamma), P(beta), P(mean), P(rstd), P(sums), N, C, HW,
                                  ref.SLOPE, P(g_gz), P(g_x), P(g_g), P(ws()), ops._stream()), "amk_bnact_bwd_bwd")
    torch.cuda.synchronize()
    return dict(z=z, mean=mean, rstd=rstd, run_mean=rm, run_var=rv, gx=gx, sums=sums, dgamma=dgamma, dbeta=dbeta, g_gz=g_gz,
                g_x=g_x, g_gamma=g_g)


def _check(got, R, tag, family):
    names = [n for n in ref.TENSORS if got.get(n) is not None]
    q = ref.ratios({k: got[k].cpu() for k in names}, R, names=names, family=family)
    print(tag, {k: round(v, 4) for k, v in q.items()})
    for name, v in q.items():
        assert v <= 1.0, f"{tag}: {name} at {v:.3f} of its bound"
    return q


def _ch(t):
    return t.view(1, -1, 1, 1)


def _leaky(b):
    b = torch.as_tensor(b, dtype=F32)
    return torch.where(b > 0, b, torch.tensor(ref.SLOPE, dtype=F32) * b)


# ---------------------------------------------------------------------------------------------- bounds, through the C ABI
@pytest.mark.parametrize("shape", ref.CPU_SHAPES + ref.GPU_SHAPES)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_kernels_within_bounds(device, family, shape):
    inp, R = _case(family, shape)
    got = {k: v.cpu() for k, v in _abi(inp, device).items()}
    _check(got, R, f"{family} {shape}", family)
    assert len(got) == len(ref.TENSORS) + 1 and all(bool(torch.isfinite(v).all()) for v in got.values())
    assert torch.equal(got["sums"][0], got["dbeta"]) and torch.equal(got["sums"][1], got["dgamma"])
    C, HW = shape[1], shape[2] * shape[3]
    xh = (inp["x"] - _ch(got["mean"])) * _ch(got["rstd"])
    t = _ch(inp["gg_gamma"]) * xh + _ch(inp["gg_beta"])
    for c, b in ref.dead_channels(family, C, HW).items():
        assert torch.equal(got["z"][:, c], _leaky(b).expand_as(got["z"][:, c])), f"channel {c}: z is not leaky_relu(beta)"
        assert not bool(got["gx"][:, c].any()), f"channel {c}: gx is not zero"
        want = t[:, c] if b > 0 else torch.tensor(ref.SLOPE, dtype=F32) * t[:, c]
        assert torch.equal(got["g_gz"][:, c], want), f"channel {c}: g_gz is not s (gg_gamma xh + gg_beta)"
    for c, v in ref.flat_channels(family, C).items():
        assert float(got["mean"][c]) == v, f"channel {c}: mean is not the constant"
        if v == 0.0:    # another constant: shift rounds at |c gamma| eps^-1/2, and z is held to its bound above
            b = inp["beta"][c]
            assert torch.equal(got["z"][:, c], _leaky(b).expand_as(got["z"][:, c])), f"channel {c}: z is not leaky_relu(beta)"


@pytest.mark.parametrize("shape", [(5, 4, 31, 31), (2, 3, 65, 65)])
def test_optional_pointers_change_nothing_else(device, shape):
    inp, _ = _case("diffuse", shape)
    full = _abi(inp, device)

    def same(got, names):
        for name in names:
            assert torch.equal(got[name], full[name]), name

    got = _abi(inp, device, param_grads=False)
    assert got["dgamma"] is None and got["dbeta"] is None
    same(got, ("z", "mean", "rstd", "run_mean", "run_var", "gx", "sums", "g_gz", "g_x", "g_gamma"))
    got = _abi(inp, device, running=False)
    same(got, ("z", "mean", "rstd", "gx", "sums", "dgamma", "dbeta", "g_gz", "g_x", "g_gamma"))
    got = _abi(inp, device, g_gamma=False)
    assert got["g_gamma"] is None
    same(got, ("z", "gx", "sums", "g_gz", "g_x"))
    null, zeros = _abi(inp, device, gg="null"), _abi(inp, device, gg="zeros")
    for name in ("g_gz", "g_x", "g_gamma"):
        assert torch.equal(null[name], zeros[name]), name
    _, R0 = _case("diffuse", shape, gg=False)
    _check(null, R0, f"gg null {shape}", "diffuse")


# ---------------------------------------------------------------------------------------------- through autograd
def _bn(inp, device):
    C = inp["gamma"].numel()
    bn = nn.BatchNorm2d(C)
    assert bn.eps == 1e-5 and bn.momentum == 0.1
    with torch.no_grad():
        bn.weight.copy_(inp["gamma"])
        bn.bias.copy_(inp["beta"])
        bn.running_mean.copy_(inp["run_mean"])
        bn.running_var.copy_(inp["run_var"])
    return bn.to(device)


def _off_by_4_bytes(t):
    """t's values in storage that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _autograd(inp, device, full, shift=()):
    """ops.bn_leaky_relu and its gradients through torch.autograd.grad.  full: <ggx, gx> + <gg_gamma, dgamma> + <gg_beta,
    dbeta> differentiated; else the gradient penalty's structure under input_grad_only() (no ggw / ggb reach the double
    backward).  shift: the names of x / gz / ggx handed over 4 bytes off alignment."""
    from amk import ops
    from amk.models.discriminator import input_grad_only

    bn = _bn(inp, device)
    t = {k: (_off_by_4_bytes(inp[k].to(device)) if k in shift else inp[k].to(device)) for k in ("x", "gz", "ggx")}
    x, gz, ggx = t["x"].requires_grad_(), t["gz"].requires_grad_(), t["ggx"]
    assert ops.bn_leaky_relu_ok(bn, x)
    z = ops.bn_leaky_relu(x, bn, ref.SLOPE)
    out = dict(z=z.detach(), run_mean=bn.running_mean.clone(), run_var=bn.running_var.clone())
    assert int(bn.num_batches_tracked) == 1
    if full:
        gx, gw, gb = torch.autograd.grad(z, (x, bn.weight, bn.bias), gz, create_graph=True)
        out.update(dgamma=gw.detach(), dbeta=gb.detach())
        g_x, g_w, g_b, g_gz = torch.autograd.grad((gx, gw, gb), (x, bn.weight, bn.bias, gz),
                                                  (ggx, inp["gg_gamma"].to(device), inp["gg_beta"].to(device)), allow_unused=True)
    else:
        with input_grad_only():
            (gx,) = torch.autograd.grad(z, x, gz, create_graph=True)
        g_x, g_w, g_b, g_gz = torch.autograd.grad(gx, (x, bn.weight, bn.bias, gz), ggx, allow_unused=True)
    assert g_b is None                                  # the double backward has no beta gradient
    out.update(gx=gx.detach(), g_x=g_x, g_gamma=g_w, g_gz=g_gz)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("full", [False, True], ids=["input_grad_only", "full_second_order"])
@pytest.mark.parametrize("shape", [(5, 4, 31, 31), (2, 3, 65, 65)])
@pytest.mark.parametrize("family", ["diffuse", "mean_heavy"])
def test_autograd_within_bounds(device, family, shape, full):
    inp, R = _case(family, shape, gg=full)
    got = _autograd(inp, device, full)
    assert set(got) == (set(ref.TENSORS) - {"mean", "rstd"} if full else set(ref.TENSORS) - {"mean", "rstd", "dgamma", "dbeta"})
    _check(got, R, f"autograd {'full' if full else 'gp'} {family} {shape}", family)
    # the wrapper adds nothing to the kernels: the same bits as the C ABI called directly
    direct = _abi(inp, device, gg="given" if full else "null")
    for name, v in got.items():
        assert torch.equal(v, direct[name]), name


@pytest.mark.parametrize("gg", ["null", "given"])
@pytest.mark.parametrize("shape", [(5, 4, 31, 31), (2, 3, 65, 65)])
def test_ops_give_the_bits_of_the_abi(device, shape, gg):
    """ops.bn_leaky_relu through autograd -- the first-order gradients with create_graph, then the second grad with a given
    ggx and gg_gamma / gg_beta absent ("null") or given -- gives, bit for bit, what _abi's sequence gives: z, the updated
    running statistics, gx, dgamma, dbeta, g_gz, g_x and g_gamma."""
    from amk import ops

    inp, _ = _case("diffuse", shape)
    bn = _bn(inp, device)
    x, gz = inp["x"].to(device).requires_grad_(), inp["gz"].to(device).requires_grad_()
    z = ops.bn_leaky_relu(x, bn, ref.SLOPE)
    got = dict(z=z.detach(), run_mean=bn.running_mean.clone(), run_var=bn.running_var.clone())
    gx, gw, gb = torch.autograd.grad(z, (x, bn.weight, bn.bias), gz, create_graph=True)
    got.update(gx=gx.detach(), dgamma=gw.detach(), dbeta=gb.detach())
    outs, cots = ((gx,), (inp["ggx"],)) if gg == "null" else ((gx, gw, gb), (inp["ggx"], inp["gg_gamma"], inp["gg_beta"]))
    got["g_gz"], got["g_x"], got["g_gamma"] = torch.autograd.grad(outs, (gz, x, bn.weight), [c.to(device) for c in cots])
    torch.cuda.synchronize()
    want = _abi(inp, device, gg=gg)
    for name, v in got.items():
        assert v.dtype == want[name].dtype and torch.equal(v, want[name]), name


@pytest.mark.parametrize("shift", [("x",), ("gz",), ("ggx",), ("x", "gz", "ggx")], ids=lambda s: "+".join(s))
def test_storage_4_bytes_off_alignment_gives_the_same_bits(device, shift):
    inp, _ = _case("diffuse", (2, 3, 65, 65))
    for full in (False, True):
        want, got = _autograd(inp, device, full), _autograd(inp, device, full, shift=shift)
        for name in want:
            assert torch.equal(got[name], want[name]), (name, full)


def test_zz_report_worst_ratios(capsys):
    """The figures of the "Measured" block of discr_norm_ref's docstring: over all families, and per family."""
    with capsys.disabled():
        print("\ndiscr_norm worst |got - ref| / bound:", {k: round(v, 4) for k, v in sorted(ref.WORST.items())})
        for family in ref.FAMILIES:
            print("discr_norm worst,", family, {n: round(ref.WORST_BY_FAMILY[(family, n)], 4) for n in ref.TENSORS
                                                if (family, n) in ref.WORST_BY_FAMILY})
    assert all(v <= 1.0 for v in ref.WORST.values())
