"""csrc/discr_norm.hip with T = __bf16 on the MI355X (amk_bnact_bf16_*, ops.bn_leaky_relu_bf16) against the fp64 reference
and the per-element conditions of tests/discr_norm_bf16_ref.py: every output of the three entry points through the C ABI,
called the way amk.ops calls it, on every input family and every shape of the f32 tests plus three that only the bf16 walk
cares about (plane bases on every residue mod 8, planes with no body, odd pieces of a plane above the segment); through
autograd with and without input_grad_only(); dtypes; reproducibility; dispatch in NLayerDiscriminator; the whole PatchGAN
under bf16 autocast against an fp64 run of the modules, with the module path under the same autocast as the yardstick; and one
GAN train step under autocast.

Whole PatchGAN (test_patchgan_under_autocast_against_fp64): per tensor, dev = max |got - fp64| / max |fp64| of the fused path
may be at most 2 times that of the modules, and the same in rms at most 1.5 times: the margins the GroupNorm op needed on its
own whole-model test (tests/test_vqgan_bf16_gpu.py: 1.62 and 1.21 measured there).  Measured on the MI355X over the 15
tensors (output, input gradient, 13 parameter gradients): worst ratio fused / modules 1.25 in max (grad:model.8.weight,
2.00e-1 against 1.60e-1), 1.00 in rms; 9 of the 15 tensors are nearer the fp64 run on the fused path in max, 13 in rms.  The
module path's own deviation: output 1.2e-2, input gradient 1.6e-1, parameter gradients up to 1.6e-1 in max, 9e-2 in rms
(bf16 convolutions and their double backward; the norm is a small part of it).  Also in DESIGN.md section 4c.

AMK_DISCR_NORM_BF16_BOUND_REPORT=<file>: write the worst ratio per tensor over this module to that JSON file."""
import json
import os

import pytest
import torch
import torch.nn as nn

import discr_norm_bf16_ref as bref

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
KEPT = [(5, 4, 31, 31), (2, 3, 65, 65), (1, 2, 67, 67)]
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AMK_DISCR_NORM_BF16_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            by_family = {fam: {n: v for (f2, n), v in bref.WORST_BY_FAMILY.items() if f2 == fam} for fam in bref.FAMILIES}
            json.dump({"all": bref.WORST, "by_family": by_family}, f, indent=1, sort_keys=True)


def _case(family, shape, gg=True):
    """(inputs on the CPU, reference), never modified; kept for the module only on the shapes that several tests share.
    gg=False: gg_gamma = gg_beta = 0."""
    key = (family, shape, gg)
    if key in _CACHE:
        return _CACHE[key]
    inp = bref.make_inputs(family, shape)
    if not gg:
        inp["gg_gamma"], inp["gg_beta"] = torch.zeros_like(inp["gamma"]), torch.zeros_like(inp["beta"])
    case = (inp, bref.reference(inp, family))
    if shape in KEPT:
        _CACHE[key] = case
    return case


def _dev(inp, device):
    """The inputs on the device in the dtypes the kernels take: x, gz and ggx bf16 (exact: they are bf16 values), the rest f32."""
    return {k: v.to(device=device, dtype=BF16 if k in bref.BF16_INPUTS else F32).contiguous() for k, v in inp.items()}


def _abi(inp, device, gg="given"):
    """amk_bnact_bf16_fwd, _bwd and _bwd_bwd as ops._BNActBF16 / _BNActGradBF16 call them."""
    from amk import lib, ops

    L, P = lib.load(), ops._ptr
    t = _dev(inp, device)
    x, gz, ggx, gamma, beta = t["x"], t["gz"], t["ggx"], t["gamma"], t["beta"]
    N, C, H, W = x.shape
    HW = H * W
    ws = lambda: torch.empty(int(L.amk_bnact_ws_floats(N, C, HW)), device=device, dtype=F32)  # noqa: E731
    vec = lambda: torch.empty(C, device=device, dtype=F32)  # noqa: E731
    z, mean, rstd = torch.empty_like(x), vec(), vec()
    rm, rv = t["run_mean"].clone(), t["run_var"].clone()
    lib.check(L.amk_bnact_bf16_fwd(P(x), P(gamma), P(beta), N, C, HW, bref.EPS, bref.MOMENTUM, bref.SLOPE, P(z), P(mean),
                                   P(rstd), P(rm), P(rv), P(ws()), ops._stream()), "amk_bnact_bf16_fwd")
    gx, sums, dgamma, dbeta = torch.empty_like(x), torch.empty(2, C, device=device, dtype=F32), vec(), vec()
    lib.check(L.amk_bnact_bf16_bwd(P(gz), P(x), P(gamma), P(beta), P(mean), P(rstd), N, C, HW, bref.SLOPE, P(gx), P(sums),
                                   P(dgamma), P(dbeta), P(ws()), ops._stream()), "amk_bnact_bf16_bwd")
    ggg, ggb = {"given": (t["gg_gamma"], t["gg_beta"]), "null": (None, None)}[gg]
    g_gz, g_x, g_g = torch.empty_like(x), torch.empty_like(x), vec()
    lib.check(L.amk_bnact_bf16_bwd_bwd(P(ggx), P(ggg), P(ggb), P(gz), P(x), P(gamma), P(beta), P(mean), P(rstd), P(sums), N, C,
                                       HW, bref.SLOPE, P(g_gz), P(g_x), P(g_g), P(ws()), ops._stream()),
              "amk_bnact_bf16_bwd_bwd")
    torch.cuda.synchronize()
    return dict(z=z, mean=mean, rstd=rstd, run_mean=rm, run_var=rv, gx=gx, sums=sums, dgamma=dgamma, dbeta=dbeta, g_gz=g_gz,
                g_x=g_x, g_gamma=g_g)


def _check(got, R, tag, family):
    names = [n for n in bref.TENSORS if got.get(n) is not None]
    got = {k: got[k].cpu() for k in names}
    for name in names:
        assert got[name].dtype == (BF16 if name in bref.ROUNDED else F32), name
    q = bref.ratios(got, R, names=names, family=family)
    print(tag, {k: round(v, 4) for k, v in q.items()})
    for name, v in q.items():
        assert v <= 1.0, f"{tag}: {name} at {v:.3f} of its bound"
    for name in names:
        if name in bref.ROUNDED:
            ok = bref.inside(got[name].to(F64).reshape(R[name].shape), R, name)
            assert bool(ok.all()), f"{tag}: {int((~ok).sum())} elements of {name} outside RNE's image of their bound"
    return q


# ---------------------------------------------------------------------------------------------- bounds, through the C ABI
@pytest.mark.parametrize("shape", bref.SHAPES)
@pytest.mark.parametrize("family", bref.FAMILIES)
def test_kernels_within_bounds(device, family, shape):
    inp, R = _case(family, shape)
    got = {k: v.cpu() for k, v in _abi(inp, device).items()}
    _check(got, R, f"{family} {shape}", family)
    assert all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    assert torch.equal(got["sums"][0], got["dbeta"]) and torch.equal(got["sums"][1], got["dgamma"])
    C, HW = shape[1], shape[2] * shape[3]
    for c, b in bref.ref.dead_channels(family, C, HW).items():
        b32 = torch.tensor(b, dtype=F32)
        want = (b32 if b > 0 else torch.tensor(bref.SLOPE, dtype=F32) * b32).to(BF16)
        assert bool((got["z"][:, c] == want).all()), f"channel {c}: z is not RNE(leaky_relu(beta))"
        assert not bool(got["gx"][:, c].any()), f"channel {c}: gx is not zero"
    for c, v in bref.ref.flat_channels(family, C).items():
        assert float(got["mean"][c]) == v, f"channel {c}: mean is not the constant"


# ---------------------------------------------------------------------------------------------- through autograd
def _bn(inp, device):
    bn = nn.BatchNorm2d(inp["gamma"].numel())
    with torch.no_grad():
        bn.weight.copy_(inp["gamma"])
        bn.bias.copy_(inp["beta"])
        bn.running_mean.copy_(inp["run_mean"])
        bn.running_var.copy_(inp["run_var"])
    return bn.to(device)


def _autograd(inp, device, full, cot_dtype=BF16):
    """ops.bn_leaky_relu_bf16 and its gradients through torch.autograd.grad.  full: <ggx, gx> + <gg_gamma, dgamma> + <gg_beta,
    dbeta> differentiated; else the gradient penalty's structure under input_grad_only() (no ggw / ggb reach the double
    backward).  cot_dtype: the dtype in which the cotangent of gx is handed over."""
    from amk import ops
    from amk.models.discriminator import input_grad_only

    bn = _bn(inp, device)
    t = _dev(inp, device)
    x, gz, ggx = t["x"].requires_grad_(), t["gz"].requires_grad_(), t["ggx"]
    assert ops.bn_leaky_relu_bf16_ok(bn, x) and not ops.bn_leaky_relu_ok(bn, x)
    z = ops.bn_leaky_relu_bf16(x, bn, bref.SLOPE)
    out = dict(z=z.detach(), run_mean=bn.running_mean.clone(), run_var=bn.running_var.clone())
    assert int(bn.num_batches_tracked) == 1
    if full:
        gx, gw, gb = torch.autograd.grad(z, (x, bn.weight, bn.bias), gz, create_graph=True)
        out.update(dgamma=gw.detach(), dbeta=gb.detach())
        g_x, g_w, g_b, g_gz = torch.autograd.grad((gx, gw, gb), (x, bn.weight, bn.bias, gz),
                                                  (ggx, t["gg_gamma"], t["gg_beta"]), allow_unused=True)
    else:
        with input_grad_only():
            (gx,) = torch.autograd.grad(z, x, gz, create_graph=True)
        g_x, g_w, g_b, g_gz = torch.autograd.grad(gx, (x, bn.weight, bn.bias, gz), ggx.to(cot_dtype), allow_unused=True)
    assert g_b is None                                  # the double backward has no beta gradient
    out.update(gx=gx.detach(), g_x=g_x, g_gamma=g_w, g_gz=g_gz)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("full", [False, True], ids=["input_grad_only", "full_second_order"])
@pytest.mark.parametrize("shape", [(5, 4, 31, 31), (1, 2, 67, 67)])
@pytest.mark.parametrize("family", ["diffuse", "mean_heavy"])
def test_autograd_within_bounds(device, family, shape, full):
    inp, R = _case(family, shape, gg=full)
    got = _autograd(inp, device, full)
    assert set(got) == (set(bref.TENSORS) - {"mean", "rstd"} if full else set(bref.TENSORS) - {"mean", "rstd", "dgamma", "dbeta"})
    _check(got, R, f"autograd {'full' if full else 'gp'} {family} {shape}", family)
    # the wrapper adds nothing to the kernels: the same bits as the C ABI called directly
    direct = _abi(inp, device, gg="given" if full else "null")
    for name, v in got.items():
        assert torch.equal(v, direct[name]), name


@pytest.mark.parametrize("gg", ["null", "given"])
@pytest.mark.parametrize("shape", [(5, 4, 31, 31), (1, 2, 67, 67)])
def test_ops_give_the_bits_of_the_abi(device, shape, gg):
    """ops.bn_leaky_relu_bf16 through autograd -- the first-order gradients with create_graph, then the second grad with a
    given ggx and gg_gamma / gg_beta absent ("null") or given -- gives, bit for bit, what _abi's sequence gives: z, the
    updated running statistics, gx, dgamma, dbeta, g_gz, g_x and g_gamma."""
    from amk import ops

    inp, _ = _case("diffuse", shape)
    bn = _bn(inp, device)
    t = _dev(inp, device)
    x, gz = t["x"].requires_grad_(), t["gz"].requires_grad_()
    z = ops.bn_leaky_relu_bf16(x, bn, bref.SLOPE)
    got = dict(z=z.detach(), run_mean=bn.running_mean.clone(), run_var=bn.running_var.clone())
    gx, gw, gb = torch.autograd.grad(z, (x, bn.weight, bn.bias), gz, create_graph=True)
    got.update(gx=gx.detach(), dgamma=gw.detach(), dbeta=gb.detach())
    outs, cots = ((gx,), (t["ggx"],)) if gg == "null" else ((gx, gw, gb), (t["ggx"], t["gg_gamma"], t["gg_beta"]))
    got["g_gz"], got["g_x"], got["g_gamma"] = torch.autograd.grad(outs, (gz, x, bn.weight), cots)
    torch.cuda.synchronize()
    want = _abi(inp, device, gg=gg)
    for name, v in got.items():
        assert v.dtype == want[name].dtype and torch.equal(v, want[name]), name


def test_dtypes_and_running_statistics(device):
    """bf16: z, gx, g_gz, g_x.  f32: dgamma, dbeta, g_gamma, the running statistics.  One update of the running statistics and
    of num_batches_tracked per call.  An f32 cotangent is brought to bf16 and gives the bits of the bf16 one."""
    from amk import ops

    inp, _ = _case("diffuse", (5, 4, 31, 31))
    for full in (False, True):
        got = _autograd(inp, device, full)
        for name, v in got.items():
            assert v.dtype == (BF16 if name in bref.ROUNDED else F32), (name, v.dtype)
    want, got = _autograd(inp, device, False), _autograd(inp, device, False, cot_dtype=F32)
    for name in want:
        assert torch.equal(want[name], got[name]), name
    bn = _bn(inp, device)
    x = _dev(inp, device)["x"]
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    z1 = ops.bn_leaky_relu_bf16(x, bn, bref.SLOPE)
    rm1, rv1 = bn.running_mean.clone(), bn.running_var.clone()
    assert int(bn.num_batches_tracked) == 1 and not torch.equal(rm0, rm1) and not torch.equal(rv0, rv1)
    assert bn.running_mean.dtype == F32 and bn.running_var.dtype == F32
    z2 = ops.bn_leaky_relu_bf16(x, bn, bref.SLOPE)
    assert int(bn.num_batches_tracked) == 2 and torch.equal(z1, z2)
    # the second call starts from the first one's statistics: the bits of the C ABI handed those
    second = _abi(dict(inp, run_mean=rm1.cpu(), run_var=rv1.cpu()), device)
    assert torch.equal(bn.running_mean, second["run_mean"]) and torch.equal(bn.running_var, second["run_var"])
    with torch.no_grad():
        assert ops.bn_leaky_relu_bf16(x, bn, bref.SLOPE).grad_fn is None


def test_reproducible_and_independent_of_the_batch(device):
    """Two runs give the same bits.  A batch of 2N made of two copies of a batch of N gives the same z rows: at (4, 4, 31, 31)
    the batch of 4 is one segment per channel and the batch of 8 two segments with the same values at the same alignment
    (16 planes of 961 elements apart, a multiple of 8), so the partials are equal to the bit, Chan's merge of two equal
    triples returns their mean unchanged and twice their M2, and mean, rstd and z come out to the bit."""
    for shape in [(5, 4, 31, 31), (1, 2, 67, 67)]:
        inp, _ = _case("diffuse", shape)
        a, b = _abi(inp, device), _abi(inp, device)
        for name in a:
            assert torch.equal(a[name], b[name]), (shape, name)
    inp = bref.make_inputs("diffuse", (4, 4, 31, 31))
    assert bref.make_geo(4, 4, 961)["S"] == 1 and bref.make_geo(8, 4, 961)["S"] == 2
    a = _abi(inp, device)
    c = _abi({k: (torch.cat([v, v]) if k in bref.BF16_INPUTS else v) for k, v in inp.items()}, device)
    assert torch.equal(c["mean"], a["mean"]) and torch.equal(c["rstd"], a["rstd"])
    assert torch.equal(c["z"][:4], a["z"]) and torch.equal(c["z"][4:], a["z"])


# ---------------------------------------------------------------------------------------------- dispatch
def test_dispatch_in_the_discriminator(device, monkeypatch):
    from amk import ops
    from amk.models.discriminator import NLayerDiscriminator

    calls = []
    real = ops.bn_leaky_relu_bf16

    def counting(*a, **k):
        calls.append(a[0].dtype)
        return real(*a, **k)

    monkeypatch.setattr(ops, "bn_leaky_relu_bf16", counting)
    monkeypatch.delenv("AMK_DISCR_NORM", raising=False)
    monkeypatch.setenv("AMK_DISCR_NORM_BF16", "1")
    torch.manual_seed(0)
    d = NLayerDiscriminator(3, 16, 3).to(device)
    x = torch.rand(2, 3, 64, 64, device=device)

    def run(inp=x):
        calls.clear()
        with torch.autocast("cuda", dtype=BF16):
            out = d(inp)
        return len(calls), out

    n, out = run()
    assert n == 3 and calls == [BF16] * 3 and out.dtype == BF16 and bool(torch.isfinite(out.float()).all())
    assert int(d.model[3].num_batches_tracked) == 1
    calls.clear()
    d(x)                                                     # f32 outside autocast: the f32 op, not this one
    assert not calls
    monkeypatch.setenv("AMK_DISCR_NORM_BF16", "0")
    assert run()[0] == 0
    monkeypatch.setenv("AMK_DISCR_NORM_BF16", "1")
    monkeypatch.setenv("AMK_DISCR_NORM", "aten")
    assert run()[0] == 0
    monkeypatch.delenv("AMK_DISCR_NORM")
    d.eval()
    assert run()[0] == 0
    d.train()
    assert run(x.contiguous(memory_format=torch.channels_last))[0] == 0
    assert run()[0] == 3
    # bf16 parameters, f16 and non-contiguous inputs keep the modules
    bn = nn.BatchNorm2d(8).to(device)
    xb = torch.randn(2, 8, 5, 5, device=device, dtype=BF16)
    assert ops.bn_leaky_relu_bf16_ok(bn, xb)
    assert not ops.bn_leaky_relu_bf16_ok(bn, xb.half()) and not ops.bn_leaky_relu_bf16_ok(bn, xb.float())
    assert not ops.bn_leaky_relu_bf16_ok(bn, xb.permute(0, 1, 3, 2)) and not ops.bn_leaky_relu_bf16_ok(bn, xb.cpu())
    assert not ops.bn_leaky_relu_bf16_ok(nn.BatchNorm2d(8).to(device).to(BF16), xb)
    assert not ops.bn_leaky_relu_bf16_ok(nn.BatchNorm2d(8, affine=False).to(device), xb)
    assert not ops.bn_leaky_relu_bf16_ok(nn.BatchNorm2d(8, track_running_stats=False).to(device), xb)
    assert not ops.bn_leaky_relu_bf16_ok(nn.BatchNorm2d(8, momentum=None).to(device), xb)
    assert not ops.bn_leaky_relu_bf16_ok(bn, xb[:1, :, :1, :1])


# ---------------------------------------------------------------------------------------------- whole PatchGAN
def _gan_pass(d, img, amp):
    """pred, the GP-style input gradient, and the parameter gradients of pred.mean() + penalty."""
    from amk.models.discriminator import input_grad_only

    x = img.clone().requires_grad_()
    with torch.autocast("cuda", dtype=BF16, enabled=amp):
        pred = d(x)
    with input_grad_only():
        (g,) = torch.autograd.grad(pred, x, torch.ones_like(pred), create_graph=True)
    loss = pred.float().mean() + (g.flatten(1).norm(dim=1) - 1).pow(2).mean() if amp else \
        pred.mean() + (g.flatten(1).norm(dim=1) - 1).pow(2).mean()
    loss.backward()
    out = {"pred": pred.detach(), "input_grad": g.detach()}
    out.update({"grad:" + n: p.grad.clone() for n, p in d.named_parameters()})
    return {k: v.double().cpu() for k, v in out.items()}


def test_patchgan_under_autocast_against_fp64(device, monkeypatch):
    from amk import ops
    from amk.models.discriminator import NLayerDiscriminator

    torch.manual_seed(1)
    d_on = NLayerDiscriminator(3, 32, 3).to(device)
    d_off = NLayerDiscriminator(3, 32, 3).to(device)
    d_off.load_state_dict(d_on.state_dict())
    d64 = NLayerDiscriminator(3, 32, 3)
    d64.load_state_dict(d_on.state_dict())
    d64 = d64.double()
    img = torch.rand(4, 3, 64, 64, device=device)
    calls = []
    real = ops.bn_leaky_relu_bf16
    monkeypatch.setattr(ops, "bn_leaky_relu_bf16", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.delenv("AMK_DISCR_NORM", raising=False)
    monkeypatch.setenv("AMK_DISCR_NORM_BF16", "1")
    on = _gan_pass(d_on, img, True)
    assert len(calls) == 3
    monkeypatch.setenv("AMK_DISCR_NORM_BF16", "0")
    off = _gan_pass(d_off, img, True)
    assert len(calls) == 3
    want = {k: v for k, v in _gan_pass_cpu64(d64, img.cpu().double()).items()}
    assert set(on) == set(off) == set(want)
    dev = lambda got, k: (float((got[k] - want[k]).abs().max() / want[k].abs().max()),  # noqa: E731
                          float((got[k] - want[k]).pow(2).mean().sqrt() / want[k].pow(2).mean().sqrt()))
    worst = [0.0, 0.0]
    for k in sorted(want):
        (a_max, a_rms), (b_max, b_rms) = dev(on, k), dev(off, k)
        print(f"{k}: fused max {a_max:.3e} rms {a_rms:.3e} | modules max {b_max:.3e} rms {b_rms:.3e}")
        if b_max > 0:
            worst = [max(worst[0], a_max / b_max), max(worst[1], a_rms / b_rms)]
    print(f"worst ratio fused / modules: {worst[0]:.3f} in max, {worst[1]:.3f} in rms")
    for k in sorted(want):
        (a_max, a_rms), (b_max, b_rms) = dev(on, k), dev(off, k)
        assert bool(torch.isfinite(on[k]).all()), k
        # the yardstick must say something: a wrong term in a backward moves a gradient by order 1, so the module path's own
        # deviation has to sit clearly below that (the second-order gradients of this random-weight PatchGAN under bf16
        # convolutions reach 0.16 of a tensor's maximum on the module path: see the module docstring)
        assert b_max < 0.5, f"{k}: the module path itself is {b_max:.3e} from the fp64 run"
        assert a_max <= 2 * b_max, f"{k}: max deviation {a_max:.3e} fused against {b_max:.3e} modules"
        assert a_rms <= 1.5 * b_rms, f"{k}: rms deviation {a_rms:.3e} fused against {b_rms:.3e} modules"


def _gan_pass_cpu64(d, img):
    from amk.models.discriminator import input_grad_only

    x = img.clone().requires_grad_()
    pred = d(x)
    with input_grad_only():
        (g,) = torch.autograd.grad(pred, x, torch.ones_like(pred), create_graph=True)
    (pred.mean() + (g.flatten(1).norm(dim=1) - 1).pow(2).mean()).backward()
    out = {"pred": pred.detach(), "input_grad": g.detach()}
    out.update({"grad:" + n: p.grad.clone() for n, p in d.named_parameters()})
    return out


# ---------------------------------------------------------------------------------------------- train step
def test_train_step_under_autocast_stays_finite(device, monkeypatch):
    """One GAN step at the sizes of tests/test_autocast_gpu.py with the switch on: the three pairs run fused in both phases,
    every loss and parameter stays finite."""
    from amk import ops
    from amk.models import ViTVQGAN
    from amk.models.discriminator import NLayerDiscriminator
    from amk.train import VQGANTrainStep

    calls = []
    real = ops.bn_leaky_relu_bf16
    monkeypatch.setattr(ops, "bn_leaky_relu_bf16", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.delenv("AMK_DISCR_NORM", raising=False)
    monkeypatch.setenv("AMK_DISCR_NORM_BF16", "1")
    torch.manual_seed(0)
    vit = dict(dim=128, img_size=64, patch_size=8, n_heads=2, d_head=64, depth=2, mlp_dim=256, dropout=0.0)
    model = ViTVQGAN(vit, dict(codebook_size=512, codebook_dim=32)).to(device)
    discr = NLayerDiscriminator(3, 16, 3).to(device)
    img = torch.rand(4, 3, 64, 64, device=device)
    logs = VQGANTrainStep(model, discr, autocast=BF16).step(img)
    assert calls and len(calls) % 3 == 0
    assert all(bool(torch.isfinite(v)) for v in logs.values()), {k: float(v) for k, v in logs.items()}
    for p in list(model.parameters()) + list(discr.parameters()):
        assert p.dtype == F32 and bool(torch.isfinite(p).all())
    for b in discr.buffers():
        assert bool(torch.isfinite(b.float()).all())


def test_zz_report_worst_ratios(capsys):
    with capsys.disabled():
        print("\ndiscr_norm_bf16 worst ratios:", {k: round(v, 4) for k, v in sorted(bref.WORST.items())})
        for family in bref.FAMILIES:
            print("discr_norm_bf16 worst,", family, {n: round(bref.WORST_BY_FAMILY[(family, n)], 4) for n in bref.TENSORS
                                                     if (family, n) in bref.WORST_BY_FAMILY})
    assert all(v <= 1.0 for v in bref.WORST.values())
