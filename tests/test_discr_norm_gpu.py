"""GPU checks of the fused BatchNorm2d + LeakyReLU (csrc/discr_norm.hip through amk.ops.bn_leaky_relu): forward,
running statistics, first-order gradients and the gradient penalty's second-order gradients against the ATen f32 path
on the GPU (1e-4 of each tensor's maximum) and float64 on the CPU; bitwise reproducibility, HIP-graph replay, and the
fallbacks to the modules."""
import pytest
import torch
import torch.nn as nn

from amk import ops
from amk.models.discriminator import NLayerDiscriminator, input_grad_only

pytestmark = pytest.mark.gpu

SLOPE = 0.2
BENCH_SHAPES = [(32, 128, 64, 64), (32, 256, 32, 32), (32, 512, 31, 31)]
SMALL_SHAPES = [(1, 3, 5, 7), (2, 5, 3, 3), (3, 6, 17, 9), (3, 7, 1, 1), (1, 2, 100, 101), (3, 10, 31, 31)]


def _modules(C, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(C, generator=g))
        bn.bias.copy_(0.3 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_var.copy_(1 + 0.1 * torch.rand(C, generator=g))
    return bn


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = 0.7 + 1.3 * torch.randn(shape, generator=g)
    gz = torch.randn(shape, generator=g)
    ggx = torch.randn(shape, generator=g)
    ggw = torch.randn(shape[1], generator=g)
    ggb = torch.randn(shape[1], generator=g)
    return x, gz, ggx, ggw, ggb


def _run(bn, x0, gz0, ggx, ggw, ggb, fused):
    """z, running stats, first-order grads, GP-structure second-order grads (x, gamma, beta, gz) and the full
    second-order grads (with gg_gamma, gg_beta)."""
    x = x0.clone().requires_grad_()
    gz = gz0.clone().requires_grad_()
    if fused:
        assert ops.bn_leaky_relu_ok(bn, x)
        z = ops.bn_leaky_relu(x, bn, SLOPE)
    else:
        z = nn.functional.leaky_relu(bn(x), SLOPE)
    out = {"z": z.detach().clone(), "rm": bn.running_mean.clone(), "rv": bn.running_var.clone(),
           "nbt": bn.num_batches_tracked.clone()}
    gx, gw, gb = torch.autograd.grad(z, (x, bn.weight, bn.bias), gz, create_graph=True)
    out.update(gx=gx.detach().clone(), gw=gw.detach().clone(), gb=gb.detach().clone())
    # the gradient penalty's structure: input gradient only, then differentiate <ggx, gx>
    with input_grad_only():
        (gxp,) = torch.autograd.grad(z, x, gz, create_graph=True)
    d = torch.autograd.grad(gxp, (x, bn.weight, bn.bias, gz), ggx, allow_unused=True, retain_graph=True)
    for k, v in zip(("gp_x", "gp_w", "gp_b", "gp_gz"), d):
        out[k] = torch.zeros_like(bn.bias) if v is None else v.detach().clone()
    d = torch.autograd.grad((gx, gw, gb), (x, bn.weight, bn.bias, gz), (ggx, ggw, ggb), allow_unused=True)
    for k, v in zip(("gg_x", "gg_w", "gg_b", "gg_gz"), d):
        out[k] = torch.zeros_like(bn.bias) if v is None else v.detach().clone()
    return out


def _compare(a, b, tol, what):
    for k in a:
        if k == "nbt":
            assert int(a[k]) == int(b[k]), what
            continue
        x, y = a[k].double().cpu(), b[k].double().cpu()
        scale = max(float(y.abs().max()), 1e-6)
        err = float((x - y).abs().max())
        assert err <= tol * scale, f"{what} {k}: {err:.3e} of max {scale:.3e}"


def _compare_aten(fused, aten, ref, tol):
    """fused within tol of ATen f32, unless ATen itself is farther than that from float64: then fused must be at
    least as close to float64 as ATen.  (MIOpen's batch-norm backward at 32 x 512 x 31 x 31 is: its dgamma / dbeta
    are several per cent off float64 there, gx 6e-4.)"""
    for k in fused:
        if k == "nbt":
            assert int(fused[k]) == int(aten[k])
            continue
        f, a, r = fused[k].double().cpu(), aten[k].double().cpu(), ref[k].double().cpu()
        scale = max(float(r.abs().max()), 1e-6)
        e_fa, e_f, e_a = (float((u - v).abs().max()) for u, v in ((f, a), (f, r), (a, r)))
        assert e_fa <= tol * scale or e_f <= e_a, f"{k}: fused-aten {e_fa:.3e}, fused-f64 {e_f:.3e}, aten-f64 {e_a:.3e}"


@pytest.mark.parametrize("shape", SMALL_SHAPES + BENCH_SHAPES)
def test_against_aten_and_float64(shape, device):
    C = shape[1]
    x, gz, ggx, ggw, ggb = _inputs(shape, 3)
    bn_f, bn_a = _modules(C, 4).to(device), _modules(C, 4).to(device)
    args = [t.to(device) for t in (x, gz, ggx, ggw, ggb)]
    fused = _run(bn_f, *args, fused=True)
    aten = _run(bn_a, *args, fused=False)
    # float64 reference: on the CPU, or for the benchmark's shapes on the GPU (ATen's own float64 kernels)
    ref_dev = "cpu" if shape[0] * C * shape[2] * shape[3] <= (1 << 22) else device
    bn_d = _modules(C, 4).double().to(ref_dev)
    ref = _run(bn_d, *[t.double().to(ref_dev) for t in (x, gz, ggx, ggw, ggb)], fused=False)
    _compare(fused, ref, 1e-4, "vs float64")
    _compare_aten(fused, aten, ref, 1e-4)


@pytest.mark.parametrize("shape", [(3, 6, 17, 9), (32, 512, 31, 31)])
def test_bitwise_reproducible(shape, device):
    x, gz, ggx, ggw, ggb = [t.to(device) for t in _inputs(shape, 5)]
    runs = [_run(_modules(shape[1], 6).to(device), x, gz, ggx, ggw, ggb, fused=True) for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_graph_replay_bitwise(device):
    shape = (4, 16, 31, 31)
    x0, gz0, ggx, _, _ = [t.to(device) for t in _inputs(shape, 7)]
    bn = _modules(shape[1], 8).to(device)
    x = x0.clone().requires_grad_()

    def step():
        z = ops.bn_leaky_relu(x, bn, SLOPE)
        with input_grad_only():
            (gx,) = torch.autograd.grad(z, x, gz0, create_graph=True)
        loss = (z * gz0).sum() + (gx * ggx).sum()
        gxx, gw, gb = torch.autograd.grad(loss, (x, bn.weight, bn.bias))
        return [z.detach(), gx.detach(), gxx, gw, gb]

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, static):
        assert torch.equal(a, b)


def test_fallbacks_keep_modules(device, monkeypatch):
    calls = []
    real = ops.bn_leaky_relu

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "bn_leaky_relu", counting)
    torch.manual_seed(0)
    d = NLayerDiscriminator(3, 16, 3).to(device)
    x = torch.rand(2, 3, 64, 64, device=device)
    d(x)
    assert len(calls) == 3
    assert int(d.model[3].num_batches_tracked) == 1
    calls.clear()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        d(x)
    assert not calls
    d.eval()
    d(x)
    assert not calls
    d.train()
    monkeypatch.setenv("AMK_DISCR_NORM", "aten")
    d(x)
    assert not calls
    d.cpu()(x.cpu())
    assert not calls


def test_discriminator_matches_modules(device, monkeypatch):
    """Whole PatchGAN: fused and module paths agree on the output, the GP-style gradients and the running stats."""
    torch.manual_seed(1)
    d1 = NLayerDiscriminator(3, 32, 3).to(device)
    d2 = NLayerDiscriminator(3, 32, 3).to(device)
    d2.load_state_dict(d1.state_dict())
    img = torch.rand(4, 3, 64, 64, device=device)
    res = []
    for d, mode in ((d1, "amk"), (d2, "aten")):
        monkeypatch.setenv("AMK_DISCR_NORM", mode)
        x = img.clone().requires_grad_()
        pred = d(x)
        with input_grad_only():
            (g,) = torch.autograd.grad(pred, x, torch.ones_like(pred), create_graph=True)
        loss = pred.mean() + (g.flatten(1).norm(dim=1) - 1).pow(2).mean()
        loss.backward()
        res.append([pred.detach(), g.detach()] + [p.grad.clone() for p in d.parameters()]
                   + [b.clone() for b in d.buffers()])
    for a, b in zip(*res):
        if a.dtype == torch.int64:
            assert torch.equal(a, b)
            continue
        scale = max(float(b.abs().max()), 1e-6)
        assert float((a - b).abs().max()) <= 1e-4 * scale
