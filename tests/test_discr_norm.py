"""CPU checks of the BatchNorm2d + LeakyReLU spec (tests/discr_norm_spec.py) that csrc/discr_norm.hip implements:
float64 against autograd of nn.BatchNorm2d + nn.LeakyReLU, gradcheck / gradgradcheck of its autograd structure, the
C ABI's bindings, and the module fallbacks that keep CPU runs on the modules."""
import pytest
import torch
import torch.nn as nn

import discr_norm_spec as spec

SHAPES = [(2, 3, 5, 7), (3, 6, 4, 4), (1, 5, 9, 1), (2, 4, 31, 31)]
EPS, SLOPE = 1e-5, 0.2


def _setup(shape, seed):
    g = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    x = (1.5 + torch.randn(shape, generator=g, dtype=torch.float64)).requires_grad_()
    gamma = (1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_()
    beta = (0.3 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_()
    return g, x, gamma, beta


def _autograd_z(x, gamma, beta):
    bn = nn.BatchNorm2d(x.shape[1], eps=EPS).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    bn.train()
    return nn.functional.leaky_relu(nn.functional.batch_norm(x, None, None, gamma, beta, True, 0.1, EPS), SLOPE)


def _close(a, b, tol=1e-12):
    a, b = a.detach(), b.detach()
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol * max(scale, 1.0), (float((a - b).abs().max()), scale)


@pytest.mark.parametrize("shape", SHAPES)
def test_spec_matches_autograd(shape):
    g, x, gamma, beta = _setup(shape, 1)
    z_ref = _autograd_z(x, gamma, beta)
    z, mu, r = spec.fwd(x, gamma, beta, EPS, SLOPE)
    _close(z, z_ref)

    gz = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_()
    gx_r, gw_r, gb_r = torch.autograd.grad(z_ref, (x, gamma, beta), gz, create_graph=True)
    gx, gw, gb = spec.bwd(gz, x.detach(), gamma.detach(), beta.detach(), mu.detach(), r.detach(), SLOPE)
    _close(gx, gx_r)
    _close(gw, gw_r)
    _close(gb, gb_r)

    ggx = torch.randn(shape, generator=g, dtype=torch.float64)
    ggw = torch.randn(shape[1], generator=g, dtype=torch.float64)
    ggb = torch.randn(shape[1], generator=g, dtype=torch.float64)
    for with_params in (False, True):
        outs, grads = [gx_r], [ggx]
        if with_params:
            outs, grads = [gx_r, gw_r, gb_r], [ggx, ggw, ggb]
        d_gz, d_x, d_w, d_b = torch.autograd.grad(outs, (gz, x, gamma, beta), grads, retain_graph=True, allow_unused=True)
        g_gz, g_x, g_w = spec.bwd_bwd(ggx, ggw if with_params else None, ggb if with_params else None, gz.detach(),
                                      x.detach(), gamma.detach(), beta.detach(), mu.detach(), r.detach(), SLOPE)
        _close(g_gz, d_gz)
        _close(g_x, d_x)
        _close(g_w, d_w)
        assert d_b is None or float(d_b.abs().max()) < 1e-12


@pytest.mark.parametrize("shape", [(2, 3, 3, 5), (3, 2, 2, 3)])
def test_spec_gradcheck(shape):
    _, x, gamma, beta = _setup(shape, 2)
    f = lambda x, w, b: spec.BNAct.apply(x, w, b, EPS, SLOPE)  # noqa: E731
    assert torch.autograd.gradcheck(f, (x, gamma, beta))
    assert torch.autograd.gradgradcheck(f, (x, gamma, beta))


def test_bindings_declared():
    from amk import lib

    names = set(lib.declared_symbols())
    for n in ("amk_bnact_ws_floats", "amk_bnact_fwd", "amk_bnact_bwd", "amk_bnact_bwd_bwd"):
        assert n in names and n in lib.SIGNATURES


def test_cpu_and_eval_keep_modules(monkeypatch):
    from amk import ops
    from amk.models.discriminator import NLayerDiscriminator

    def boom(*a, **k):
        raise AssertionError("fused BatchNorm + LeakyReLU taken on a path that must keep the modules")

    monkeypatch.setattr(ops, "bn_leaky_relu", boom)
    torch.manual_seed(0)
    d = NLayerDiscriminator(3, 8, 3)
    x = torch.randn(2, 3, 64, 64)
    y_train = d(x)
    assert int(d.model[3].num_batches_tracked) == 1
    d.eval()
    y_eval = d(x)
    assert y_train.shape == y_eval.shape
    assert sorted(d.state_dict()) == sorted(NLayerDiscriminator(3, 8, 3).state_dict())
