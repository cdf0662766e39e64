"""torch restatement of the formulas csrc/gn_act.hip implements (GroupNorm(G, C, eps) + optional Swish on NCHW): the spec
the kernels are tested against.  Per sample n and group g (cpg = C / G channels, m = cpg H W values): xh = (x - mu) r,
y = gamma_c xh + beta_c, z = act(y); act 0 = identity, act 1 = swish y sigma(y)."""
import torch


def _c(v):
    return v.view(1, -1, 1, 1)


def _runs(x, G):
    return x.reshape(x.shape[0], G, -1)


def _per_elem(v, x, G):
    """(N, G) per-run values broadcast to x's shape."""
    N, C = x.shape[:2]
    return v.reshape(N, G, 1).expand(N, G, C // G).reshape(N, C, 1, 1)


def act_fwd(y, act):
    return y * torch.sigmoid(y) if act == 1 else y


def act_grad(y, act):
    if act != 1:
        return torch.ones_like(y)
    sg = torch.sigmoid(y)
    return sg * (1 + y * (1 - sg))


def fwd(x, gamma, beta, G, eps, act):
    """z, mean (N, G), rstd (N, G) (biased variance)."""
    xr = _runs(x, G)
    mu = xr.mean(2)
    var = ((xr - mu.unsqueeze(2)) ** 2).mean(2)
    r = (var + eps).rsqrt()
    y = _c(gamma) * ((x - _per_elem(mu, x, G)) * _per_elem(r, x, G)) + _c(beta)
    return act_fwd(y, act), mu, r


def bwd(gz, x, gamma, beta, mu, r, G, act):
    """gx, dgamma, dbeta."""
    xh = (x - _per_elem(mu, x, G)) * _per_elem(r, x, G)
    gy = gz * act_grad(_c(gamma) * xh + _c(beta), act)
    m = x[0].numel() // G
    s1 = _runs(_c(gamma) * gy, G).sum(2)
    s2 = _runs(_c(gamma) * gy * xh, G).sum(2)
    gx = _per_elem(r, x, G) * (_c(gamma) * gy - _per_elem(s1 / m, x, G) - xh * _per_elem(s2 / m, x, G))
    return gx, (gy * xh).sum((0, 2, 3)), gy.sum((0, 2, 3))


class GNAct(torch.autograd.Function):
    """The structure of amk.ops._GNAct on the spec."""

    @staticmethod
    def forward(ctx, x, gamma, beta, G, eps, act):
        z, mu, r = fwd(x, gamma, beta, G, eps, act)
        ctx.save_for_backward(x, gamma, beta, mu, r)
        ctx.G, ctx.act = G, act
        return z

    @staticmethod
    def backward(ctx, gz):
        x, gamma, beta, mu, r = ctx.saved_tensors
        gx, dw, db = bwd(gz, x, gamma, beta, mu, r, ctx.G, ctx.act)
        return gx, dw, db, None, None, None
