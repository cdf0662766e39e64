"""torch restatement of the formulas csrc/discr_norm.hip implements (training-mode BatchNorm2d + LeakyReLU on NCHW):
the spec the kernels are tested against.  Per channel, n = N H W; xh = (x - mu) r, y = gamma xh + beta,
z = y > 0 ? y : slope y, s = dz/dy."""
import torch


def _c(v):
    return v.view(1, -1, 1, 1)


def fwd(x, gamma, beta, eps, slope):
    """z, mean, rstd (biased variance)."""
    mu = x.mean((0, 2, 3))
    var = ((x - _c(mu)) ** 2).mean((0, 2, 3))
    r = (var + eps).rsqrt()
    y = _c(gamma) * (x - _c(mu)) * _c(r) + _c(beta)
    return torch.where(y > 0, y, slope * y), mu, r


def _common(gz, x, gamma, beta, mu, r, slope):
    xh = (x - _c(mu)) * _c(r)
    s = torch.where(_c(gamma) * xh + _c(beta) > 0, torch.ones_like(x), torch.full_like(x, slope))
    n = x.numel() // x.shape[1]
    return xh, s, s * gz, n


def bwd(gz, x, gamma, beta, mu, r, slope):
    """gx, dgamma, dbeta."""
    xh, s, gy, n = _common(gz, x, gamma, beta, mu, r, slope)
    sgy, sgyx = gy.sum((0, 2, 3)), (gy * xh).sum((0, 2, 3))
    gx = _c(gamma * r) * (gy - _c(sgy / n) - xh * _c(sgyx / n))
    return gx, sgyx, sgy


def bwd_bwd(ggx, gg_gamma, gg_beta, gz, x, gamma, beta, mu, r, slope):
    """g_gz, g_x, g_gamma of <ggx, gx> + <gg_gamma, dgamma> + <gg_beta, dbeta> (the beta gradient is zero)."""
    xh, s, gy, n = _common(gz, x, gamma, beta, mu, r, slope)
    if gg_gamma is None:
        gg_gamma = torch.zeros_like(gamma)
    if gg_beta is None:
        gg_beta = torch.zeros_like(beta)
    A = gy.sum((0, 2, 3)) / n
    B = (gy * xh).sum((0, 2, 3)) / n
    C = ggx.sum((0, 2, 3)) / n
    D = (ggx * xh).sum((0, 2, 3)) / n
    E = (ggx * gy).sum((0, 2, 3)) / n
    gr = _c(gamma * r)
    g_gz = s * (gr * (ggx - _c(C) - xh * _c(D)) + _c(gg_gamma) * xh + _c(gg_beta))
    g_x = (-_c(gamma * r * r) * (xh * _c(E - A * C - 3 * B * D) + _c(B) * (ggx - _c(C)) + _c(D) * (gy - _c(A)))
           + _c(gg_gamma * r) * (gy - _c(A) - xh * _c(B)))
    g_gamma = n * r * (E - A * C - B * D)
    return g_gz, g_x, g_gamma


class BNActGrad(torch.autograd.Function):
    """The structure of amk.ops._BNActGrad on the spec: (gx, dgamma, dbeta), backward = bwd_bwd."""

    @staticmethod
    def forward(ctx, gz, x, gamma, beta, mu, r, slope):
        ctx.save_for_backward(gz, x, gamma, beta, mu, r)
        ctx.slope = slope
        return bwd(gz, x, gamma, beta, mu, r, slope)

    @staticmethod
    def backward(ctx, ggx, ggw, ggb):
        gz, x, gamma, beta, mu, r = ctx.saved_tensors
        g_gz, g_x, g_gamma = bwd_bwd(ggx, ggw, ggb, gz, x, gamma, beta, mu, r, ctx.slope)
        return g_gz, g_x, g_gamma, None, None, None, None


class BNAct(torch.autograd.Function):
    """The structure of amk.ops._BNAct on the spec."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, slope):
        z, mu, r = fwd(x, gamma, beta, eps, slope)
        ctx.save_for_backward(x, gamma, beta, mu, r)
        ctx.slope = slope
        return z

    @staticmethod
    def backward(ctx, gz):
        x, gamma, beta, mu, r = ctx.saved_tensors
        gx, dw, db = BNActGrad.apply(gz, x, gamma, beta, mu, r, ctx.slope)
        return gx, dw, db, None, None
