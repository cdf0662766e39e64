"""AgentAttention at head dims 32 and 128 on the GPU: the module against the reference-pinned fixtures, against the
CPU oracle over chunk-boundary shapes, the full-size properties (batch independence, bitwise repeat, oracle) and a
forward + backward under bf16 autocast."""
import pytest
import torch

from oracle import ref_cpu
from oracle.fixture_recipe import seeded, seeded_params
from util import assert_close, load_golden, weights_of

pytestmark = pytest.mark.gpu
TOL = 2e-5
DIMS = [32, 128]


def _abs_close(a, b, tol, what):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    scale = max(float(b.abs().max()), 1e-3)
    err = float((a - b).abs().max())
    assert err <= tol * scale * 5, f"{what}: abs err {err:.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("d", DIMS)
def test_agent_head_dim_golden(device, d):
    from amk.models import AgentAttention

    fx = load_golden(f"agent_d{d}")
    dim, h, dd, agent_num = (int(v) for v in fx["dims"])
    assert dd == d
    m = AgentAttention(dim, h, d, agent_num=agent_num)
    res = m.load_state_dict(weights_of(fx), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m = m.to(device)
    x = torch.from_numpy(fx["x"]).to(device).requires_grad_(True)
    out = m(x)
    assert_close(out, fx["out"], TOL, "out")
    (out * torch.from_numpy(fx["cot"]).to(device)).sum().backward()
    assert_close(x.grad, fx["gx"], TOL, "grad x")
    for n, p in m.named_parameters():
        if n in ("bias1", "bias2"):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
            continue
        _abs_close(p.grad, fx["g:" + n], TOL, f"grad {n}")


# test_agent_vs_oracle's list: ragged bins, T < chunk, a last chunk of one token, an exactly full chunk (128-token
# chunks: 256 / 513 / 129), P = 1, P <= 8 and 8 < P <= 16; for the 64-token chunks of D = 128 also T = 64 (one full
# chunk) and T = 65 (a last chunk of one token)
SHAPES = [(2, 10, 384, 6, 47), (1, 1024, 384, 6, 47), (2, 65, 256, 4, 16), (1, 300, 128, 2, 4), (1, 37, 64, 1, 1),
          (1, 513, 128, 2, 4), (2, 256, 192, 3, 9), (1, 200, 448, 7, 49), (2, 129, 512, 8, 64), (1, 140, 576, 9, 81)]
CASES = [(d,) + s for d in DIMS for s in SHAPES] + [(128, 1, 64, 256, 4, 16), (128, 2, 65, 192, 3, 9)]


@pytest.mark.parametrize("d,B,T,dim,h,agent_num", CASES)
def test_agent_head_dim_vs_oracle(device, d, B, T, dim, h, agent_num):
    from amk.models import AgentAttention

    m = AgentAttention(dim, h, d, agent_num=agent_num)
    shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
    w = seeded_params(shapes, 90 + h + d)
    m.load_state_dict(w, strict=True)
    x = seeded((B, T, dim), 91 + T)
    cot = seeded((B, T, dim), 92 + T)
    wr = {n: v.clone().requires_grad_(True) for n, v in w.items()}
    xr = x.clone().requires_grad_(True)
    out_r = ref_cpu.agent_attention(xr, wr, h, d, agent_num)
    names = sorted(wr)
    g_r = torch.autograd.grad((out_r * cot).sum(), [xr] + [wr[n] for n in names], allow_unused=True)

    m = m.to(device)
    xd = x.to(device).requires_grad_(True)
    out = m(xd)
    assert tuple(out.shape) == (B, T, dim)
    assert_close(out, out_r, TOL, "out")
    (out * cot.to(device)).sum().backward()
    assert_close(xd.grad, g_r[0], TOL, "grad x")
    params = dict(m.named_parameters())
    for n, g in zip(names, g_r[1:]):
        if n in ("bias1", "bias2"):
            continue
        _abs_close(params[n].grad, g, TOL, f"grad {n}")


@pytest.mark.parametrize("d", DIMS)
def test_agent_head_dim_full_size_properties(device, d):
    """B 64, T 1024, h 6: one element alone equals it in the batch, forward and backward repeat bitwise, one element
    against the CPU oracle."""
    from amk.models import AgentAttention

    torch.manual_seed(d)
    m = AgentAttention(384, 6, d).to(device)
    x = torch.randn(64, 1024, 384, device=device, requires_grad=True)
    cot = torch.randn(64, 1024, 384, device=device)
    out = m(x)
    (g,) = torch.autograd.grad((out * cot).sum(), [x])
    out2 = m(x)
    (g2,) = torch.autograd.grad((out2 * cot).sum(), [x])
    assert torch.equal(out, out2) and torch.equal(g, g2)
    xs = x[17:18].detach().clone().requires_grad_(True)
    outs = m(xs)
    (gs,) = torch.autograd.grad((outs * cot[17:18]).sum(), [xs])
    assert_close(outs, out[17:18], 1e-6, "element alone vs in batch")
    assert_close(gs, g[17:18], 1e-6, "grad: element alone vs in batch")
    w = {n: p.detach().cpu() for n, p in m.named_parameters()}
    xr = x[17:18].detach().cpu().requires_grad_(True)
    out_r = ref_cpu.agent_attention(xr, w, 6, d, 47)
    (g_r,) = torch.autograd.grad((out_r * cot[17:18].cpu()).sum(), [xr])
    assert_close(out[17:18], out_r, TOL, "vs oracle")
    assert_close(g[17:18], g_r, TOL, "grad vs oracle")


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("d", DIMS)
def test_agent_head_dim_under_bf16_autocast(device, d):
    """bf16 projections around the f32 agent core: runs, and stays within bf16 rounding of the f32 module."""
    from amk.models import AgentAttention

    m = AgentAttention(192, 3, d, agent_num=9)
    m.load_state_dict(seeded_params({n: tuple(p.shape) for n, p in m.named_parameters()}, 95 + d), strict=True)
    m = m.to(device)
    x = seeded((2, 200, 192), 96).to(device)
    cot = seeded((2, 200, 192), 97).to(device)
    x32 = x.clone().requires_grad_(True)
    out32 = m(x32)
    (out32 * cot).sum().backward()
    g32 = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    x16 = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = m(x16)
    (out16.float() * cot).sum().backward()
    assert torch.isfinite(out16).all() and torch.isfinite(x16.grad).all()
    assert _rel(out16, out32) < 2e-2, _rel(out16, out32)
    assert _rel(x16.grad, x32.grad) < 2e-2, _rel(x16.grad, x32.grad)
    for n in ("qkv.weight", "W_o.weight", "dwc.1.weight"):
        p = dict(m.named_parameters())[n]
        assert p.grad is not None and p.grad.dtype == torch.float32
        assert _rel(p.grad, g32[n]) < 3e-2, (n, _rel(p.grad, g32[n]))
