"""SoftmaxAttention at head dims 96, 160, 192, 224 and 256 on the GPU: the attention core against the oracle (layouts,
ragged sizes, masks, a dead row), the module against the reference-pinned fixtures (tools/gen_attention_golden_dh.py),
SwitchHeadAttention and ViT at dim_head 96, reproducibility, bf16 autocast, and which kernels run."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu
from oracle.fixture_recipe import seeded, seeded_params
from util import assert_close, load_golden, weights_of

pytestmark = pytest.mark.gpu

TOL = 2e-5   # test_module_other_head_dims' tolerance
NEW_DIMS = [96, 160, 192, 224, 256]

# (B, H, I, J, mask): ragged sizes around the 32-row tiles and the 128-row workgroups, I != J, T = 1024
CASES = [
    (1, 2, 1, 31, None),
    (2, 1, 31, 65, "key"),
    (1, 2, 65, 300, None),
    (2, 2, 300, 65, "key"),
    (1, 1, 300, 1, None),
    (1, 2, 65, 65, "causal"),
    (1, 1, 300, 300, "dead"),
    (1, 1, 1024, 1024, None),
]


def _masks(B, I, J, kind):
    key, causal = None, None
    if kind == "key":
        key = torch.ones(B, J, dtype=torch.bool)
        key[0, J // 2:] = False
        key[-1, :1] = False
    elif kind in ("causal", "dead"):
        causal = torch.ones(I, J).triu(1).bool()
        if kind == "dead":
            causal[5, :] = True   # one fully masked query row: a uniform softmax over all keys
    return key, causal


@pytest.mark.parametrize("layout", ["bhtd", "bthd"])
@pytest.mark.parametrize("B,H,I,J,mask", CASES)
@pytest.mark.parametrize("D", NEW_DIMS)
def test_core_vs_oracle(device, D, B, H, I, J, mask, layout):
    from amk import ops

    seed = D + I + J
    q = seeded((B, H, I, D), seed + 1)
    k = seeded((B, H, J, D), seed + 2)
    v = seeded((B, H, J, D), seed + 3)
    cot = seeded((B, H, I, D), seed + 4)
    key, causal = _masks(B, I, J, mask)
    scale = D ** -0.5
    qc, kc, vc = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref = ref_cpu.attention_core(qc, kc, vc, scale, key, causal)
    g_ref = torch.autograd.grad((o_ref * cot).sum(), [qc, kc, vc])

    def to_dev(t):
        t = t.to(device)
        if layout == "bthd":  # (B,T,H,D) storage viewed as (B,H,T,D): the projection layout
            t = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        return t.requires_grad_(True)

    qd, kd, vd = to_dev(q), to_dev(k), to_dev(v)
    o = ops.attention(qd, kd, vd, scale, key_mask=None if key is None else key.to(device),
                      causal_mask=None if causal is None else causal.to(device))
    g = torch.autograd.grad((o * cot.to(device)).sum(), [qd, kd, vd])
    assert_close(o, o_ref, TOL, "o")
    # one key: P = 1, so dq = dk = 0 in exact arithmetic and both sides hold only the rounding residue of dP - delta
    # (two f32 dot products of length D) times k or q and the scale: held to 4 ulps of the largest such term
    for name, a, b in zip(("dq", "dk", "dv"), g, g_ref):
        if J == 1 and name != "dv":
            noise = 4 * 2.0 ** -23 * float((cot.abs() * v.abs()).sum(-1).max()) * max(float(k.abs().max()), float(q.abs().max())) * scale
            assert float(a.abs().max()) <= noise and float(b.abs().max()) <= noise, (name, noise)
            continue
        assert_close(a, b, TOL, name)


@pytest.mark.parametrize("variant", ["self", "cross_ctxmask", "self_causal"])
@pytest.mark.parametrize("D", [96, 192, 256])
def test_module_vs_reference_fixture(device, D, variant):
    from amk.models import SoftmaxAttention

    fx = load_golden(f"softmax_attention_d{D}")
    dim, h, d = (int(v) for v in fx["dims"])
    m = SoftmaxAttention(dim, num_heads=h, dim_head=d)
    m.load_state_dict(weights_of(fx), strict=True)
    m = m.to(device)
    x = torch.from_numpy(fx["x"]).to(device).requires_grad_(True)
    ctx = torch.from_numpy(fx["context"]).to(device).requires_grad_(True)
    kw = {"self": dict(),
          "cross_ctxmask": dict(context=ctx, context_mask=torch.from_numpy(fx["ctxmask"]).to(device)),
          "self_causal": dict(causal_mask=torch.from_numpy(fx["causal"]).to(device))}[variant]
    out = m(x, **kw)
    assert_close(out, fx[f"{variant}:out"], TOL, "out")
    (out * torch.from_numpy(fx["cot"]).to(device)).sum().backward()
    assert_close(x.grad, fx[f"{variant}:gx"], TOL, "grad x")
    if "context" in kw:
        assert_close(ctx.grad, fx[f"{variant}:gctx"], TOL, "grad context")
    for n, p in m.named_parameters():
        key = f"{variant}:g:{n}"
        if key in fx:
            assert_close(p.grad, fx[key], TOL, f"grad {n}")


def test_switchhead_dim_head_96(device):
    """SwitchHeadAttention(dim_head=96), self-attention, against the oracle: routing, output and gradients."""
    from amk.models import SwitchHeadAttention

    B, T, dim, h, E, k, d = 2, 65, 512, 4, 5, 2, 96
    shapes = {"q.0.weight": (h * d, dim), "k.0.weight": (h * d, dim), "W_s.0.weight": (h * E, dim), "W_d.0.weight": (h * E, dim)}
    for e in range(E):
        shapes[f"experts_v.{e}.weight"] = (d, dim)
        shapes[f"experts_out.{e}.weight"] = (dim, d)
    w = seeded_params(shapes, 96)
    x = seeded((B, T, dim), 97)
    cot = seeded((B, T, dim), 98)
    wr = {n: t.clone().requires_grad_(True) for n, t in w.items()}
    xr = x.clone().requires_grad_(True)
    out_r, sel_v, sel_o = ref_cpu.switchhead_attention(xr, wr, h, d, E, k)
    (gx_r,) = torch.autograd.grad((out_r * cot).sum(), [xr])

    m = SwitchHeadAttention(dim, h, d, num_experts=E, sel_experts=k)
    m.load_state_dict(w, strict=True)
    m = m.to(device)
    xd = x.to(device).requires_grad_(True)
    out = m(xd)
    assert torch.equal(m.last_selected_v.cpu(), sel_v)
    assert torch.equal(m.last_selected_out.cpu(), sel_o)
    assert_close(out, out_r, TOL, "out")
    (out * cot.to(device)).sum().backward()
    assert_close(xd.grad, gx_r, TOL, "grad x")


def test_vit_dim_head_96(device):
    """A small ViT with d_head = 96: logits and parameter gradients against the oracle's ViT forward."""
    from amk.models import ViT

    torch.manual_seed(0)
    m = ViT(dim=64, image_size=32, patch_size=8, n_heads=2, d_head=96, depth=2, mlp_dim=128, dropout=0.0, num_classes=10)
    w = {n: t.detach().clone().requires_grad_(t.dtype.is_floating_point) for n, t in m.state_dict().items()}
    imgs = seeded((2, 3, 32, 32), 99)
    labels = torch.tensor([3, 7])
    logits_r = ref_cpu.vit_forward(imgs, w, 8, 2, 96, 2)
    loss_r = torch.nn.functional.cross_entropy(logits_r, labels)
    names = [n for n in sorted(w) if w[n].requires_grad]
    g_r = torch.autograd.grad(loss_r, [w[n] for n in names], allow_unused=True)

    m = m.to(device)
    logits = m(imgs.to(device))
    assert_close(logits, logits_r, 5e-5, "logits")
    torch.nn.functional.cross_entropy(logits, labels.to(device)).backward()
    params = dict(m.named_parameters())
    checked = 0
    for n, gr in zip(names, g_r):
        if gr is None or n not in params or gr.numel() == 0:   # (the zero-width FFN of the dropout-as-mult quirk)
            continue
        g = params[n].grad
        assert g is not None, n
        err = float((g.detach().cpu().double() - gr.double()).abs().max())
        assert err <= 2e-4 * max(float(gr.abs().max()), 1e-3), f"grad {n}: abs err {err:.3e}"
        checked += 1
    assert checked >= 10, checked


@pytest.mark.parametrize("D", NEW_DIMS)
def test_backward_bitwise_reproducible(device, D):
    from amk import ops

    B, H, I, J = 2, 2, 200, 333
    mk = lambda seed, T: seeded((B, T, H, D), seed).to(device).permute(0, 2, 1, 3)
    cot = seeded((B, H, I, D), 5).to(device)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            q, k, v = (t.requires_grad_(True) for t in (mk(1, I), mk(2, J), mk(3, J)))
            o = ops.attention(q, k, v, D ** -0.5)
            runs.append(torch.autograd.grad((o * cot).sum(), [q, k, v]))
    finally:
        torch.use_deterministic_algorithms(prev)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_autocast_dim_head_96(device):
    """Under bf16 autocast a D = 96 module runs the f32 kernels on upcast inputs (no bf16 attention kernel)."""
    from amk import ops
    from amk.models import SoftmaxAttention

    torch.manual_seed(0)
    m = SoftmaxAttention(192, num_heads=2, dim_head=96).to(device)
    x = seeded((2, 77, 192), 11).to(device)
    ctx = seeded((2, 50, 192), 12).to(device)
    km = torch.ones(2, 50, dtype=torch.bool, device=device)
    km[1, 30:] = False
    out32 = m(x, context=ctx, context_mask=km)
    ops.KERNEL_EVENTS = {}
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out16 = m(x, context=ctx, context_mask=km)
        out16.float().sum().backward()
        torch.cuda.synchronize()
        names = set(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    assert not any(n.startswith("attn_bf16") for n in names), names
    assert any(n.startswith("attn_fwd") for n in names), names
    err = float((out16.detach().float() - out32.detach()).abs().max() / out32.detach().abs().max())
    assert err < 2e-2, err


@pytest.mark.parametrize("D", NEW_DIMS + [64])
def test_launches_generic_kernels(device, D, monkeypatch):
    """The forward and backward run the head-dim kernels themselves, not a padded D = 128 / 256 path.  Head dim 64 has
    its own forward and one-pass backward; its reproducible two-kernel backward is the D = 64 instantiation of the same
    recompute kernels, and no hand-written copy of them runs."""
    from torch.profiler import ProfilerActivity, profile

    from amk import ops

    kernels = ["attn_bwd_delta_gen_kernel", "attn_bwd_dkdv_gen_kernel", "attn_bwd_dq_gen_kernel"]
    if D == 64:
        monkeypatch.setattr(ops, "ATTENTION_BACKWARD_TWO_KERNEL", True)
    else:
        kernels.append("attn_fwd_gen_plain_kernel")
    q, k, v = (seeded((1, 2, 100, D), s).to(device).requires_grad_(True) for s in (1, 2, 3))
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        o = ops.attention(q, k, v, D ** -0.5)
        o.sum().backward()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    tag = f"<{D},"
    for kernel in kernels:
        hits = [n for n in names if kernel in n]
        assert hits, (kernel, sorted(set(names))[:40])
        assert all(tag in n or f"<{D}>" in n or f"ILi{D}E" in n for n in hits), hits
    assert not any("attn_bf16" in n for n in names)
    for old in ("attn_bwd_delta_kernel", "attn_bwd_dkdv_kernel", "attn_bwd_dq_kernel"):
        assert not any(old in n for n in names), (old, [n for n in names if old in n])
