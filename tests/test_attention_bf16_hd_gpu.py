"""SoftmaxAttention at head dims 32 and 128 under torch.autocast(bfloat16) with the head dim enabled in
ops.ATTENTION_BF16_DIMS: the core runs on csrc/attn_bf16_hd.hip.

Checker: fixtures generated from the reference's SoftmaxAttention under torch.autocast("cpu", dtype=bfloat16)
(tests/golden/softmax_attention_bf16_d{32,128}.npz, tools/gen_attention_bf16_golden_dh.py), stored next to the same
module's f32 results and the reference's own autocast-vs-f32 deviation (`<variant>:err`).  The bar is the D = 64 module
test's (tests/test_attention_bf16_gpu.py): within 2e-2 (max-norm relative) of the autocast fixture, and no further from
the f32 fixture than 1.5x what the reference's own autocast is."""
import pytest
import torch

from util import load_golden, rel_err, weights_of

pytestmark = pytest.mark.gpu
HD_KERNELS = ("attn_bf16_hd_fwd_kernel", "attn_bf16_hd_bwd_kernel")


@pytest.fixture(autouse=True)
def _dims(monkeypatch):
    from amk import ops

    monkeypatch.setattr(ops, "ATTENTION_BF16_DIMS", frozenset((32, 64, 128)))


@pytest.mark.parametrize("d_head", [32, 128])
@pytest.mark.parametrize("variant", ["self", "cross_ctxmask", "self_causal"])
def test_module_under_autocast_matches_reference_autocast(device, variant, d_head):
    from amk import ops
    from amk.models import SoftmaxAttention

    fx = load_golden(f"softmax_attention_bf16_d{d_head}")
    err_out, err_gx, err_gctx, err_gparams = (float(e) for e in fx[f"{variant}:err"])
    dim, h, d = (int(v) for v in fx["dims"])
    assert d == d_head
    m = SoftmaxAttention(dim, h, d).to(device)
    m.load_state_dict({k: v.to(device) for k, v in weights_of(fx).items()}, strict=True)
    x = torch.from_numpy(fx["x"]).to(device).requires_grad_(True)
    kw = {}
    wrt = [x]
    if variant == "cross_ctxmask":
        kw["context"] = torch.from_numpy(fx["context"]).to(device).requires_grad_(True)
        kw["context_mask"] = torch.from_numpy(fx["ctxmask"]).to(device)
        wrt.append(kw["context"])
    if variant == "self_causal":
        kw["causal_mask"] = torch.from_numpy(fx["causal"]).to(device)
    ops.KERNEL_EVENTS = {}
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(x, **kw)
        gs = torch.autograd.grad((out.float() * torch.from_numpy(fx["cot"]).to(device)).sum(), wrt + [p for _, p in sorted(m.named_parameters())])
        torch.cuda.synchronize()
        names = {n for n in ops.KERNEL_EVENTS if n.startswith("attn")}
    finally:
        ops.KERNEL_EVENTS = None
    sfx = "<masked>" if variant != "self" else ""
    assert names == {n + sfx for n in HD_KERNELS}, names
    g = lambda key: torch.from_numpy(fx[key])
    assert rel_err(out.float(), g(f"{variant}:out")) < 2e-2
    assert rel_err(out.float(), g(f"{variant}:out_f32")) < 1.5 * err_out
    assert rel_err(gs[0], g(f"{variant}:gx")) < 2e-2
    assert rel_err(gs[0], g(f"{variant}:gx_f32")) < 1.5 * err_gx
    off = 1
    if "context" in kw:
        assert rel_err(gs[1], g(f"{variant}:gctx")) < 2e-2
        assert rel_err(gs[1], g(f"{variant}:gctx_f32")) < 1.5 * err_gctx
        off = 2
    if variant == "self":      # (the fixture keeps parameter gradients for the two masked variants)
        return
    for (n, _), grad in zip(sorted(m.named_parameters()), gs[off:]):
        assert rel_err(grad, g(f"{variant}:g:{n}")) < 2e-2, n
        assert rel_err(grad, g(f"{variant}:g32:{n}")) < 1.5 * err_gparams, n


def test_decoder_layer_d_head_128_runs_on_the_hd_kernels(device):
    """One transformer.Decoder layer at d_head 128 with a causal and a context mask, forward + backward under autocast:
    both attentions launch only attn_bf16_hd_* attention kernels, and every gradient is finite."""
    from amk import ops
    from amk.models import transformer

    torch.manual_seed(0)
    B, T, S, dim = 2, 40, 70, 64
    dec = transformer.Decoder(dim, n_heads=2, d_head=128, depth=1).to(device)
    x = torch.randn(B, T, dim, device=device, requires_grad=True)
    ctx = torch.randn(B, S, dim, device=device, requires_grad=True)
    ctx_mask = torch.ones(B, S, dtype=torch.bool, device=device)
    ctx_mask[0, -9:] = False
    ops.KERNEL_EVENTS = {}
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = dec(x, ctx, context_mask=ctx_mask, causal_mask=ops.causal_mask(T, T, device))
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        names = {n for n in ops.KERNEL_EVENTS if n.startswith("attn")}
    finally:
        ops.KERNEL_EVENTS = None
    assert names == {n + "<masked>" for n in HD_KERNELS}, names
    assert out.shape == (B, T, dim) and bool(torch.isfinite(out.float()).all())
    for n, t in [("x", x), ("context", ctx)] + list(dec.named_parameters()):
        assert t.grad is not None and bool(torch.isfinite(t.grad.float()).all()), n
