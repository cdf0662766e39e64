"""Parti's training loss through the fused logits + bias + cross-entropy head (Parti.loss_from_hidden,
ops.linear_cross_entropy(..., bias=to_logits.bias)): the switch changes the path and not the step, the fused arm meets the
reference's fixture at tests/test_parti_gpu.py's own tolerances, bf16 autocast takes the bf16 head, and generate is
untouched."""
import pytest
import torch

from test_parti_golden import fixture
from test_parti_gpu import TOL_OUT, StubVQ, _check_grads, _load
from util import assert_close

pytestmark = pytest.mark.gpu


def _abs_close(a, b, tol, what):
    """The margin of the Muse switch test (tests/test_ce_head_gpu.py): tol x the largest element."""
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    scale = max(float(b.abs().max()), 1e-4)
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"{what}: abs err {err:.3e} (scale {scale:.3e})"


def _model(device, name="parti_small"):
    from amk.models import Parti

    fx = fixture(name)
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    m = _load(Parti(dim, StubVQ(V, T, torch.from_numpy(fx["ids"])), None, None, 77, h, d, depth), fx, device)
    return m, fx, torch.from_numpy(fx["text"]).to(device), torch.zeros(B, 3, 8, 8, device=device)


def _step(m, text, imgs, on, monkeypatch, autocast=False):
    from amk import ops

    monkeypatch.setattr(ops, "CE_HEAD", on)
    m.zero_grad(set_to_none=True)
    ops.KERNEL_EVENTS = {}
    try:
        if autocast:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = m(text, imgs)
        else:
            loss = m(text, imgs)
        loss.float().backward()
        torch.cuda.synchronize()
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    return loss.detach().float(), grads, [n for n in names if "ce_head" in n]


def test_switch_changes_the_path_not_the_step(device, monkeypatch):
    m, fx, text, imgs = _model(device)
    loss0, g0, k0 = _step(m, text, imgs, False, monkeypatch)
    loss1, g1, k1 = _step(m, text, imgs, True, monkeypatch)
    assert not k0
    assert sorted(n.split()[0] for n in k1) == ["ce_head_bias_bwd", "ce_head_bias_fwd"], k1
    assert_close(loss1, loss0, 5e-5, "loss")
    assert set(g0) == set(g1) and len(g0) > 10 and "to_logits.bias" in g1
    for n in g0:
        _abs_close(g1[n], g0[n].cpu(), 3e-4, f"grad {n}")
    # the fused arm against the reference's own numbers, at the tolerances of tests/test_parti_gpu.py
    assert_close(loss1, fx["loss"], TOL_OUT, "loss")
    _check_grads(m, fx)


def test_bf16_autocast_takes_the_bf16_head(device, monkeypatch):
    m, fx, text, imgs = _model(device)
    loss, grads, k = _step(m, text, imgs, True, monkeypatch, autocast=True)
    assert sorted(n.split()[0] for n in k) == ["bf16_ce_head_bias_bwd", "bf16_ce_head_bias_fwd"], k
    assert bool(torch.isfinite(loss)) and grads["to_logits.bias"].dtype == torch.float32
    # (a sanity margin, not a bound: bf16 operands carry 2^-8 relative roundings through the decoder's layers, so the
    # loss moves in its third digit; the head's own error is held element-wise in tests/test_ce_head_bias_bf16_gpu.py)
    assert abs(float(loss) - float(fx["loss"].item())) < 0.05 * abs(float(fx["loss"].item()))
    _, _, k0 = _step(m, text, imgs, False, monkeypatch, autocast=True)
    assert not k0


def test_generate_is_untouched(device):
    from amk import ops
    from amk.models import Parti

    fx = fixture("parti_generate_small")
    dim, h, d, depth, V, L, T, B = (int(v) for v in fx["dims"])
    m = _load(Parti(dim, StubVQ(V, T), None, None, 77, h, d, depth), fx, device)
    ops.KERNEL_EVENTS = {}
    try:
        ids = m.generate(torch.from_numpy(fx["text"]).to(device), gumbel=torch.from_numpy(fx["gumbel"]).to(device))
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    assert torch.equal(ids.cpu(), torch.from_numpy(fx["ids"]))
    assert not any("ce_head" in n for n in names)
