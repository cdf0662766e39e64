"""amk.models.VQGAN on the MI355X: the reference's state_dict loads strictly; forward + backward agree with the reference's own
fp64 run (tests/golden/vqgan_small.npz, written by tools/gen_vqgan_golden.py with the weights of tests/vqgan_ref.py) with the
fused GroupNorm + Swish kernels on and off; the README's contract at 256 px; the factory; and one Muse train step over the
frozen conv tokenizer.

Tolerance: the suite's model tolerance, 2e-5 (max |got - want| / max |want|, plus util.assert_close's element-wise check).
It rests on vendor convolutions, so the module path alone (switch off) was measured against the fp64 fixture on the MI355X:
4.5e-6 at worst (the gradient of encoder.model.15.block.0.gn.weight; out 1.8e-6, input gradient 2.6e-6, loss 1.5e-7), against
5.3e-6 for the reference's own f32 CPU run (tests/golden/vqgan_small.json).  That is below 1e-5, so 2e-5 stands."""
import json
import os
import types

import pytest
import torch

import vqgan_ref
from util import GOLDEN, assert_close, load_golden, rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
_STATE = {}


def _meta():
    with open(os.path.join(GOLDEN, "vqgan_small.json")) as f:
        return json.load(f)


def _small(device):
    from amk.models import VQGAN

    torch.manual_seed(0)
    model = VQGAN(vqgan_ref.DIM, vqgan_ref.CODES)
    sd = vqgan_ref.recipe_state_dict(model, _meta()["seed"])
    model.load_state_dict(sd, strict=True)
    return model.to(device), sd


def _run(device, monkeypatch, fused):
    """{name: tensor} of one forward + backward of the small model, as the fixture's tool runs the reference."""
    from amk import ops

    key = bool(fused)
    if key in _STATE:
        return _STATE[key]
    monkeypatch.setattr(ops, "GN_ACT", fused)
    monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
    model, _ = _small(device)
    imgs, cot = vqgan_ref.inputs(_meta()["seed"])
    imgs = imgs.to(device).requires_grad_(True)
    out, loss = model(imgs)
    ((out * cot.to(device)).sum() + loss).backward()
    idx = model.encode_imgs(imgs.detach())
    torch.cuda.synchronize()
    res = {"out": out.detach(), "loss": loss.detach(), "indices": idx.reshape(-1), "grad_imgs": imgs.grad}
    params = dict(model.named_parameters())
    for n in vqgan_ref.stored_grad_names(model):
        res["grad:" + n] = params[n].grad
    res["proj_out_grads"] = [p.grad for n, p in params.items() if ".proj_out." in n]
    res["events"] = {k: len(v) for k, v in ops.KERNEL_EVENTS.items()}
    _STATE[key] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in res.items()}
    return _STATE[key]


def test_reference_state_dict_loads_strictly(device):
    model, sd = _small(device)
    keys = set(model.state_dict())
    assert keys == set(sd)
    assert {"encoder.model.1.block.0.gn.weight", "encoder.model.14.q.weight", "decoder.model.0.weight",
            "encoder.model.14.proj_out.bias", "codebook.embedding.weight", "pre_quant.weight", "post_quant.bias"} <= keys
    assert sum(1 for n in keys if n.endswith("gn.weight")) == 70
    assert model.num_patches == 256 and model.codebook.codebook_size == vqgan_ref.CODES


def _against_fixture(res, tag):
    fx = load_golden("vqgan_small")
    assert set(fx) == {k for k in res if k not in ("proj_out_grads", "events")}
    assert torch.equal(res["indices"], torch.from_numpy(fx["indices"])), f"{tag}: indices"
    worst = {}
    for k, want in fx.items():
        if k == "indices":
            continue
        want = torch.from_numpy(want)
        worst[k] = float((res[k].double() - want).abs().max() / want.abs().max())
    print(tag, "worst deviation", max(worst.values()), "at", max(worst, key=worst.get), "| out", worst["out"], "grad_imgs",
          worst["grad_imgs"], "loss", worst["loss"])
    for k, want in fx.items():
        if k != "indices":
            assert_close(res[k], torch.from_numpy(want), TOL, f"{tag}: {k}")
    assert res["proj_out_grads"] and all(g is None for g in res["proj_out_grads"])
    return worst


def test_golden_with_the_fused_kernels(device, monkeypatch):
    res = _run(device, monkeypatch, True)
    # 70 GroupNorms per forward, all fused; the second forward (encode_imgs) runs the encoder's 28 again
    assert res["events"].get("gnact_fwd") == 70 + 28 and res["events"].get("gnact_bwd") == 70
    _against_fixture(res, "fused")


def test_golden_with_the_switch_off(device, monkeypatch):
    res = _run(device, monkeypatch, False)
    assert "gnact_fwd" not in res["events"] and "gnact_bwd" not in res["events"]
    _against_fixture(res, "modules")


def test_switch_on_against_off(device, monkeypatch):
    on, off = _run(device, monkeypatch, True), _run(device, monkeypatch, False)
    assert torch.equal(on["indices"], off["indices"])
    for k in on:
        if k.startswith("grad") or k in ("out", "loss"):        # each is within TOL of the fixture
            assert rel_err(on[k], off[k]) <= 2 * TOL, f"on against off: {k}"


def test_readme_contract_at_256px(device):
    from amk.models import VQGAN

    torch.manual_seed(0)
    model = VQGAN(256, 8192).to(device).eval()
    imgs = torch.rand(1, 3, 256, 256, device=device)
    with torch.no_grad():
        out, loss = model(imgs)
        idx = model.encode_imgs(imgs)
        dec = model.decode_indices(idx)
    assert out.shape == (1, 3, 256, 256) and loss.dim() == 0 and bool(torch.isfinite(out).all())
    assert idx.shape == (1, 256) and idx.dtype == torch.int64 and 0 <= int(idx.min()) and int(idx.max()) < 8192
    assert dec.shape == (1, 3, 256, 256) and bool(torch.isfinite(dec).all())


def test_factory_builds_the_vqgan():
    from amk.models import VQGAN, build_model
    from models import VQGAN as alias

    cfg = types.SimpleNamespace(model=types.SimpleNamespace(name="vqgan"),
                                codebook=types.SimpleNamespace(codebook_dim=32, codebook_size=64))
    m = build_model(cfg)
    assert isinstance(m, VQGAN) and alias is VQGAN
    assert m.codebook.codebook_dim == 32 and m.codebook.codebook_size == 64 and m.pre_quant.weight.shape == (32, 32, 1, 1)
    with pytest.raises(NotImplementedError, match="vqgan"):
        build_model(types.SimpleNamespace(model=types.SimpleNamespace(name="muse")))


def test_muse_trains_over_the_frozen_conv_tokenizer(device):
    from amk.models import MUSE, VQGAN
    from amk.train import MaskedTokenTrainStep

    torch.manual_seed(0)
    vq = VQGAN(32, 512).to(device)
    model = MUSE(dim=64, vq=vq, text_dim=24, n_heads=1, d_head=64, depth=1, mult=2).to(device)
    vq0 = {n: p.detach().clone() for n, p in vq.named_parameters()}
    dec0 = {n: p.detach().clone() for n, p in model.decoder.named_parameters()}
    ts = MaskedTokenTrainStep(model, lr=1e-3, schedule="constant", bucket_bytes=128 << 10)   # no warm-up: step 0 moves
    loss = ts.step(torch.randn(1, 5, 24, device=device), torch.rand(1, 3, 256, 256, device=device))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.as_tensor(loss)).all())
    assert any(not torch.equal(p, dec0[n]) for n, p in model.decoder.named_parameters())
    for n, p in vq.named_parameters():
        assert not p.requires_grad and p.grad is None and torch.equal(p, vq0[n]), n
