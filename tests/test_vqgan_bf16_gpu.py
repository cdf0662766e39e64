"""amk.models.VQGAN under bf16 autocast on the MI355X, its 70 GroupNorms (+ Swish) on amk_gnact_bf16_*.

The whole model cannot be pinned under bf16: the fixture's smallest top-2 codebook margin is 5e-4, far below bf16 noise on the
encoder's output, so indices legitimately differ.  The two halves around the lookup can (tests/golden/vqgan_small_halves.npz,
the reference's own fp64 run, tools/gen_vqgan_halves_golden.py): pre_quant(encoder(imgs)) and decoder(post_quant(zq)), each
with its input gradient and the gradients of every gn.weight / gn.bias.  There is no derivable tolerance for ~70 bf16 roundings
through vendor convolutions, so the yardstick is the module path under the same autocast (AMK_GN_ACT_BF16 off), measured
against the same fixture in the same run: per tensor, dev = max |got - fp64| / max |fp64| of the fused path may be at most 2
times that of the modules, and the same in rms at most 1.5 times (two realisations of the same roundings: a tensor's max moves
by tens of percent between them, its rms by less; a wrong term in the backward moves a gradient by order 1).  The modules' own
deviation must stay below 0.1 for every tensor, or the yardstick says nothing.

Then the whole model under autocast (event counts, finiteness, dtypes) and one MaskedTokenTrainStep(autocast=bfloat16) of a
small MUSE over the frozen tokenizer.

Measured on the MI355X, deviation from the fp64 fixture in max / in rms, fused against modules:
    enc:out        1.70e-2 / 1.41e-2  against  1.48e-2 / 1.38e-2      enc:grad_imgs  2.40e-2 / 2.52e-2  against  2.39e-2 / 2.52e-2
    dec:out        2.28e-2 / 2.17e-2  against  2.58e-2 / 2.27e-2      dec:grad_zq    2.38e-2 / 2.80e-2  against  2.68e-2 / 2.90e-2
    worst gn gradient, encoder   4.4e-2 / 3.5e-2 (model.2.block.0.gn)  against  5.9e-2 / 3.6e-2
    worst gn gradient, decoder   4.0e-2 / 3.2e-2 (model.11.gn.gn)      against  4.3e-2 / 3.3e-2
    worst ratio fused / modules over the 144 tensors: 1.62 in max (decoder.model.11.gn.gn.weight), 1.21 in rms
    (decoder.model.27.block.3.gn.weight); the modules' worst deviation 5.9e-2, below the 0.1 cap.
"""
import json
import os

import pytest
import torch

import vqgan_halves_ref as halves
import vqgan_ref
from util import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
_STATE = {}


def _seed():
    with open(os.path.join(GOLDEN, "vqgan_small.json")) as f:
        return json.load(f)["seed"]


def _small(device):
    from amk.models import VQGAN

    torch.manual_seed(0)
    model = VQGAN(vqgan_ref.DIM, vqgan_ref.CODES)
    model.load_state_dict(vqgan_ref.recipe_state_dict(model, _seed()), strict=True)
    return model.to(device)


def _halves(device, monkeypatch, fused):
    """{name: CPU tensor} of both halves under bf16 autocast, and the kernel events of the run."""
    from amk import ops

    if fused not in _STATE:
        monkeypatch.setattr(ops, "GN_ACT", True)
        monkeypatch.setattr(ops, "GN_ACT_BF16", fused)
        monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
        inp = {k: v.to(device) for k, v in halves.inputs(_seed()).items()}
        res = halves.run_halves(_small(device), inp, autocast=BF16)
        torch.cuda.synchronize()
        _STATE[fused] = ({k: v.cpu() for k, v in res.items()}, {k: len(v) for k, v in ops.KERNEL_EVENTS.items()})
    return _STATE[fused]


def _devs(res, fx):
    out = {}
    for k, want in fx.items():
        want = torch.from_numpy(want)
        d = res[k].double() - want
        out[k] = (float(d.abs().max() / want.abs().max()), float(d.pow(2).mean().sqrt() / want.pow(2).mean().sqrt()))
    return out


@pytest.mark.parametrize("half", ["enc", "dec"])
def test_halves_against_the_fp64_fixture(device, monkeypatch, half):
    fx = {k: v for k, v in load_golden("vqgan_small_halves").items() if k.startswith(half + ":")}
    assert len(fx) == 2 + 2 * (28 if half == "enc" else 42)
    (on, ev_on), (off, ev_off) = _halves(device, monkeypatch, True), _halves(device, monkeypatch, False)
    assert ev_on.get("gnact_bf16_fwd") == 70 and ev_on.get("gnact_bf16_bwd") == 70
    assert not any(k.startswith("gnact") for k in ev_off)
    assert on[half + ":out"].dtype == BF16
    d_on, d_off = _devs(on, fx), _devs(off, fx)
    for k in sorted(fx):
        print(f"{k}: fused max {d_on[k][0]:.3e} rms {d_on[k][1]:.3e} | modules max {d_off[k][0]:.3e} rms {d_off[k][1]:.3e}")
    worst = lambda d, i: max((v[i], k) for k, v in d.items())  # noqa: E731
    print(f"{half} worst: fused max {worst(d_on, 0)} rms {worst(d_on, 1)} | modules max {worst(d_off, 0)} rms {worst(d_off, 1)}")
    for k in sorted(fx):
        assert bool(torch.isfinite(on[k]).all()), k
        assert d_off[k][0] < 0.1, f"{k}: the module path itself is {d_off[k][0]:.3e} from the fp64 fixture"
        assert d_on[k][0] <= 2 * d_off[k][0], f"{k}: max deviation {d_on[k][0]:.3e} fused against {d_off[k][0]:.3e} modules"
        assert d_on[k][1] <= 1.5 * d_off[k][1], f"{k}: rms deviation {d_on[k][1]:.3e} fused against {d_off[k][1]:.3e} modules"


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "switch_off"])
def test_whole_model_under_autocast(device, monkeypatch, fused):
    """Forward + backward + encode_imgs: all 70 norms (and the encoder's 28 again) on the bf16 kernels, none on the f32 ones;
    with the switch off no gnact_* call at all."""
    from amk import ops

    monkeypatch.setattr(ops, "GN_ACT", True)
    monkeypatch.setattr(ops, "GN_ACT_BF16", fused)
    monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
    model = _small(device)
    imgs, cot = vqgan_ref.inputs(_seed())
    imgs = imgs.to(device).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF16):
        out, loss = model(imgs)
    ((out.float() * cot.to(device)).sum() + loss.float()).backward()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        idx = model.encode_imgs(imgs.detach())
    torch.cuda.synchronize()
    ev = {k: len(v) for k, v in ops.KERNEL_EVENTS.items() if k.startswith("gnact")}
    if fused:
        assert ev == {"gnact_bf16_fwd": 70 + 28, "gnact_bf16_bwd": 70}
    else:
        assert ev == {}
    assert out.dtype == BF16 and bool(torch.isfinite(out).all()) and bool(torch.isfinite(loss).all())
    assert idx.shape == (2, 16) and 0 <= int(idx.min()) and int(idx.max()) < vqgan_ref.CODES
    assert bool(torch.isfinite(imgs.grad).all())
    for n, p in model.named_parameters():
        if ".proj_out." in n:
            assert p.grad is None, n
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


def test_muse_trains_under_autocast_over_the_frozen_conv_tokenizer(device, monkeypatch):
    from amk import ops
    from amk.models import MUSE, VQGAN
    from amk.train import MaskedTokenTrainStep

    monkeypatch.setattr(ops, "GN_ACT", True)
    monkeypatch.setattr(ops, "GN_ACT_BF16", True)
    torch.manual_seed(0)
    vq = VQGAN(32, 512).to(device)
    model = MUSE(dim=64, vq=vq, text_dim=24, n_heads=1, d_head=64, depth=1, mult=2).to(device)
    vq0 = {n: p.detach().clone() for n, p in vq.named_parameters()}
    dec0 = {n: p.detach().clone() for n, p in model.decoder.named_parameters()}
    ts = MaskedTokenTrainStep(model, lr=1e-3, schedule="constant", bucket_bytes=128 << 10, autocast=BF16)
    monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
    loss = ts.step(torch.randn(1, 5, 24, device=device), torch.rand(1, 3, 256, 256, device=device))
    torch.cuda.synchronize()
    ev = {k: len(v) for k, v in ops.KERNEL_EVENTS.items() if k.startswith("gnact")}
    assert ev == {"gnact_bf16_fwd": 28}, ev             # the frozen tokenizer's encoder, forward only, nothing saved
    assert bool(torch.isfinite(torch.as_tensor(loss)).all())
    assert any(not torch.equal(p, dec0[n]) for n, p in model.decoder.named_parameters())
    for n, p in vq.named_parameters():
        assert not p.requires_grad and p.grad is None and torch.equal(p, vq0[n]), n
