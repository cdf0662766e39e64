"""The split-bf16 plane shadow of FlatAdam (amk/optim.py: enable_planes) under VQGANTrainStep on a two-layer ViT-VQGAN
of dim 32: the planes follow every optimizer step bit for bit, a weight written in place takes the f32 path until
refresh_shadow(), captured steps equal eager ones to the bit, switching to bf16 autocast and back leaves nothing stale,
and a step on the planes agrees with the same step off them at the tolerance tests/test_train_step_gpu.py holds against
the oracle.

The in-place write is ``p.copy_`` under no_grad (what load_state_dict does): it bumps ``p._version``, which is how a stale
plane set is noticed.  ``p.data.copy_`` goes through a detached alias with a version counter of its own and leaves
``p._version`` alone -- torch offers nothing to notice it by, for the planes as for the bf16 copies before them; such code
has to call refresh_shadow() (the docstring of FlatAdam says so)."""
import copy

import pytest
import torch

import gemm_x6_ref as ref
from util import assert_close

pytestmark = pytest.mark.gpu

CFG = dict(dim=32, img_size=32, patch_size=4, n_heads=2, d_head=64, depth=2, mlp_dim=96, dropout=0.0)


def _nets(device):
    from amk.models import ViTVQGAN
    from amk.models.discriminator import NLayerDiscriminator

    torch.manual_seed(0)
    gen = ViTVQGAN(CFG, dict(codebook_size=256, codebook_dim=32)).to(device)
    dis = NLayerDiscriminator(3, 8, 2).to(device)
    g = torch.Generator().manual_seed(3)
    return gen, dis, torch.rand(4, 3, 32, 32, generator=g).to(device), torch.rand(4, 1, 1, 1, generator=g).to(device)


@pytest.fixture
def reproducible():
    from amk import ops

    old, old_conv = ops.DETERMINISTIC_ATTENTION_BACKWARD, torch.backends.cudnn.deterministic
    old_mode, ops.GEMM_MODE, ops.X6_LINEAR = (ops.GEMM_MODE, ops.X6_LINEAR, ops.X6_AUTO_FORMS), "auto", True
    ops.X6_AUTO_FORMS = frozenset(("fwd", "dx"))   # every form: the input gradients on the planes of W^T as well
    ops.DETERMINISTIC_ATTENTION_BACKWARD = True    # (AMK_DETERMINISTIC=1)
    # the discriminator's convolutions too: MIOpen's default weight-gradient kernels add with atomics, and two eager runs
    # of this step then differ in the last bits with the planes on or off (measured: d_loss by 5e-7, parameters by 1e-7)
    torch.backends.cudnn.deterministic = True
    yield ops
    ops.DETERMINISTIC_ATTENTION_BACKWARD, torch.backends.cudnn.deterministic = old, old_conv
    ops.GEMM_MODE, ops.X6_LINEAR, ops.X6_AUTO_FORMS = old_mode


def _with_planes(model):
    return [(n, p) for n, p in model.named_parameters() if hasattr(p, "_amk_x6")]


def _assert_planes_current(model):
    """Every kept plane set equals a fresh amk_gemm_x6_split of the weight as it is now (and of its transpose)."""
    found = _with_planes(model)
    assert len(found) >= 10, [n for n, _ in found]
    for n, p in found:
        pl, w = p._amk_x6, p.detach()
        R, K = w.shape
        assert p._amk_x6_version == p._version, n
        want = ref.split_planes_gpu(w.contiguous()).view(torch.int16)
        got = pl.w.view(3, -1, ref.pad32(K))
        if pl.gate:
            got = got[:, ref.gate_order(w)[1].to(w.device)]
        assert torch.equal(got.view(torch.int16), want), f"planes of {n}"
        want_t = ref.split_planes_gpu(w.t().contiguous()).view(torch.int16)
        assert torch.equal(pl.wt.view(3, K, ref.pad32(R)).view(torch.int16), want_t), f"transposed planes of {n}"
    return found


def test_planes_follow_the_step_and_in_place_writes_fall_back(device, reproducible):
    ops = reproducible
    from amk.models.vitvqgan import SwiGLU
    from amk.train import VQGANTrainStep

    gen, dis, imgs, eta = _nets(device)
    tr = VQGANTrainStep(gen, dis, lr=1e-3, warmup_steps=0, decay_steps=1000)
    found = _assert_planes_current(gen)
    assert sum(p._amk_x6.gate for _, p in found) == 2 * CFG["depth"]          # the w12 of every block, encoder + decoder
    assert tr.g_optim.planes_bytes >= sum(12 * p.numel() for _, p in found)
    before = [p.detach().clone() for _, p in found]
    tr.step(imgs, eta=eta)
    assert sum(not torch.equal(a, p.detach()) for a, (_, p) in zip(before, found)) >= 10   # the step moved the weights
    _assert_planes_current(gen)
    # ---- one FFN, its w3 written behind the optimizer's back
    ffn = next(m for m in gen.modules() if isinstance(m, SwiGLU))
    w12, w3 = ffn.w12.weight, ffn.w3.weight
    x = torch.randn(4, 64, w12.shape[1], device=device)
    with torch.no_grad():
        assert ops._x6_planes("ffn", x, w12, w3, gate=w12) is not None
        on = ffn(x)
        w3.copy_(w3 * 1.5)
        assert ops._x6_planes("ffn", x, w12, w3, gate=w12) is None
        stale = ffn(x)
        ops.X6_LINEAR = False
        try:
            off = ffn(x)
        finally:
            ops.X6_LINEAR = True
        assert torch.equal(stale, off) and not torch.equal(stale, on)
        tr.g_optim.refresh_shadow()
        assert ops._x6_planes("ffn", x, w12, w3, gate=w12) is not None
        _assert_planes_current(gen)
        assert_close(ffn(x), off, 3e-6, "the refreshed planes hold the new weight")


def test_captured_steps_equal_eager_steps(device, reproducible):
    from amk.train import VQGANTrainStep

    gen0, dis0, imgs, eta = _nets(device)
    runs = []
    for graphed in (False, True):
        gen, dis = copy.deepcopy(gen0), copy.deepcopy(dis0)
        tr = VQGANTrainStep(gen, dis, lr=1e-3, warmup_steps=2, decay_steps=50, capturable=True)
        assert _with_planes(gen)
        draw = tr.gradient_penalty
        tr.gradient_penalty = lambda real, fake, e=None: draw(real, fake, eta)   # (a replay would re-use its captured draw)
        if graphed:
            tr.capture(imgs, warmup=2)
        else:
            tr.step(imgs), tr.step(imgs)
        logs = [{k: v.clone() for k, v in tr.step(imgs).items() if torch.is_tensor(v)} for _ in range(3)]
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graphed
        _assert_planes_current(gen)
        runs.append((logs, [p.detach().clone() for p in gen.parameters()]))
    (l0, p0), (l1, p1) = runs
    for a, b in zip(l0, l1):
        assert a.keys() == b.keys() and "loss" in a
        for k in a:
            assert torch.equal(a[k], b[k]), (k, a[k], b[k])
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)


def test_autocast_switch_leaves_no_stale_planes(device, reproducible):
    from amk.train import VQGANTrainStep

    gen, dis, imgs, eta = _nets(device)
    tr = VQGANTrainStep(gen, dis, lr=1e-3, warmup_steps=0, decay_steps=1000)
    tr.step(imgs, eta=eta)
    tr.autocast = torch.bfloat16
    assert not _with_planes(gen) and tr.g_optim.planes_bytes == 0
    tr.step(imgs, eta=eta)             # the weights move while no planes are kept
    tr.autocast = None
    assert not any(hasattr(p, "_amk_bf16") for p in gen.parameters())
    _assert_planes_current(gen)
    tr.step(imgs, eta=eta)
    _assert_planes_current(gen)


def test_step_on_planes_agrees_with_step_off(device, reproducible):
    ops = reproducible
    from amk.train import VQGANTrainStep

    gen0, dis0, imgs, eta = _nets(device)
    out = []
    for on in (True, False):
        gen, dis = copy.deepcopy(gen0), copy.deepcopy(dis0)
        ops.X6_LINEAR = on            # (AMK_X6_LINEAR)
        try:
            tr = VQGANTrainStep(gen, dis, lr=1e-3, warmup_steps=0, decay_steps=1000)
            assert bool(_with_planes(gen)) == on
            logs = tr.step(imgs, eta=eta)
        finally:
            ops.X6_LINEAR = True
        moments = [opt.state_of(p)["exp_avg"].clone() for opt in (tr.g_optim, tr.d_optim) for p in opt.params]
        name_of = {id(p): n for net in (gen, dis) for n, p in net.named_parameters()}
        out.append(({k: float(logs[k]) for k in ("d_loss", "g_loss", "l1", "l2", "codebook_loss", "loss")}, moments,
                    [name_of[id(p)] for opt in (tr.g_optim, tr.d_optim) for p in opt.params]))
    (la, ma, names), (lb, mb, _) = out
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-4 * max(1.0, abs(lb[k])), (k, la[k], lb[k])
    for n, a, b in zip(names, ma, mb):
        assert_close(a, b, 1e-4, n + " (first moment)")
