"""The whole GAN step with the gradient penalty ON (gp_lambda = 10: the one double backward of the step, through the fused
BatchNorm + LeakyReLU kernels) under the allocation poisoner of tests/poison.py, at the size of
tests/test_models_gpu.py::_graph_replay_case: eager under both fills, captured with the fills inside the graph (every replay
poisons again), and -- without poison -- the allocation order of tools/kbench_lpips.py --step: two trainers, each with a
captured step, replayed in turn.  f32 and bf16 autocast, without the perceptual term and with it on the torch chain
(ops.LPIPS 0) and on the fused head (ops.LPIPS 1).  Everything runs on the reproducible attention backward and with the
convolutions' deterministic algorithms, so that identical inputs give identical bits."""
import copy

import pytest
import torch

from poison import poisoned_empty

pytestmark = pytest.mark.gpu

VIT = dict(dim=64, img_size=32, patch_size=8, n_heads=1, d_head=64, depth=1, mlp_dim=128, dropout=0.0)
# (autocast, perceptual term, ops.LPIPS)
CONFIGS = [(None, False, False), (None, True, False), (None, True, True),
           (torch.bfloat16, False, False), (torch.bfloat16, True, False), (torch.bfloat16, True, True)]
_ID = lambda c: f"{'bf16' if c[0] else 'f32'}_{('lpips_fused' if c[2] else 'lpips_chain') if c[1] else 'no_per_loss'}"  # noqa: E731
ROUNDS = 12


@pytest.fixture
def reproducible(monkeypatch):
    from amk import ops

    monkeypatch.setattr(ops, "DETERMINISTIC_ATTENTION_BACKWARD", True)    # no dq atomics, ordered codebook gradient
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield monkeypatch
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def _parts(device, cfg, monkeypatch):
    from amk import ops
    from amk.models import LPIPS, ViTVQGAN
    from amk.models.discriminator import NLayerDiscriminator

    autocast, with_per, fused = cfg
    monkeypatch.setattr(ops, "LPIPS", fused)
    torch.manual_seed(0)
    model = ViTVQGAN(VIT, dict(codebook_size=64, codebook_dim=32)).to(device)
    discr = NLayerDiscriminator(3, 8, 3).to(device)
    per = LPIPS().to(device) if with_per else None
    img = torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(device)
    eta = torch.rand(4, 1, 1, 1, generator=torch.Generator().manual_seed(4)).to(device)
    return model, discr, per, img, eta


def _trainer(model, discr, per, cfg, **kw):
    from amk.train import VQGANTrainStep

    return VQGANTrainStep(copy.deepcopy(model), copy.deepcopy(discr), warmup_steps=1, gp_lambda=10.0, autocast=cfg[0],
                          per_loss=per, per_loss_weight=1.0, **kw)


def _close(le, lg, what):
    for k in le:
        assert bool(torch.isfinite(lg[k])) and bool(torch.isfinite(le[k])), f"{what}: {k} is not finite"
        assert float((le[k] - lg[k]).abs()) <= 2e-5 * max(1.0, float(le[k].abs())), f"{what}: {k} {float(le[k])} / {float(lg[k])}"


def _params_close(a, b, what):
    for mod in ("model", "discr"):
        for (n, p), q in zip(getattr(a, mod).named_parameters(), getattr(b, mod).parameters()):
            p, q = p.detach(), q.detach()
            assert bool(torch.isfinite(q).all()), f"{what}: {mod} {n} is not finite"
            assert float((p - q).abs().max()) <= 2e-5 * max(1.0, float(p.abs().max())), f"{what}: {mod} {n}"


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_eager_steps_do_not_depend_on_the_fill(device, reproducible, cfg):
    """Two trainers from identical copies, three steps each, one under each fill: every log and every parameter finite and
    bitwise equal."""
    model, discr, per, img, eta = _parts(device, cfg, reproducible)
    runs = {}
    for fill in ("nan", "big"):
        with poisoned_empty(fill):
            tr = _trainer(model, discr, per, cfg)
            logs = [{k: v.detach().clone() for k, v in tr.step(img, eta=eta).items()} for _ in range(3)]
        torch.cuda.synchronize()
        runs[fill] = (tr, logs)
    (ta, la), (tb, lb) = runs["nan"], runs["big"]
    assert "d_loss" in la[0] and ("per_loss" in la[0]) == cfg[1]
    for s, (x, y) in enumerate(zip(la, lb)):
        for k in x:
            assert bool(torch.isfinite(x[k])) and bool(torch.isfinite(y[k])), f"step {s}: {k} is not finite ({float(x[k])}, {float(y[k])})"
            assert torch.equal(x[k], y[k]), f"step {s}: {k} differs between the fills: {float(x[k])!r} / {float(y[k])!r}"
    for mod in ("model", "discr"):
        for (n, p), q in zip(getattr(ta, mod).named_parameters(), getattr(tb, mod).parameters()):
            assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(q).all()), f"{mod} {n} is not finite"
            assert torch.equal(p, q), f"{mod} {n} differs between the fills in {int((p != q).sum())} of {p.numel()} elements"


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_step_captured_under_poison_matches_eager_steps(device, reproducible, cfg):
    """The capture is taken inside poisoned_empty("nan"): the fills are nodes of the graph, so every replay finds NaN in
    every buffer the step allocates.  Twelve replays against an eager twin's twelve steps."""
    from amk.graphs import GraphedStep

    model, discr, per, img, eta = _parts(device, cfg, reproducible)
    eager = _trainer(model, discr, per, cfg, capturable=True)
    graphed = _trainer(model, discr, per, cfg, capturable=True)
    graphed._set_lr()
    with poisoned_empty("nan"):
        g = GraphedStep(lambda x, e: graphed.step_body(x, True, 1, e), [img, eta], warmup=1)   # one eager step, then the capture
    graphed.global_step = 1
    eager.step(img, eta=eta)
    for r in range(ROUNDS):
        le = eager.step(img, eta=eta)
        graphed._set_lr()
        lg = g.replay(img, eta)
        graphed.global_step += 1
        _close(le, lg, f"replay {r}")
    _params_close(eager, graphed, "after the replays")


@pytest.mark.parametrize("cfg", CONFIGS, ids=_ID)
def test_two_captured_trainers_replayed_in_turn(device, reproducible, cfg):
    """tools/kbench_lpips.py --step in small: trainer A is built, stepped and captured; only then trainer B is built, takes
    three eager steps and is captured (its graph's pool is allocated after A's); A and B replay alternately.  Each is held
    to its own eager twin.  No poison."""
    from amk.graphs import GraphedStep

    model, discr, per, img, eta = _parts(device, cfg, reproducible)
    pairs = []
    for name in ("A", "B"):
        tr = _trainer(model, discr, per, cfg, capturable=True)
        for _ in range(3):
            tr.step(img, eta=eta)
        g = GraphedStep(lambda x, e, tr=tr: tr.step_body(x, True, 1, e), [img, eta], warmup=2, before_each=tr._tick)
        pairs.append((name, tr, g))
    twins = []
    for name, tr, g in pairs:
        tw = _trainer(model, discr, per, cfg, capturable=True)
        for _ in range(5):
            tw.step(img, eta=eta)
        assert tw.global_step == tr.global_step == 5
        twins.append(tw)
    for r in range(ROUNDS):
        for (name, tr, g), tw in zip(pairs, twins):
            le = tw.step(img, eta=eta)
            tr._set_lr()
            lg = g.replay(img, eta)
            tr.global_step += 1
            _close(le, lg, f"round {r}, trainer {name}")
    for (name, tr, g), tw in zip(pairs, twins):
        _params_close(tw, tr, f"trainer {name}")
