"""The LPIPS distance head's reference, bounds and emulation (tests/lpips_ref.py) and amk.models.lpips.LPIPS on the CPU: the
gradient formula against fp64 autograd, the emulation of csrc/lpips.hip's f32 operation order under HALF of every bound on
every family, the module's torch chain in f32 against the fp64 restatement, its state_dict keys, load_vgg16_features and the
constructor's refusals.  No GPU."""
import pytest
import torch

import lpips_ref as ref

F32, F64 = torch.float32, torch.float64
# C x HW chosen for the geometry: no channel split (3 x 35), 4, 16 and 64 slices, vector and scalar walks, more than one tile
SHAPES = [(2, 3, 5, 7), (1, 1, 1, 1), (2, 64, 8, 8), (1, 65, 9, 7), (1, 16, 32, 32), (2, 512, 4, 4), (1, 5, 64, 65)]
MID = (2, 64, 8, 8)
_IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731


@pytest.mark.parametrize("weights", ref.WEIGHTS)
@pytest.mark.parametrize("family", [f for f in ref.FAMILIES if f != "zero_pixels"])
def test_gradient_formula_equals_fp64_autograd(family, weights):
    inp = ref.make_inputs(family, (2, 17, 5, 6), weights)
    a, b, w, g = (inp[k].to(F64) for k in ("a", "b", "w", "g"))
    assert bool((a.pow(2).sum(1) > 0).all())
    a.requires_grad_()
    (auto,) = torch.autograd.grad(ref.head(a, b, w), a, g)
    mine = ref.head_grad(a.detach(), b, w, g)
    assert float((auto - mine).abs().max()) <= 1e-12 * max(1.0, float(auto.abs().max()))


def test_zero_norm_pixels_get_a_zero_gradient_and_autograd_a_nan():
    inp = ref.make_inputs("zero_pixels", (2, 9, 8, 8))
    a, b, w, g = (inp[k].to(F64) for k in ("a", "b", "w", "g"))
    dead = (a.pow(2).sum(1, keepdim=True) == 0).expand_as(a)
    assert bool(dead.any()) and not bool(dead.all())
    mine = ref.head_grad(a, b, w, g)
    assert bool(torch.isfinite(mine).all()) and not bool(mine[dead].any())
    a.requires_grad_()
    (auto,) = torch.autograd.grad(ref.head(a, b, w), a, g)
    assert bool(torch.isnan(auto[dead]).all())
    assert float((auto[~dead] - mine[~dead]).abs().max()) <= 1e-12 * float(mine.abs().max())


def _cases():
    out = [("relu", s, "pos") for s in SHAPES]
    out += [(f, MID, wt) for f in ref.FAMILIES for wt in ref.WEIGHTS if (f, wt) != ("relu", "pos")]
    out += [("zero_pixels", (1, 65, 9, 7), "mixed"), ("near", (1, 16, 32, 32), "pos")]
    return out


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("family,shape,weights", _cases(), ids=_IDS)
def test_emulation_stays_within_half_of_every_bound(family, shape, weights, bf16):
    inp = ref.make_inputs(family, shape, weights, bf16=bf16)
    R = ref.reference(inp, bf16=bf16)
    got = ref.emulate(inp, bf16=bf16)
    q = ref.ratios(got, R)
    print(family, shape, weights, {k: round(v, 4) for k, v in q.items()})
    assert all(v <= 0.5 for v in q.values()), q
    if family == "identical":
        assert not bool(got["out"].any()) and not bool(got["ga"].any())
    dead = (inp["a"].pow(2).sum(1, keepdim=True) == 0).expand_as(inp["a"])
    assert not bool(got["ga"][dead].any()) and bool(torch.isfinite(got["ga"]).all())
    assert bool((got["rows"][0].reshape(dead[:, 0].shape) == 0).eq(dead[:, 0]).all())     # row 0 marks the zero norm


def test_bounds_refuse_a_planted_defect():
    """A gradient without the projection term, a value with one channel left out and a bf16 store that truncates twice all
    land outside."""
    inp = ref.make_inputs("relu", MID)
    R = ref.reference(inp)
    short = ref.head(inp["a"][:, 1:].to(F64), inp["b"][:, 1:].to(F64), inp["w"][1:].to(F64))
    assert ref.ratios(dict(out=short, ga=R["ga"]), R)["out"] > 1.0
    R = ref.reference(inp)
    a, b, w, g = (inp[k].to(F64) for k in ("a", "b", "w", "g"))
    na, _, ah, _, e, wv = ref._parts(a, b, w, ref.EPS)
    no_proj = (2 * g / 64).view(-1, 1, 1, 1) * wv * e / (na + ref.EPS)
    assert ref.ratios(dict(out=R["out"], ga=no_proj), R)["ga"] > 1.0
    inpb = ref.make_inputs("relu", MID, bf16=True)
    Rb = ref.reference(inpb, bf16=True)
    ga32 = ref.emulate(inpb, bf16=False)["ga"]
    trunc = (ga32.view(torch.int32) & -65536).view(F32)                     # two bf16 roundings' worth in the worst case
    trunc2 = ((trunc * (1 - 2.0 ** -7)).view(torch.int32) & -65536).view(F32)
    assert ref.ratios(dict(out=Rb["out"], ga=trunc2), Rb)["ga"] > 1.0


# ---------------------------------------------------------------------------------------------- the module
KEYS = (["scaling_layer.shift", "scaling_layer.scale"]
        + [f"net.slice{s}.{i}.{leaf}" for s, idx in ((1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)), (4, (17, 19, 21)),
                                                      (5, (24, 26, 28))) for i in idx for leaf in ("weight", "bias")]
        + [f"lin{k}.model.1.weight" for k in range(5)] + [f"lins.{k}.model.1.weight" for k in range(5)])


def test_state_dict_keys_and_shapes():
    from amk.models import LPIPS
    from amk.models.lpips import CHANNELS

    m = LPIPS()
    sd = m.state_dict()
    assert sorted(sd) == sorted(KEYS)
    for k, c in enumerate(CHANNELS):
        assert tuple(sd[f"lin{k}.model.1.weight"].shape) == (1, c, 1, 1)
        assert m.lins[k] is getattr(m, f"lin{k}")
        assert float(sd[f"lin{k}.model.1.weight"].min()) >= 0
    assert tuple(sd["scaling_layer.shift"].shape) == (1, 3, 1, 1)
    assert torch.equal(sd["scaling_layer.shift"].flatten(), torch.tensor([-.030, -.088, -.188]))
    assert torch.equal(sd["scaling_layer.scale"].flatten(), torch.tensor([.458, .448, .450]))
    assert not m.training and not any(p.requires_grad for p in m.parameters())     # the lin weights too
    assert tuple(sd["net.slice1.0.weight"].shape) == (64, 3, 3, 3) and tuple(sd["net.slice5.28.weight"].shape) == (512, 512, 3, 3)


@pytest.mark.parametrize("normalize", [False, True])
def test_module_chain_on_the_cpu_matches_the_fp64_restatement(normalize):
    from amk.models import LPIPS

    sd, in0, in1, loss64, g64 = ref.module_case(0)
    m = LPIPS()
    m.load_state_dict(sd)
    if normalize:
        x0, x1 = (in0 + 1) / 2, (in1 + 1) / 2
        want = ref.module_value(sd, x0, x1, normalize=True)
    else:
        x0, x1 = in0, in1
        want = ref.module_value(sd, x0, x1)
    x = x0.clone().requires_grad_()
    val, per = m(x, x1, retPerLayer=True, normalize=normalize)
    assert tuple(val.shape) == (2, 1, 1, 1) and val.dtype == F32 and len(per) == 5
    assert float((val.detach().to(F64) - want).abs().max()) <= 1e-4 * float(want.abs().max())
    if not normalize:
        (gx,) = torch.autograd.grad(val.mean(), x)
        assert abs(float(val.mean()) - float(loss64)) <= 1e-4 * abs(float(loss64))
        assert float((gx.to(F64) - g64).abs().max()) <= 1e-3 * float(g64.abs().max())
    assert float(m(x1, x1).abs().max()) == 0.0


def test_load_vgg16_features_takes_both_key_forms(tmp_path):
    from amk.models import LPIPS

    torch.manual_seed(3)
    src = LPIPS()
    tv = {}
    for key, v in src.net.state_dict().items():                             # slice3.10.weight -> features.10.weight
        tv["features." + key.split(".", 1)[1]] = v.clone()
    tv["classifier.0.weight"] = torch.zeros(2, 2)
    bare = {k[len("features."):]: v for k, v in tv.items() if k.startswith("features.")}
    for form in (tv, bare):
        torch.manual_seed(4)
        m = LPIPS()
        assert not torch.equal(m.net.slice3[1].weight, src.net.slice3[1].weight)
        m.load_vgg16_features(form)
        for (ka, va), (kb, vb) in zip(m.net.state_dict().items(), src.net.state_dict().items()):
            assert ka == kb and torch.equal(va, vb)
    with pytest.raises(KeyError, match="features.28.bias"):
        LPIPS().load_vgg16_features({k: v for k, v in tv.items() if k != "features.28.bias"})
    lin_file = tmp_path / "vgg.pth"                                          # a lin-weight file of the package
    torch.save({k: v for k, v in src.state_dict().items() if k.startswith("lin") and not k.startswith("lins")}, lin_file)
    torch.manual_seed(5)
    m = LPIPS(pretrained=True, model_path=str(lin_file))
    for k in range(5):
        assert torch.equal(m.lins[k].model[1].weight, src.lins[k].model[1].weight)


def test_constructor_refusals():
    from amk.models import LPIPS

    with pytest.raises(RuntimeError, match="download"):
        LPIPS(pretrained=True)
    for net in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match=net):
            LPIPS(net=net)
    with pytest.raises(NotImplementedError, match="spatial"):
        LPIPS(spatial=True)
    assert LPIPS(eval_mode=False).training
    assert "model.0.weight" in LPIPS(use_dropout=False).lin0.state_dict()


def test_training_mode_with_dropout_runs_the_chain(monkeypatch):
    from amk import ops
    from amk.models import LPIPS

    calls = []
    monkeypatch.setattr(ops, "lpips_distance", lambda *a, **k: calls.append(1) or torch.zeros(2))
    m = LPIPS(eval_mode=False)
    x = torch.rand(2, 3, 16, 16)
    m(x, x.flip(0))
    assert not calls
    m.eval()
    m(x, x.flip(0))
    assert len(calls) == 5
