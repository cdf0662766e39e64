"""csrc/lpips.hip on the MI355X (amk_lpips_fwd / _bwd and the bf16 pair) against the fp64 reference and the per-element bounds
of tests/lpips_ref.py, through the C ABI called the way ops._LpipsDist calls it: a seeded sweep over the channel counts, plane
sizes and batch sizes at which the kernels take another path, every input family at one mid shape, the exact results
(identical inputs, zero-norm pixels), batch invariance and run-to-run reproducibility (bitwise), sentinels around every output
and the refusals; then ops.lpips_distance's dispatch, amk.models.LPIPS against the fp64 restatement of the module, and
VQGANTrainStep with the perceptual term, eager with the switch on and off and captured."""
import ctypes

import pytest
import torch

import lpips_ref as ref

pytestmark = pytest.mark.gpu
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
_IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731
PAD, MARK = 64, -12345.0

# (N, C, H, W): C in {1, 3, 64, 65, 512}, HW in {1, 4, 7, 63, 64, 65, 255, 256, 1023, 1025, 4097} (and 4096, a level of the
# step), N in {1, 2, 3}; odd C HW so that planes and samples start misaligned; 1, 4, 16 and 64 channel slices; one tile and
# several; N C HW <= 2^21
SWEEP = [(1, 1, 1, 1), (2, 3, 2, 2), (3, 64, 1, 7), (1, 65, 7, 9), (2, 512, 8, 8), (3, 3, 5, 13), (2, 65, 15, 17),
         (1, 64, 16, 16), (2, 512, 16, 16), (1, 3, 31, 33), (2, 64, 25, 41), (1, 65, 17, 241), (3, 1, 17, 241),
         (1, 512, 31, 33), (2, 1, 16, 16), (3, 65, 8, 8), (1, 512, 2, 2), (2, 64, 2, 2), (1, 64, 64, 64), (2, 3, 64, 64)]
MID = (2, 65, 16, 16)


def test_the_sweep_covers_what_it_claims():
    assert {c[1] for c in SWEEP} == {1, 3, 64, 65, 512} and {c[0] for c in SWEEP} == {1, 2, 3}
    assert {c[2] * c[3] for c in SWEEP} >= {1, 4, 7, 63, 64, 65, 255, 256, 1023, 1025, 4097}
    assert all(c[0] * c[1] * c[2] * c[3] <= 2 ** 21 for c in SWEEP + [MID])
    for vw in (4, 8):
        geos = [ref.make_geo(c[1], c[2] * c[3], vw) for c in SWEEP]
        assert {g["CS"] for g in geos} == {1, 4, 16, 64} and {g["W"] for g in geos} == {1, vw}
        assert any(g["tiles"] > 1 and g["CS"] == 1 for g in geos) and any(g["tiles"] > 1 and g["CS"] > 1 for g in geos)
    assert any((c[1] * c[2] * c[3]) % 2 for c in SWEEP if c[0] > 1)


def _guarded(n, dtype, device):
    """A tensor of n elements inside a buffer with PAD marked elements on each side (the view stays 16-byte aligned)."""
    buf = torch.full((n + 2 * PAD,), MARK, device=device, dtype=dtype)
    return buf, buf[PAD:PAD + n]


def _untouched(buf, n):
    return bool((buf[:PAD] == MARK).all()) and bool((buf[PAD + n:] == MARK).all())


def _abi(inp, device, bf16):
    """amk_lpips[_bf16]_fwd and _bwd as ops._LpipsDist calls them; every output sits between sentinels.  CPU tensors back."""
    from amk import lib, ops

    L, P = lib.load(), ops._ptr
    dt = BF16 if bf16 else F32
    a, b = (inp[k].to(device=device, dtype=dt).contiguous() for k in ("a", "b"))
    w, g = inp["w"].to(device), inp["g"].to(device)
    N, C, H, W = a.shape
    HW = H * W
    pre = "amk_lpips_bf16_" if bf16 else "amk_lpips_"
    nws = int(getattr(L, pre + "ws_floats")(N, C, HW))
    assert nws == ref.ws_floats(N, C, HW, 8 if bf16 else 4)
    bufs = dict(out=_guarded(N, F32, device), rows=_guarded(3 * N * HW, F32, device), ws=_guarded(nws, F32, device),
                ga=_guarded(N * C * HW, dt, device))
    out, rows, ws, ga = (bufs[k][1] for k in ("out", "rows", "ws", "ga"))
    lib.check(getattr(L, pre + "fwd")(P(a), P(b), P(w), N, C, HW, ref.EPS, P(out), P(rows), P(ws), ops._stream()), pre + "fwd")
    lib.check(getattr(L, pre + "bwd")(P(g), P(a), P(b), P(w), P(rows), N, C, HW, ref.EPS, P(ga), ops._stream()), pre + "bwd")
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        assert _untouched(buf, view.numel()), f"a write outside {name}"
        assert not bool((view == MARK).any()) or name == "ws", f"{name} not fully written"
    return dict(out=out.cpu().clone(), ga=ga.view(N, C, H, W).cpu().clone(), rows=rows.view(3, N, HW).cpu().clone())


def _check(inp, device, bf16, what, record):
    got = _abi(inp, device, bf16)
    R = ref.reference(inp, bf16=bf16)
    q = ref.ratios(got, R, record=record)
    print(what, {k: round(v, 4) for k, v in q.items()})
    assert bool(torch.isfinite(got["out"]).all()) and bool(torch.isfinite(got["ga"].float()).all()), what
    assert q["out"] <= 1.0 and q["ga"] <= 1.0, (what, q)
    return got


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", SWEEP, ids=_IDS)
def test_kernels_within_bounds_over_the_sweep(device, case, bf16):
    i = SWEEP.index(case)
    family = ("relu", "near", "zero_pixels")[i % 3]
    inp = ref.make_inputs(family, case, ref.WEIGHTS[i % 2], seed=i, bf16=bf16)
    _check(inp, device, bf16, f"{family} {case} {'bf16' if bf16 else 'f32'}", "bf16" if bf16 else "f32")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("weights", ref.WEIGHTS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_every_family_at_the_mid_shape(device, family, weights, bf16):
    inp = ref.make_inputs(family, MID, weights, bf16=bf16)
    got = _check(inp, device, bf16, f"{family} {weights} {'bf16' if bf16 else 'f32'}", "bf16" if bf16 else "f32")
    if family == "identical":                                   # exactly zero, value and gradient
        assert not bool(got["out"].any()) and not bool(got["ga"].any())
    dead = (inp["a"].pow(2).sum(1, keepdim=True) == 0)
    if family == "zero_pixels":
        assert bool(dead.any()) and not bool(dead.all())
    assert not bool(got["ga"][dead.expand_as(inp["a"])].any())
    assert bool((got["rows"][0].reshape(dead[:, 0].shape) == 0).eq(dead[:, 0]).all())     # row 0 marks the zero norm


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(3, 65, 15, 17), (2, 512, 16, 16), (3, 64, 64, 64)], ids=_IDS)
def test_a_sample_alone_equals_the_sample_in_its_batch_and_runs_repeat(device, case, bf16):
    """Bitwise.  Sample 1 is run inside its batch and alone (in (3, 65, 15, 17) it starts at an odd element inside the batch
    and at an aligned one alone); and the same call twice gives the same bits."""
    inp = ref.make_inputs("relu", case, "mixed", seed=5, bf16=bf16)
    full, again = _abi(inp, device, bf16), _abi(inp, device, bf16)
    for name in ("out", "ga", "rows"):
        assert torch.equal(full[name], again[name]), name
    one = dict(inp, a=inp["a"][1:2].clone(), b=inp["b"][1:2].clone(), g=inp["g"][1:2].clone())
    got = _abi(one, device, bf16)
    assert torch.equal(got["out"][0], full["out"][1]) and torch.equal(got["ga"][0], full["ga"][1])
    assert torch.equal(got["rows"][:, 0], full["rows"][:, 1])


def test_refusals_come_before_any_launch(device):
    from amk import lib, ops

    L, P = lib.load(), ops._ptr
    N, C, HW = 2, 8, 16
    null = ctypes.c_void_p(0)
    for bf16 in (False, True):
        pre = "amk_lpips_bf16_" if bf16 else "amk_lpips_"
        dt = BF16 if bf16 else F32
        a = torch.rand(N * C * HW + 8, device=device).to(dt)
        b = torch.rand(N * C * HW + 8, device=device).to(dt)
        w, g = torch.rand(C, device=device), torch.rand(N, device=device)
        bufs = dict(out=_guarded(N, F32, device), rows=_guarded(3 * N * HW, F32, device), ws=_guarded(64, F32, device),
                    ga=_guarded(N * C * HW + 8, dt, device))
        out, rows, ws, ga = (bufs[k][1] for k in ("out", "rows", "ws", "ga"))
        off = ctypes.c_void_p(a.data_ptr() + a.element_size())            # not 16-byte aligned
        ga_off = ctypes.c_void_p(ga.data_ptr() + ga.element_size())
        fwd, bwd = getattr(L, pre + "fwd"), getattr(L, pre + "bwd")
        st = ops._stream()
        def refused(rc, code, word):
            assert rc == code and word in L.amk_last_error(), (rc, L.amk_last_error())
        refused(fwd(null, P(b), P(w), N, C, HW, ref.EPS, P(out), P(rows), P(ws), st), -1, b"null")
        refused(fwd(P(a), P(b), P(w), N, C, HW, ref.EPS, P(out), null, P(ws), st), -1, b"null")
        refused(fwd(P(a), P(b), P(w), 0, C, HW, ref.EPS, P(out), P(rows), P(ws), st), -1, b"non-positive")
        refused(fwd(P(a), P(b), P(w), N, 0, HW, ref.EPS, P(out), P(rows), P(ws), st), -1, b"non-positive")
        refused(fwd(P(a), P(b), P(w), N, C, 0, ref.EPS, P(out), P(rows), P(ws), st), -1, b"non-positive")
        refused(fwd(off, P(b), P(w), N, C, HW, ref.EPS, P(out), P(rows), P(ws), st), -1, b"16-byte")
        refused(fwd(P(a), off, P(w), N, C, HW, ref.EPS, P(out), P(rows), P(ws), st), -1, b"16-byte")
        refused(fwd(P(a), P(b), P(w), 1 << 20, 1, (1 << 19) + 1, ref.EPS, P(out), P(rows), P(ws), st), -2, b"2^31")
        refused(bwd(P(g), P(a), P(b), P(w), P(rows), N, C, HW, ref.EPS, null, st), -1, b"null")
        refused(bwd(null, P(a), P(b), P(w), P(rows), N, C, HW, ref.EPS, P(ga), st), -1, b"null")
        refused(bwd(P(g), P(a), P(b), P(w), P(rows), N, C, -1, ref.EPS, P(ga), st), -1, b"non-positive")
        refused(bwd(P(g), P(a), P(b), P(w), P(rows), N, C, HW, ref.EPS, ga_off, st), -1, b"16-byte")
        refused(bwd(P(g), P(a), P(b), P(w), P(rows), 1 << 20, 1, (1 << 19) + 1, ref.EPS, P(ga), st), -2, b"2^31")
        assert int(getattr(L, pre + "ws_floats")(0, C, HW)) == 0
        torch.cuda.synchronize()
        for name, (buf, view) in bufs.items():                               # nothing was launched: nothing was written
            assert bool((buf == MARK).all()), name


# ---------------------------------------------------------------------------------------------- the op
FUSED = {"lpips_fwd", "lpips_bwd", "lpips_bf16_fwd", "lpips_bf16_bwd"}


def _op_inputs(device, bf16=False):
    inp = ref.make_inputs("relu", MID, "pos", seed=2, bf16=bf16)
    dt = BF16 if bf16 else F32
    return inp, inp["a"].to(device=device, dtype=dt).requires_grad_(), inp["b"].to(device=device, dtype=dt), inp["w"].to(device)


def test_op_runs_the_fused_kernels_and_equals_the_abi(device, monkeypatch):
    from amk import ops

    monkeypatch.setattr(ops, "LPIPS", True)
    for bf16 in (False, True):
        inp, a, b, w = _op_inputs(device, bf16)
        monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
        with torch.autocast("cuda", dtype=BF16, enabled=bf16):
            assert ops.lpips_distance_ok(a, b, w)
            out = ops.lpips_distance(a, b, w)
        assert out.dtype == F32 and tuple(out.shape) == (2,) and type(out.grad_fn).__name__ == "_LpipsDistBackward"
        (ga,) = torch.autograd.grad(out, a, inp["g"].to(device))
        torch.cuda.synchronize()
        names = {"lpips_bf16_fwd", "lpips_bf16_bwd"} if bf16 else {"lpips_fwd", "lpips_bwd"}
        assert set(ops.KERNEL_EVENTS) == names
        monkeypatch.setattr(ops, "KERNEL_EVENTS", None)
        direct = _abi(inp, device, bf16)
        assert ga.dtype == a.dtype and torch.equal(out.cpu(), direct["out"]) and torch.equal(ga.cpu(), direct["ga"])


def test_op_keeps_the_chain_for_what_the_kernels_do_not_take(device, monkeypatch):
    from amk import ops

    inp, a, b, w = _op_inputs(device)
    g = inp["g"].to(device)
    monkeypatch.setattr(ops, "LPIPS", True)
    want = ops.lpips_distance(a, b, w)
    (gwant,) = torch.autograd.grad(want, a, g)
    tol = lambda t: 1e-5 * float(t.abs().max())  # noqa: E731  (two f32 evaluations of the same sums)
    monkeypatch.setattr(ops, "KERNEL_EVENTS", {})

    def chain(a_, b_, w_, **kw):
        with torch.autocast("cuda", **kw) if kw else torch.autocast("cuda", enabled=False):
            assert not ops.lpips_distance_ok(a_, b_, w_)
            out = ops.lpips_distance(a_, b_, w_)
        assert "LpipsDist" not in type(out.grad_fn).__name__
        return out

    # a non-contiguous feature and a channels-last one
    at = a.detach().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_()
    out = chain(at, b, w)
    assert float((out.detach() - want.detach()).abs().max()) <= tol(want.detach())
    chain(a.detach().contiguous(memory_format=torch.channels_last).requires_grad_(), b, w)
    # a b that requires grad: both gradients are the chain's
    br = b.clone().requires_grad_()
    out = chain(a, br, w)
    ga, gb = torch.autograd.grad(out, (a, br), g)
    assert float((ga - gwant).abs().max()) <= tol(gwant) and bool(torch.isfinite(gb).all()) and bool(gb.any())
    a64, b64 = a.detach().double().requires_grad_(), b.double().requires_grad_()
    ga64, gb64 = torch.autograd.grad(ref.head(a64, b64, w.double()), (a64, b64), g.double())
    assert float((gb - gb64).abs().max()) <= tol(gb64) and float((ga - ga64).abs().max()) <= tol(ga64)
    # a w that requires grad, f16 features, f32 features under autocast, bf16 features outside it, CPU tensors
    chain(a, b, w.clone().requires_grad_())
    chain(a.detach().half(), b.half(), w)
    chain(a, b, w, dtype=BF16)
    chain(a.detach().to(BF16), b.to(BF16), w.to(BF16))
    cpu = ops.lpips_distance(a.detach().cpu(), b.cpu(), w.cpu())
    assert float((cpu - want.detach().cpu()).abs().max()) <= tol(want.detach())
    # the switch off
    monkeypatch.setattr(ops, "LPIPS", False)
    out = chain(a, b, w)
    assert float((out.detach() - want.detach()).abs().max()) <= tol(want.detach())
    torch.cuda.synchronize()
    assert not (set(ops.KERNEL_EVENTS) & FUSED)


# ---------------------------------------------------------------------------------------------- the module
def _deviation(v, want, floor):
    d = (v.detach().to(F64).cpu() - want).abs()
    return float(d.max()), float(d.pow(2).mean().sqrt())


@pytest.mark.parametrize("autocast", [False, True], ids=["f32", "bf16_autocast"])
def test_module_fused_path_is_as_close_to_fp64_as_the_chain(device, monkeypatch, autocast):
    """loss = LPIPS(in0, in1).mean() and d loss / d in0 on 2 x 3 x 32 x 32 (levels 32^2 .. 2^2) against the fp64 restatement:
    the fused path's deviation is at most twice the chain's own, as max and as rms, plus 1e-5 max |reference|."""
    from amk import ops
    from amk.models import LPIPS

    sd, in0, in1, loss64, g64 = ref.module_case(0)
    m = LPIPS().to(device)
    m.load_state_dict(sd)              # a bare LPIPS(): frozen by its constructor, so the heads reach the kernels
    x1 = in1.to(device)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "LPIPS", fused)
        monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
        x = in0.to(device).requires_grad_()
        with torch.autocast("cuda", dtype=BF16, enabled=autocast):
            val = m(x, x1)
            loss = val.mean()
        assert tuple(val.shape) == (2, 1, 1, 1)
        assert val.dtype == (F32 if fused or not autocast else BF16)
        (gx,) = torch.autograd.grad(loss, x)
        torch.cuda.synchronize()
        assert len(ops.KERNEL_EVENTS.get("lpips_bf16_fwd" if autocast else "lpips_fwd", [])) == (5 if fused else 0)
        assert len(ops.KERNEL_EVENTS.get("lpips_bf16_bwd" if autocast else "lpips_bwd", [])) == (5 if fused else 0)
        monkeypatch.setattr(ops, "KERNEL_EVENTS", None)
        assert bool(torch.isfinite(gx).all())
        res[fused] = (abs(float(loss.detach()) - float(loss64)), *_deviation(gx, g64, 0))
    floor_l, floor_g = 1e-5 * abs(float(loss64)), 1e-5 * float(g64.abs().max())
    print("module", "autocast" if autocast else "f32", "fused (loss, grad max, grad rms)", res[True], "chain", res[False],
          "ratios", [res[True][i] / max(res[False][i], 1e-300) for i in range(3)])
    assert res[True][0] <= 2 * res[False][0] + floor_l
    assert res[True][1] <= 2 * res[False][1] + floor_g
    assert res[True][2] <= 2 * res[False][2] + floor_g


# ---------------------------------------------------------------------------------------------- the step
def _step_parts(device, per_weight=1.0, with_per=True, **kw):
    from amk.models import LPIPS, ViTVQGAN
    from amk.models.discriminator import NLayerDiscriminator
    from amk.train import VQGANTrainStep

    vit = dict(dim=64, img_size=32, patch_size=8, n_heads=1, d_head=64, depth=1, mlp_dim=128, dropout=0.0)
    torch.manual_seed(0)
    model = ViTVQGAN(vit, dict(codebook_size=64, codebook_dim=32)).to(device)
    discr = NLayerDiscriminator(3, 8, 3).to(device)
    per = LPIPS().to(device) if with_per else None
    return VQGANTrainStep(model, discr, warmup_steps=1, gp_lambda=0.0, per_loss=per, per_loss_weight=per_weight, **kw), per


def test_step_with_the_perceptual_term_fused_and_chain_agree(device, monkeypatch):
    from amk import ops

    monkeypatch.setattr(ops, "DETERMINISTIC_ATTENTION_BACKWARD", True)
    imgs = torch.rand(4, 3, 32, 32, device=device)
    logs, grads = {}, {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "LPIPS", fused)
        step, per = _step_parts(device)
        assert not per.training and not any(p.requires_grad for p in per.parameters())
        ids = {id(p) for p in per.parameters()}
        assert not ids & {id(p) for red in (step.g_red, step.d_red) for p in red.params}
        monkeypatch.setattr(ops, "KERNEL_EVENTS", {})
        logs[fused] = step.g_phase(imgs, sync=False)
        torch.cuda.synchronize()
        assert bool(set(ops.KERNEL_EVENTS) & FUSED) == fused
        monkeypatch.setattr(ops, "KERNEL_EVENTS", None)
        grads[fused] = {n: p.grad.clone() for n, p in step.model.named_parameters() if p.grad is not None}
        assert all(p.grad is None for p in per.parameters())
    assert set(logs[True]) == {"g_loss", "l1", "l2", "codebook_loss", "loss", "per_loss"}
    assert float(logs[True]["per_loss"]) > 0
    for k in logs[True]:
        assert float((logs[True][k] - logs[False][k]).abs()) <= 2e-5 * max(1.0, float(logs[False][k].abs())), k
    assert set(grads[True]) == set(grads[False]) and grads[True]
    for n, p in grads[False].items():
        assert float((grads[True][n] - p).abs().max()) <= 2e-5 * max(1.0, float(p.abs().max())), n


def test_step_without_the_term_logs_what_it_did(device):
    imgs = torch.rand(4, 3, 32, 32, device=device)
    today = {"g_loss", "l1", "l2", "codebook_loss", "loss"}
    step, _ = _step_parts(device, with_per=False)
    assert set(step.g_phase(imgs, sync=False)) == today
    step, _ = _step_parts(device, per_weight=0.0)
    assert set(step.g_phase(imgs, sync=False)) == today
    assert set(step.step(imgs)) == today | {"d_loss"}


def test_captured_step_with_the_perceptual_term_matches_eager_steps(device, monkeypatch):
    from amk import ops

    monkeypatch.setattr(ops, "LPIPS", True)
    imgs = torch.rand(4, 3, 32, 32, device=device)
    e2, _ = _step_parts(device, capturable=True)
    c2, _ = _step_parts(device, capturable=True)
    c2.model.load_state_dict(e2.model.state_dict())
    c2.discr.load_state_dict(e2.discr.state_dict())
    c2.per_loss.load_state_dict(e2.per_loss.state_dict())
    e2.step(imgs)
    c2.step(imgs)
    c2.capture(imgs, warmup=0)
    for _ in range(2):
        le, lc = e2.step(imgs), c2.step(imgs)
        assert "per_loss" in lc
        for k in le:
            assert float((le[k] - lc[k]).abs()) <= 2e-5 * max(1.0, float(le[k].abs())), k
    assert c2.global_step == e2.global_step == 3
    for (n, p), q in zip(e2.model.named_parameters(), c2.model.parameters()):
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-5 * max(1.0, float(p.detach().abs().max())), n


def test_zz_report_worst_ratios(capsys):
    with capsys.disabled():
        print("\nlpips worst ratios:", {f"{a}:{b}": round(v, 4) for (a, b), v in sorted(ref.WORST.items())})
    assert ref.WORST and all(v <= 1.0 for (_, key), v in ref.WORST.items() if not key.startswith("tight_"))
