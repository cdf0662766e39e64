"""The masked-token loss head (csrc/ce_head.hip, ops.linear_cross_entropy) on the MI355X: loss, dx and dw held
element-wise to both tiers of tests/ce_head_ref.py over tile edges, valid-row patterns and input families; skipped rows
really skipped; out-of-range targets; padded layouts; reproducibility; graph capture; the reference's own numbers; the
models' switch; the gradient reducer's direct writes."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import ce_head_ref as ref
from util import GOLDEN, assert_close, load_golden, weights_of

pytestmark = pytest.mark.gpu

D_LOSS = 0.7
WORST = {}   # name -> [hard ratio, q / (TIGHT_FACTOR Q_EMU)], printed by the last test of the file


def _op(x, w, target, ignore_index=-1, d_loss=D_LOSS):
    from amk import ops

    xg, wg = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    loss = ops.linear_cross_entropy(xg, wg, target, ignore_index)
    (loss * d_loss).backward()
    return loss.detach(), xg.grad, wg.grad


def _hold(got, R, what):
    for name, g in zip(("loss", "dx", "dw"), got):
        nbad, ratio, q = ref.measures(g, R, name)
        tight = q / (ref.TIGHT_FACTOR * ref.Q_EMU[name])
        print(f"{what} {name}: hard ratio {ratio:.4f}, q {q:.4f} ({tight:.4f} of the tight limit)")
        w = WORST.setdefault(name, [0.0, 0.0])
        w[0], w[1] = max(w[0], ratio), max(w[1], tight)
        assert nbad == 0, f"{what} {name}: {nbad} elements outside the hard bound (worst {ratio:.3f} x)"
        assert tight <= 1.0, f"{what} {name}: q {q:.3f} above {ref.TIGHT_FACTOR} x Q_EMU = {ref.TIGHT_FACTOR * ref.Q_EMU[name]}"


def _inputs(family, M, V, K, pattern, device, seed=0):
    target = ref.make_target(M, V, pattern, seed=seed)
    x, w = ref.make_inputs(family, M, V, K, target, seed=seed + K)
    return x.to(device), w.to(device), target.to(device)


def _sweep_cases():
    """A seeded sweep that hits every M, V and K of the tile-edge lists at least once, plus the largest case."""
    Ms, Vs, Ks = [1, 127, 128, 129, 300], [1, 4, 127, 128, 129, 1000], [4, 36, 64, 260]
    g = torch.Generator().manual_seed(7)
    n = max(len(Ms), len(Vs), len(Ks))
    cols = []
    for vals in (Ms, Vs, Ks):
        order = [vals[i] for i in torch.randperm(len(vals), generator=g).tolist()]
        cols.append([order[i % len(order)] for i in range(n)])
    fams = ref.FAMILIES
    cases = [(cols[0][i], cols[1][i], cols[2][i], fams[i % len(fams)]) for i in range(n)]
    cases += [(300, 8192, 64, "unit"), (129, 128, 1024, "peaked"), (300, 8192, 1024, "climb")]
    return cases


@pytest.mark.parametrize("M,V,K,family", _sweep_cases())
def test_tile_edges(device, M, V, K, family):
    x, w, t = _inputs(family, M, V, K, "all" if M == 1 else "random64", device, seed=M + V)
    _hold(_op(x, w, t), ref.reference(x, w, t, -1, D_LOSS), f"edges {M}x{V}x{K} {family}")


@pytest.mark.parametrize("pattern", ["all", "first", "last", "last_tile", "random64", "edges"])
def test_valid_patterns(device, pattern):
    x, w, t = _inputs("unit", 300, 1000, 260, pattern, device)
    _hold(_op(x, w, t), ref.reference(x, w, t, -1, D_LOSS), f"pattern {pattern}")


def test_slice_and_tile_boundary_targets(device):
    """Targets at column 0, V - 1 and on both sides of every slice / tile boundary, four tiles per slice."""
    M, V, K = 300, 8192, 36
    ns, vper = ref.slices(M, V)
    assert vper // ref.TILE == 4 and ns == 16
    x, w, t = _inputs("unit", M, V, K, "edges", device)
    _hold(_op(x, w, t), ref.reference(x, w, t, -1, D_LOSS), "boundary targets")


def test_no_valid_row(device):
    x, w, t = _inputs("unit", 300, 1000, 260, "none", device)
    loss, dx, dw = _op(x, w, t)
    assert bool(torch.isnan(loss)) and not bool(dx.any()) and not bool(dw.any())


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_families(device, family):
    x, w, t = _inputs(family, 129, 1000, 260, "random64", device)
    _hold(_op(x, w, t), ref.reference(x, w, t, -1, D_LOSS), f"family {family}")


def test_climb_over_two_tiles_per_slice(device):
    M, V, K = 129, 4096, 64
    assert ref.slices(M, V)[1] == 2 * ref.TILE
    x, w, t = _inputs("climb", M, V, K, "random64", device)
    _hold(_op(x, w, t), ref.reference(x, w, t, -1, D_LOSS), "climb two tiles")


def test_ignore_index_other_than_minus_one(device):
    x, w, t = _inputs("unit", 129, 129, 36, "random64", device)
    t = torch.where(t == -1, torch.full_like(t, 5), t)     # 5 is also a valid word: those rows are ignored all the same
    got = _op(x, w, t, ignore_index=5)
    _hold(got, ref.reference(x, w, t, 5, D_LOSS), "ignore_index 5")
    xd = x.double().requires_grad_()
    lt = F.cross_entropy(F.linear(xd, w.double()), t, ignore_index=5)
    assert abs(float(got[0]) - float(lt.detach())) < 1e-5


def test_skipped_rows_are_really_skipped(device):
    """NaN / Inf in the x rows whose target is ignored change no bit of loss, dw and the valid dx rows."""
    x, w, t = _inputs("unit", 300, 1000, 260, "random64", device)
    ign = t == -1
    x0 = x.clone()
    x0[ign] = 0
    x1 = x.clone()
    x1[ign] = float("nan")
    x1[ign.nonzero().flatten()[::2]] = float("inf")
    a, b = _op(x0, w, t), _op(x1, w, t)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[1][~ign], b[1][~ign])
    assert bool(torch.isfinite(b[0])) and not bool(b[1][ign].any())
    _hold(b, ref.reference(x0, w, t, -1, D_LOSS), "skipped rows")


def test_out_of_range_targets(device):
    """w is the first V rows of a 2 V-row buffer, so a wrong index would still land inside the allocation."""
    M, V, K = 300, 500, 64
    x, w2, t = _inputs("unit", M, 2 * V, K, "random64", device)
    w = w2[:V]
    t = torch.where(t >= 0, t % V, t)
    valid = (t >= 0).nonzero().flatten()
    bad = t.clone()
    bad[valid[3]], bad[valid[-1]], bad[valid[40]] = V, 2 * V - 1, -7
    from amk import ops

    xg, w2g = x.clone().requires_grad_(), w2.clone().requires_grad_()
    loss = ops.linear_cross_entropy(xg, w2g[:V], bad, -1)      # the kernels read the view: rows V .. 2 V lie behind it
    (loss * D_LOSS).backward()
    loss, dx, dw = loss.detach(), xg.grad, w2g.grad[:V]
    assert not bool(w2g.grad[V:].any())
    R = ref.reference(x, w, bad, -1, D_LOSS)
    assert bool(torch.isnan(loss)) and R["poisoned"]
    for r in (valid[3], valid[-1], valid[40]):
        assert not bool(dx[r].any())
    _hold((loss, dx, dw), R, "out of range")
    # the same gradient as with those rows dropped, up to the mean's divisor (count includes them)
    dropped = t.clone()
    dropped[valid[3]] = dropped[valid[-1]] = dropped[valid[40]] = -1
    Rd = ref.reference(x, w, dropped, -1, D_LOSS)
    scale = Rd["count"] / R["count"]
    nbad, _, _ = ref.measures(dw.double() / scale, Rd, "dw")
    assert nbad == 0


def _raw(L, x, w, t, ignore_index, d_loss, dx, dw):
    from amk import lib as amk_lib

    P = lambda a: ctypes.c_void_p(a.data_ptr())
    M, K = x.shape
    V = w.shape[0]
    dev = x.device
    loss, lse = torch.empty((), device=dev), torch.empty(M, device=dev)
    rows, count = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    nf, nb = L.amk_ce_head_fwd_ws_bytes(M, V, K), L.amk_ce_head_bwd_ws_bytes(M, V, K)
    ws = torch.empty(max(nf, nb) // 4, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    amk_lib.check(L.amk_ce_head_fwd(P(x), x.stride(0), P(w), w.stride(0), P(t), ignore_index, M, V, K, P(loss), P(lse), P(rows),
                                    P(count), P(ws), nf, st), "fwd")
    d = torch.tensor([d_loss], device=dev)
    amk_lib.check(L.amk_ce_head_bwd(P(x), x.stride(0), P(w), w.stride(0), P(t), ignore_index, M, V, K, P(d), P(lse), P(rows),
                                    P(count), P(dx), dx.stride(0), P(dw), dw.stride(0), P(ws), nb, st), "bwd")
    return loss, rows, count


def test_padded_layouts_and_compaction(device):
    """Padded ldx / ldw / lddx / lddw: nothing is written outside the views; rows and count are the valid indices."""
    from amk import lib as amk_lib

    L = amk_lib.load()
    M, V, K = 129, 127, 36
    x, w, t = _inputs("unit", M, V, K, "random64", device)
    SENT = 12345.0
    xb, wb = torch.full((M, K + 8), SENT, device=device), torch.full((V, K + 4), SENT, device=device)
    xb[:, :K], wb[:, :K] = x, w
    dxb, dwb = torch.full((M, K + 12), SENT, device=device), torch.full((V, K + 4), SENT, device=device)
    loss, rows, count = _raw(L, xb[:, :K], wb[:, :K], t, -1, D_LOSS, dxb[:, :K], dwb[:, :K])
    assert bool((dxb[:, K:] == SENT).all()) and bool((dwb[:, K:] == SENT).all())
    valid = (t != -1).nonzero().flatten()
    assert int(count) == valid.numel() and torch.equal(rows[:valid.numel()].long(), valid) and bool((rows[valid.numel():] == -1).all())
    got = (loss, dxb[:, :K], dwb[:, :K])
    _hold(got, ref.reference(x, w, t, -1, D_LOSS), "padded")
    plain = _op(x, w, t)
    assert all(torch.equal(a, b.contiguous()) for a, b in zip(plain, got))      # the layout changes no bit


def test_run_to_run_bitwise(device):
    x, w, t = _inputs("peaked", 300, 1000, 260, "random64", device)
    a, b = _op(x, w, t), _op(x, w, t)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_graph_capture_with_changing_valid_counts(device):
    """Forward + backward captured once; replays with targets of different valid counts equal the eager results bitwise
    (the count never reaches the host).  Single stream."""
    from amk import ops
    from amk.graphs import GraphedStep

    M, V, K = 300, 1000, 64
    x, w, t0 = _inputs("unit", M, V, K, "random64", device)
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()

    def fn(t):
        loss = ops.linear_cross_entropy(xg, wg, t, -1)
        dx, dw = torch.autograd.grad(loss * D_LOSS, (xg, wg))
        return loss, dx, dw

    step = GraphedStep(fn, [t0])
    for pattern in ("first", "last_tile", "all", "none", "random64"):
        t = ref.make_target(M, V, pattern, seed=3).to(device)
        out = [o.clone() for o in step.replay(t)]
        eager = _op(x, w, t)
        for a, b in zip(out, eager):
            assert torch.equal(a, b) or (bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())), pattern


# ---------------------------------------------------------------------------------------------- models
def _abs_close(a, b, tol, what):
    a, b = a.detach().cpu().double(), torch.as_tensor(b).double()
    scale = max(float(b.abs().max()), 1e-4)
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"{what}: abs err {err:.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("variant", ["plain", "ctxmask"])
def test_loss_method_against_the_reference_numbers(device, variant):
    """muse_decoder_small: loss_from_hidden gives the reference's loss and gradients at the tolerances
    test_muse_decoder_small_golden uses for this fixture."""
    from amk import ops
    from amk.models import BidirectionalDecoder

    fx = load_golden("muse_decoder_small")
    meta = json.load(open(os.path.join(GOLDEN, "golden_meta.json")))["muse_decoder_small"]
    m = BidirectionalDecoder(**meta["cfg"])
    m.load_state_dict(weights_of(fx), strict=True)
    m = m.to(device)
    ctx = torch.from_numpy(fx["context"]).to(device).requires_grad_(True)
    kw = {} if variant == "plain" else dict(context_mask=torch.from_numpy(fx["cmask"]).to(device))
    ops.KERNEL_EVENTS = {}
    try:
        loss = m.loss_from_hidden(m.hidden(torch.from_numpy(fx["ids"]).to(device), context=ctx, **kw),
                                  torch.from_numpy(fx["tgt"]).to(device), -1)
        loss.backward()
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    assert any(n.startswith("ce_head_fwd") for n in names) and any(n.startswith("ce_head_bwd") for n in names)
    assert_close(loss, fx[f"{variant}:loss"], 5e-5, "loss")
    _abs_close(ctx.grad, fx[f"{variant}:gctx"], 3e-4, "grad context")
    checked = 0
    for n, p in m.named_parameters():
        if f"{variant}:g:{n}" in fx:
            _abs_close(p.grad, fx[f"{variant}:g:{n}"], 3e-4, f"grad {n}")
            checked += 1
    # (the fixture holds parameter gradients for the plain variant only)
    assert checked == sum(k.startswith(f"{variant}:g:") for k in fx) and (checked > 10 or variant != "plain")
    assert m.linear.weight.grad is not None


def _small_models(device):
    from amk.models import MUSE, ViTVQGAN
    from amk.models.maskgit import MaskGitTransformer

    torch.manual_seed(0)
    vq = ViTVQGAN(dict(dim=64, img_size=32, patch_size=8, n_heads=1, d_head=64, depth=1, mlp_dim=64, dropout=0.0),
                  dict(codebook_size=64, codebook_dim=32))
    muse = MUSE(dim=64, vq=vq, text_dim=24, n_heads=1, d_head=64, depth=2, mult=4).to(device)
    torch.manual_seed(1)
    vq2 = ViTVQGAN(dict(dim=64, img_size=32, patch_size=8, n_heads=1, d_head=64, depth=1, mlp_dim=64, dropout=0.0),
                   dict(codebook_size=64, codebook_dim=32))
    mg = MaskGitTransformer(dim=64, vq=vq2, vocab_size=64, n_heads=1, d_head=64, dec_depth=2, mult=4, dropout=0.0).to(device)
    mg.train()
    imgs = torch.rand(3, 3, 32, 32, device=device)
    text = torch.randn(3, 7, 24, device=device)
    return {"muse": (muse, lambda: muse(text, imgs)), "maskgit": (mg, lambda: mg(imgs))}


def _step(model, call, on, monkeypatch, autocast=False):
    from amk import ops

    monkeypatch.setattr(ops, "CE_HEAD", on)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    ops.KERNEL_EVENTS = {}
    try:
        if autocast:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = call()
        else:
            loss = call()
        loss.float().backward()
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return loss.detach().float(), grads, [n for n in names if n.startswith("ce_head")]


@pytest.mark.parametrize("which", ["muse", "maskgit"])
def test_model_switch_changes_the_path_not_the_step(device, monkeypatch, which):
    model, call = _small_models(device)[which]
    loss0, g0, k0 = _step(model, call, False, monkeypatch)
    loss1, g1, k1 = _step(model, call, True, monkeypatch)
    assert not k0 and len(k1) == 2
    assert_close(loss1, loss0, 5e-5, "loss")
    assert set(g0) == set(g1) and len(g0) > 10
    for n in g0:
        _abs_close(g1[n], g0[n].cpu(), 3e-4, f"grad {n}")
    _, _, k2 = _step(model, call, True, monkeypatch, autocast=True)
    assert not k2, "the f32 loss head must not run under bf16 autocast"


def test_reducer_receives_the_weight_gradient_in_its_bucket(device):
    from amk import ops
    from amk.dp import GradReducer

    M, V, K = 129, 256, 64
    x, w0, t = _inputs("unit", M, V, K, "random64", device)
    plain = _op(x, w0, t, d_loss=1.0)
    w = torch.nn.Parameter(w0.clone())
    red = GradReducer([w], direct_grads=True)
    if not red.direct_grads:
        pytest.skip("AMK_DIRECT_GRADS=0 in the environment")
    red.begin(sync=True)
    xg = x.clone().requires_grad_()
    ops.linear_cross_entropy(xg, w, t, -1).backward()
    red.finish(detach_unused=False)
    assert sum(sum(bk.direct) for bk in red.buckets) == 1
    assert w.grad.data_ptr() == red.buckets[0].views[0].data_ptr()
    assert torch.equal(w.grad, plain[2]) and torch.equal(xg.grad, plain[1])


def test_zz_report_worst_ratios(capsys):
    with capsys.disabled():
        print("\nce_head worst (hard ratio, q / (4 Q_EMU)):", {k: (round(a, 4), round(b, 4)) for k, (a, b) in WORST.items()})
    assert not WORST or set(WORST) == {"loss", "dx", "dw"}
