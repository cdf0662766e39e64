"""The masked-token loss head under bf16 autocast (csrc/ce_head_bf16.hip, ops.linear_cross_entropy inside
torch.autocast("cuda", bfloat16)) on the MI355X: loss, dx and dw held element-wise to both tiers of
tests/ce_head_bf16_ref.py over tile edges, valid-row patterns and input families; skipped rows really skipped;
out-of-range targets; padded layouts; reproducibility; graph capture; the accuracy against the library path; the models'
switch; the train step's bf16 shadow and the gradient reducer's direct writes."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ce_head_bf16_ref as ref

pytestmark = pytest.mark.gpu

D_LOSS = 0.7
BF16 = torch.bfloat16
NAMES = ("loss", "dx", "dw")
WORST = {}   # name -> [hard ratio, q / (TIGHT_FACTOR Q_EMU)], printed by the last test of the file


def _op(x, w, target, ignore_index=-1, d_loss=D_LOSS):
    """x bf16, w bf16 values held by an f32 master weight (what the step has): (loss f32, dx bf16, dw f32)."""
    from amk import ops

    xg, wg = x.detach().clone().requires_grad_(), w.detach().float().requires_grad_()
    with torch.autocast("cuda", dtype=BF16):
        loss = ops.linear_cross_entropy(xg, wg, target, ignore_index)
    (loss * d_loss).backward()
    assert loss.dtype == torch.float32 and xg.grad.dtype == x.dtype and wg.grad.dtype == torch.float32
    return loss.detach(), xg.grad, wg.grad


def _hold(got, R, what):
    for name, g in zip(NAMES, got):
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
    """A seeded sweep that hits every M, V and K of the tile-edge lists at least once (K = 8 is below the MFMA depth,
    K = 40 and 264 have tails of 8), plus the largest cases."""
    Ms, Vs, Ks = [1, 127, 128, 129, 300], [1, 8, 127, 128, 129, 1000], [8, 40, 64, 264]
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
    x, w, t = _inputs("unit", 300, 1000, 264, pattern, device)
    _hold(_op(x, w, t), ref.reference(x, w, t, -1, D_LOSS), f"pattern {pattern}")


def test_slice_and_tile_boundary_targets(device):
    """Targets at column 0, V - 1 and on both sides of every slice / tile boundary, four tiles per slice."""
    M, V, K = 300, 8192, 40
    ns, vper = ref.slices(M, V)
    assert vper // ref.TILE == 4 and ns == 16
    x, w, t = _inputs("unit", M, V, K, "edges", device)
    _hold(_op(x, w, t), ref.reference(x, w, t, -1, D_LOSS), "boundary targets")


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_families(device, family):
    x, w, t = _inputs(family, 129, 1000, 264, "random64", device)
    _hold(_op(x, w, t), ref.reference(x, w, t, -1, D_LOSS), f"family {family}")


def test_no_valid_row(device):
    x, w, t = _inputs("unit", 300, 1000, 264, "none", device)
    loss, dx, dw = _op(x, w, t)
    assert bool(torch.isnan(loss)) and not bool(dx.any()) and not bool(dw.any())


def test_ignore_index_other_than_minus_one(device):
    x, w, t = _inputs("unit", 129, 129, 40, "random64", device)
    t = torch.where(t == -1, torch.full_like(t, 5), t)     # 5 is also a valid word: those rows are ignored all the same
    got = _op(x, w, t, ignore_index=5)
    R = ref.reference(x, w, t, 5, D_LOSS)
    _hold(got, R, "ignore_index 5")
    lt = F.cross_entropy(F.linear(x.double(), w.double()), t, ignore_index=5)
    assert abs(float(got[0]) - float(lt)) <= float(R["bound_loss"])


def test_skipped_rows_are_really_skipped(device):
    """NaN / Inf in the x rows whose target is ignored change no bit of loss, dw and the valid dx rows."""
    x, w, t = _inputs("unit", 300, 1000, 264, "random64", device)
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


def _raw(L, x, w, t, ignore_index, d_loss, dx, dw):
    from amk import lib as amk_lib

    P = lambda a: ctypes.c_void_p(a.data_ptr())
    M, K = x.shape
    V = w.shape[0]
    dev = x.device
    loss, lse = torch.empty((), device=dev), torch.empty(M, device=dev)
    rows, count = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    nf, nb = L.amk_ce_head_bf16_fwd_ws_bytes(M, V, K), L.amk_ce_head_bf16_bwd_ws_bytes(M, V, K)
    ws = torch.empty(max(nf, nb) // 4 + 4, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    amk_lib.check(L.amk_ce_head_bf16_fwd(P(x), x.stride(0), P(w), w.stride(0), P(t), ignore_index, M, V, K, P(loss), P(lse),
                                         P(rows), P(count), P(ws), nf, st), "fwd")
    d = torch.tensor([d_loss], device=dev)
    amk_lib.check(L.amk_ce_head_bf16_bwd(P(x), x.stride(0), P(w), w.stride(0), P(t), ignore_index, M, V, K, P(d), P(lse),
                                         P(rows), P(count), P(dx), dx.stride(0), P(dw), dw.stride(0), P(ws), nb, st), "bwd")
    return loss, rows, count


def test_out_of_range_targets(device):
    """w is the first V rows of a 2 V-row buffer (and dw of one), so a wrong index would still land inside the
    allocation -- and show."""
    from amk import lib as amk_lib

    L = amk_lib.load()
    M, V, K = 300, 500, 64
    x, w2, t = _inputs("unit", M, 2 * V, K, "random64", device)
    w = w2[:V]
    t = torch.where(t >= 0, t % V, t)
    valid = (t >= 0).nonzero().flatten()
    bad = t.clone()
    bad[valid[3]], bad[valid[-1]], bad[valid[40]] = V, 2 * V - 1, -7
    SENT = 12345.0
    dx = torch.full((M, K), SENT, device=device, dtype=BF16)
    dw2 = torch.full((2 * V, K), SENT, device=device)
    loss, _, count = _raw(L, x, w, bad, -1, D_LOSS, dx, dw2[:V])
    dw = dw2[:V]
    assert bool((dw2[V:] == SENT).all())
    R = ref.reference(x, w, bad, -1, D_LOSS)
    assert bool(torch.isnan(loss)) and R["poisoned"] and int(count) == valid.numel()
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


def test_padded_layouts_and_compaction(device):
    """Padded ldx / ldw / lddx / lddw: nothing is written outside the views; rows and count are the valid indices; the
    layout changes no bit."""
    from amk import lib as amk_lib

    L = amk_lib.load()
    M, V, K = 129, 127, 40
    x, w, t = _inputs("unit", M, V, K, "random64", device)
    SENT = 12345.0
    xb = torch.full((M, K + 8), SENT, device=device, dtype=BF16)
    wb = torch.full((V, K + 16), SENT, device=device, dtype=BF16)
    xb[:, :K], wb[:, :K] = x, w
    dxb = torch.full((M, K + 24), SENT, device=device, dtype=BF16)
    dwb = torch.full((V, K + 8), SENT, device=device)
    loss, rows, count = _raw(L, xb[:, :K], wb[:, :K], t, -1, D_LOSS, dxb[:, :K], dwb[:, :K])
    assert bool((dxb[:, K:] == SENT).all()) and bool((dwb[:, K:] == SENT).all())
    valid = (t != -1).nonzero().flatten()
    assert int(count) == valid.numel() and torch.equal(rows[:valid.numel()].long(), valid) and bool((rows[valid.numel():] == -1).all())
    got = (loss, dxb[:, :K], dwb[:, :K])
    _hold(got, ref.reference(x, w, t, -1, D_LOSS), "padded")
    plain = _op(x, w, t)
    assert all(torch.equal(a, b.contiguous()) for a, b in zip(plain, got))      # the layout changes no bit


def test_run_to_run_bitwise(device):
    x, w, t = _inputs("peaked", 300, 1000, 264, "random64", device)
    a, b = _op(x, w, t), _op(x, w, t)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_graph_capture_with_changing_valid_counts(device):
    """Forward + backward captured once; replays with targets of different valid counts equal the eager results bitwise
    (the count never reaches the host).  Single stream."""
    from amk import ops
    from amk.graphs import GraphedStep

    M, V, K = 300, 1000, 64
    x, w, t0 = _inputs("unit", M, V, K, "random64", device)
    xg, wg = x.clone().requires_grad_(), w.float().requires_grad_()

    def fn(t):
        with torch.autocast("cuda", dtype=BF16):
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


# ---------------------------------------------------------------------------------------------- against the library path
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_accuracy_against_the_library_path(device, family):
    """F.linear + F.cross_entropy under autocast round every logit to bf16 (at most 2^-9 |z|) before the softmax; the
    rounding enters lse and z_t once each, so the two losses differ by at most 2^-8 mean_r max_v |z_rv| plus the fused
    head's own bound.  On `large` (bf16 ulp 16 at the logits' offset) the fused loss is inside its hard bound and the
    library's is not."""
    x, w, t = _inputs(family, 129, 1000, 264, "random64", device)
    R = ref.reference(x, w, t, -1, D_LOSS)
    fused = _op(x, w, t)[0].double()
    with torch.autocast("cuda", dtype=BF16):
        lib = F.cross_entropy(F.linear(x, w.float()), t, ignore_index=-1).double()
    cap = 2.0 ** -8 * R["zmax"] + float(R["bound_loss"])
    ef, el = abs(float(fused - R["loss"])), abs(float(lib - R["loss"]))
    print(f"{family}: fused off by {ef:.3e}, library by {el:.3e}, hard bound {float(R['bound_loss']):.3e}, |fused - lib| "
          f"{abs(float(fused - lib)):.3e} of the cap {cap:.3e}")
    assert abs(float(fused - lib)) <= cap
    if family == "large":
        assert ef <= float(R["bound_loss"]) < el


# ---------------------------------------------------------------------------------------------- models
def _step(model, call, monkeypatch, autocast, bf16_head=True):
    from amk import ops

    monkeypatch.setattr(ops, "CE_HEAD", True)
    monkeypatch.setattr(ops, "CE_HEAD_BF16", bf16_head)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    ops.KERNEL_EVENTS = {}
    try:
        if autocast:
            with torch.autocast("cuda", dtype=BF16):
                loss = call()
        else:
            loss = call()
        loss.float().backward()
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    return loss.detach().float(), grads, names


@pytest.mark.parametrize("which", ["muse", "maskgit"])
def test_model_switch_and_agreement_with_the_f32_step(device, monkeypatch, which):
    from test_ce_head_gpu import _small_models

    model, call = _small_models(device)[which]
    loss32, g32, k32 = _step(model, call, monkeypatch, autocast=False)
    loss16, g16, k16 = _step(model, call, monkeypatch, autocast=True)
    _, _, koff = _step(model, call, monkeypatch, autocast=True, bf16_head=False)
    assert sum(n.startswith("ce_head_fwd") for n in k32) == 1 and not any(n.startswith("bf16_ce_head") for n in k32)
    assert sum(n.startswith("bf16_ce_head_fwd") for n in k16) == 1 and sum(n.startswith("bf16_ce_head_bwd") for n in k16) == 1
    assert not any(n.startswith("ce_head") for n in k16)
    assert not any(n.startswith("bf16_ce_head") or n.startswith("ce_head") for n in koff)
    # the same seed, so the same mask: bf16 against f32 at the tolerances of tests/test_autocast_gpu.py
    assert abs(float(loss16 - loss32)) <= 3e-2 * abs(float(loss32)), (float(loss16), float(loss32))
    assert set(g16) == set(g32) and len(g32) > 10
    for n in g32:
        err = float((g16[n].float() - g32[n]).abs().max())
        assert err <= 6e-2 * float(g32[n].abs().max()) + 1e-6, f"grad {n}: {err:.3e} against max {float(g32[n].abs().max()):.3e}"


@pytest.mark.parametrize("capturable", [False, True])
def test_train_step_uses_the_shadow_and_the_reducers_bucket(device, monkeypatch, capturable):
    """MaskedTokenTrainStep(autocast=bfloat16) on a small MUSE: the head reads the optimizer's bf16 shadow of
    decoder.linear.weight, writes that weight's gradient into the reducer's bucket, and the loss is finite."""
    from amk import ops
    from amk.models import MUSE, ViTVQGAN
    from amk.train import MaskedTokenTrainStep

    monkeypatch.setattr(ops, "CE_HEAD", True)
    monkeypatch.setattr(ops, "CE_HEAD_BF16", True)
    torch.manual_seed(0)
    vq = ViTVQGAN(dict(dim=64, img_size=32, patch_size=8, n_heads=1, d_head=64, depth=1, mlp_dim=64, dropout=0.0),
                  dict(codebook_size=64, codebook_dim=32))
    model = MUSE(dim=64, vq=vq, text_dim=24, n_heads=1, d_head=64, depth=2, mult=4).to(device)
    ts = MaskedTokenTrainStep(model, lr=1e-3, warmup_steps=1, autocast=BF16, capturable=capturable, bucket_bytes=128 << 10)
    if not ts.red.direct_grads:
        pytest.skip("AMK_DIRECT_GRADS=0 in the environment")
    p = model.decoder.linear.weight
    assert ops._w16(p) is p._amk_bf16
    text, imgs = torch.randn(3, 7, 24, device=device), torch.rand(3, 3, 32, 32, device=device)
    ops.KERNEL_EVENTS = {}
    try:
        if capturable:
            ts.capture(text, imgs, warmup=1)
        loss = ts.step(text, imgs)
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    assert any(n.startswith("bf16_ce_head_bwd") for n in names)
    assert bool(torch.isfinite(loss))
    bucket, i = ts.red._bucket_of[p]
    assert bucket.direct[i], "the head's weight gradient did not go into the reducer's bucket"
    assert p.grad is not None and p.grad.data_ptr() == bucket.views[i].data_ptr()
    assert ops._w16(p) is p._amk_bf16       # the update refreshed the shadow: still current


def test_zz_report_worst_ratios(capsys):
    with capsys.disabled():
        print("\nbf16 ce_head worst (hard ratio, q / (4 Q_EMU)):", {k: (round(a, 4), round(b, 4)) for k, (a, b) in WORST.items()})
    assert not WORST or set(WORST) == set(NAMES)
