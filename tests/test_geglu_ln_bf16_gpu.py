"""csrc/geglu_ln_bf16.hip and ops.geglu_ffn on the MI355X: the two fused kernels against the fp64 reference and per-element
bounds of tests/geglu_ln_bf16_ref.py at every width the dispatch distinguishes (512 / 1024 / 2048 / 4096 and their
neighbours, plus the 256 / 264 pair of the f32 LayerNorm's dispatch), what a tolerance cannot see (bitwise properties,
strided views, refusals), the op's dispatch, the block's accuracy against the path before, and the op inside the models.

AMK_GEGLU_LN_BOUND_REPORT=<file>: write the worst |got - ref| / bound per tensor over this module to that JSON file."""
import copy
import ctypes
import json
import os

import pytest
import torch

import geglu_ln_bf16_ref as ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
AMK_OK, AMK_EINVAL, AMK_EUNSUPPORTED = 0, -1, -2
WIDTHS = [8, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4096]
ROWS = [1, 3, 4, 5, 67]
SENTINEL = 1.5        # bf16-exact


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AMK_GEGLU_LN_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(ref.WORST, f, indent=1, sort_keys=True)


_CACHE = {}


def _case(family, M, H):
    """((ab, dy, gamma, beta) on the CPU, reference): computed once per shape, never modified."""
    key = (family, M, H)
    if key not in _CACHE:
        inp = ref.make_inputs(family, M, H)
        _CACHE[key] = (inp, ref.reference(*inp))
    return _CACHE[key]


def _run(inp, device):
    """The two kernels through ops' thin wrappers over the C ABI."""
    from amk import ops

    ab, dy, gamma, beta = (t.to(device) for t in inp)
    y, mean, rstd = ops.geglu_ln_bf16_fwd(ab, gamma, beta, ref.EPS)
    d_ab, part = ops.geglu_ln_bf16_bwd(ab, dy, gamma, mean, rstd)
    dgb = part.sum(0)
    return {"y": y, "mean": mean, "rstd": rstd, "d_ab": d_ab, "dgamma": dgb[0], "dbeta": dgb[1]}


def _check(got, R, tag):
    q = ref.ratios({k: v.cpu() for k, v in got.items()}, R, names=[n for n in ref.TENSORS if n in got])
    print(tag, {k: round(v, 4) for k, v in q.items()})
    for name, v in q.items():
        assert v <= 1.0, f"{tag}: {name} at {v:.3f} of its bound"


# ---------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("H", WIDTHS)
def test_kernels_within_bounds_at_every_width(device, H):
    for M in ROWS:
        inp, R = _case("diffuse", M, H)
        _check(_run(inp, device), R, f"diffuse M{M} H{H}")


@pytest.mark.parametrize("M,H", [(67, 264), (5, 4096)])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_kernels_within_bounds_on_every_family(device, family, M, H):
    inp, R = _case(family, M, H)
    got = _run(inp, device)
    _check(got, R, f"{family} M{M} H{H}")
    assert all(bool(torch.isfinite(v.float()).all()) for v in got.values())
    for r in ref.zero_rows(family, M):
        assert torch.equal(got["y"][r].cpu(), inp[3].to(BF16)), f"row {r}: y is not bf16(beta)"


@pytest.mark.parametrize("M", [70001, 2051])
def test_row_loop_beyond_one_grid(device, M):
    """H = 8: four rows per workgroup; the forward's grid ends at 2048 workgroups (8192 rows), the backward's at 512
    (2048 rows = 4 x num_partials)."""
    from amk import lib

    assert lib.load().amk_geglu_ln_bf16_num_partials(M, 8) == 512 and M > 4 * 512
    inp, R = _case("diffuse", M, 8)
    _check(_run(inp, device), R, f"diffuse M{M} H8")


@pytest.mark.parametrize("family,M,H", [("diffuse", 67, 264), ("wide", 5, 1032), ("large", 3, 2056), ("diffuse", 5, 4096)])
def test_autograd_function_within_bounds(device, monkeypatch, family, M, H):
    """_GEGLUFFNMixed with dim = 2H, w1 = I and w2 = (I | 0)^T: x = ab passes through w1 exactly, y through w2 into the
    first H output columns, so the Function's output and gradients are the kernels' y, d_ab, dgamma and dbeta."""
    from amk import ops

    monkeypatch.setattr(ops, "GEGLU_FFN_BF16", True)
    (ab, dy, gamma, beta), R = _case(family, M, H)
    x = ab.to(device).requires_grad_(True)
    w1 = torch.eye(2 * H, device=device).requires_grad_(True)
    w2 = torch.eye(2 * H, H, device=device).requires_grad_(True)
    gm, bt = gamma.to(device).requires_grad_(True), beta.to(device).requires_grad_(True)
    ops.KERNEL_EVENTS = {}
    try:
        with torch.autocast("cuda", dtype=BF16):
            assert ops.geglu_ffn_ok(x, w1, gm, bt, w2)
            out = ops.geglu_ffn(x, w1, gm, bt, w2, ref.EPS)
        out.backward(torch.cat([dy, torch.zeros_like(dy)], dim=1).to(device))
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    assert names == [f"geglu_ln_bf16_fwd M{M} H{H}", f"geglu_ln_bf16_bwd M{M} H{H}"]
    assert out.dtype == BF16 and x.grad.dtype == BF16 and gm.grad.dtype == torch.float32
    assert not bool(out[:, H:].any())
    _check({"y": out.detach()[:, :H], "d_ab": x.grad, "dgamma": gm.grad, "dbeta": bt.grad}, R, f"autograd {family} M{M} H{H}")


# ---------------------------------------------------------------------------------------------- what a tolerance cannot see
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("H", [264, 1032, 4096])
def test_run_to_run_bitwise(device, H):
    inp, _ = _case("diffuse", 67, H)
    a, b = _run(inp, device), _run(inp, device)
    assert _same(a, b)
    big, _ = _case("diffuse", 2051, 8)
    assert _same(_run(big, device), _run(big, device))


@pytest.mark.parametrize("H", [264, 1032, 2056, 4096])
def test_a_row_alone_equals_the_row_in_a_batch(device, H):
    inp, _ = _case("diffuse", 67, H)
    full = _run(inp, device)
    ab, dy, gamma, beta = inp
    for r in (0, 5, 66):
        one = _run((ab[r:r + 1].contiguous(), dy[r:r + 1].contiguous(), gamma, beta), device)
        for name in ("y", "mean", "rstd", "d_ab"):
            assert torch.equal(one[name][0], full[name][r]), (name, r)


@pytest.mark.parametrize("M,H", [(67, 264), (5, 4096)])
def test_strided_ab_and_untouched_surroundings(device, M, H):
    from amk import lib, ops

    inp, _ = _case("diffuse", M, H)
    ab, dy, gamma, beta = (t.to(device) for t in inp)
    want = _run(inp, device)
    L = lib.load()
    stride = 2 * H + 24
    wide = torch.full((M + 2, stride), SENTINEL, device=device, dtype=BF16)
    view = wide[1:M + 1, 8:8 + 2 * H]
    view.copy_(ab)
    assert view.stride(0) == stride and view.data_ptr() % 16 == 0
    nparts = L.amk_geglu_ln_bf16_num_partials(M, H)
    # every output inside a sentinel-filled buffer with a margin of one row in front and behind
    y = torch.full((M + 2, H), SENTINEL, device=device, dtype=BF16)
    mean = torch.full((M + 8,), SENTINEL, device=device)
    rstd = torch.full((M + 8,), SENTINEL, device=device)
    d_ab = torch.full((M + 2, 2 * H), SENTINEL, device=device, dtype=BF16)
    part = torch.full((nparts + 2, 2, H), SENTINEL, device=device)
    P = ops._ptr
    rc = L.amk_geglu_ln_bf16_fwd(P(view), stride, M, H, P(gamma), P(beta), ref.EPS, P(y[1:]), P(mean[4:]), P(rstd[4:]), ops._stream())
    assert rc == AMK_OK
    rc = L.amk_geglu_ln_bf16_bwd(P(view), stride, P(dy), P(gamma), P(mean[4:]), P(rstd[4:]), M, H, P(d_ab[1:]), P(part[1:]), ops._stream())
    assert rc == AMK_OK
    assert torch.equal(y[1:M + 1], want["y"]) and torch.equal(d_ab[1:M + 1], want["d_ab"])
    assert torch.equal(mean[4:M + 4], want["mean"]) and torch.equal(rstd[4:M + 4], want["rstd"])
    dgb = part[1:nparts + 1].sum(0)
    assert torch.equal(dgb[0], want["dgamma"]) and torch.equal(dgb[1], want["dbeta"])
    for t, lo, hi in ((y, 1, M + 1), (d_ab, 1, M + 1), (mean, 4, M + 4), (rstd, 4, M + 4), (part, 1, nparts + 1)):
        assert bool((t[:lo] == SENTINEL).all()) and bool((t[hi:] == SENTINEL).all())
    keep = wide.clone()
    keep[1:M + 1, 8:8 + 2 * H] = SENTINEL
    assert bool((keep == SENTINEL).all())            # the input's surroundings were not written either


@pytest.mark.parametrize("what,code", [("H12", AMK_EUNSUPPORTED), ("H4104", AMK_EUNSUPPORTED), ("stride", AMK_EINVAL),
                                       ("misaligned", AMK_EINVAL), ("M0", AMK_EINVAL)])
def test_refusals_launch_nothing(device, what, code):
    """Every buffer is large enough for the arguments given (M = 4 rows of up to 4104 columns, stride up to 2 H + 4)."""
    from amk import lib, ops

    L = lib.load()
    M, H = 4, 264
    HB = 4104
    ab = torch.full((M + 1, 2 * HB + 8), SENTINEL, device=device, dtype=BF16)
    dy = torch.full((M + 1, HB), SENTINEL, device=device, dtype=BF16)
    gamma = torch.full((HB + 8,), SENTINEL, device=device)
    beta = torch.full((HB + 8,), SENTINEL, device=device)
    outs = dict(y=torch.full((M + 1, HB), SENTINEL, device=device, dtype=BF16), mean=torch.full((M + 8,), SENTINEL, device=device),
                rstd=torch.full((M + 8,), SENTINEL, device=device), d_ab=torch.full((M + 1, 2 * HB), SENTINEL, device=device, dtype=BF16),
                part=torch.full((M + 1, 2, HB), SENTINEL, device=device))
    stride, abp = 2 * H, ab.data_ptr()
    if what == "H12":
        H, stride = 12, 24
    elif what == "H4104":
        H, stride = 4104, 2 * 4104
    elif what == "stride":
        stride = 2 * H + 4
    elif what == "misaligned":
        abp += 2
    elif what == "M0":
        M = 0
    V = ctypes.c_void_p
    P = ops._ptr
    rc = L.amk_geglu_ln_bf16_fwd(V(abp), stride, M, H, P(gamma), P(beta), ref.EPS, P(outs["y"]), P(outs["mean"]), P(outs["rstd"]),
                                 ops._stream())
    assert rc == code and "amk_geglu_ln_bf16_fwd" in L.amk_last_error().decode()
    rc = L.amk_geglu_ln_bf16_bwd(V(abp), stride, P(dy), P(gamma), P(outs["mean"]), P(outs["rstd"]), M, H, P(outs["d_ab"]),
                                 P(outs["part"]), ops._stream())
    assert rc == code and "amk_geglu_ln_bf16_bwd" in L.amk_last_error().decode()
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert bool((t == SENTINEL).all()), name
    assert L.amk_geglu_ln_bf16_num_partials(0, 264) == 0


# ---------------------------------------------------------------------------------------------- op and dispatch
def _ff_step(ff, x, autocast=True, spy=None):
    """(out, {name: grad}, event names) of one forward + backward of a FeedForward."""
    from amk import ops

    ff.zero_grad(set_to_none=True)
    xi = x.detach().clone().requires_grad_(True)
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(x.device)
    ops.KERNEL_EVENTS = {}
    try:
        with torch.autocast("cuda", dtype=BF16, enabled=autocast):
            out = ff(xi)
        if out.requires_grad:
            (out.float() * cot).sum().backward()
        torch.cuda.synchronize()
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    grads = {n: p.grad for n, p in ff.named_parameters()}
    grads["x"] = xi.grad
    return out.detach(), grads, names


def _fused(names):
    return [n for n in names if n.startswith("geglu_ln_bf16")]


@pytest.mark.parametrize("dim,mult,inner", [(64, 3, 128), (1024, 6, 4096)])
@pytest.mark.parametrize("xdtype", [torch.float32, BF16])
def test_feed_forward_runs_the_fused_kernels(device, monkeypatch, dim, mult, inner, xdtype):
    from amk import lib, ops
    from amk.models import transformer

    monkeypatch.setattr(ops, "GEGLU_FFN_BF16", True)
    L = lib.load()
    calls = []
    for sym in ("amk_geglu_fwd", "amk_geglu_bwd", "amk_add_layernorm_fwd", "amk_add_layernorm_bwd"):
        real = getattr(L, sym)
        monkeypatch.setattr(L, sym, lambda *a, _r=real, _s=sym: (calls.append(_s), _r(*a))[1])
    torch.manual_seed(0)
    ff = transformer.FeedForward(dim, mult=mult).to(device)
    assert ff.ff[3].weight.shape[1] == inner
    assert list(ff.state_dict()) == ["ff.0.weight", "ff.2.gamma", "ff.2.beta", "ff.3.weight"]
    x = torch.randn(2, 65, dim, device=device).to(xdtype)
    out, g, names = _ff_step(ff, x)
    assert names == [f"geglu_ln_bf16_fwd M130 H{inner}", f"geglu_ln_bf16_bwd M130 H{inner}"], names
    assert not calls, calls
    assert out.dtype == BF16 and out.shape == x.shape
    assert g["ff.0.weight"].dtype == g["ff.3.weight"].dtype == g["ff.2.gamma"].dtype == torch.float32
    assert g["ff.0.weight"].shape == ff.ff[0].weight.shape and g["ff.2.gamma"].shape == (inner,)
    assert ff.ff[2].beta.grad is None and "ff.2.beta" not in g
    assert g["x"].dtype == xdtype and g["x"].shape == x.shape
    assert all(bool(torch.isfinite(v.float()).all()) for v in g.values())
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):     # the generate loops: same forward, nothing saved
        ops.KERNEL_EVENTS = {}
        try:
            out2 = ff(x)
            names2 = list(ops.KERNEL_EVENTS)
        finally:
            ops.KERNEL_EVENTS = None
    assert names2 == [f"geglu_ln_bf16_fwd M130 H{inner}"] and torch.equal(out2, out)


@pytest.mark.parametrize("case", ["switch_off", "no_autocast", "inner170", "inner0", "w2_frozen"])
def test_dispatch_keeps_todays_path(device, monkeypatch, case):
    from amk import ops
    from amk.models import transformer

    monkeypatch.setattr(ops, "GEGLU_FFN_BF16", case != "switch_off")
    torch.manual_seed(0)
    dim, mult = {"inner170": (128, 2), "inner0": (1024, 0.0)}.get(case, (64, 3))
    ff = transformer.FeedForward(dim, mult=mult).to(device)
    assert ff.ff[3].weight.shape[1] == {"inner170": 170, "inner0": 0}.get(case, 128)
    if case == "w2_frozen":
        ff.ff[3].weight.requires_grad_(False)
    x = torch.randn(2, 65, dim, device=device)
    autocast = case != "no_autocast"
    out, g, names = _ff_step(ff, x, autocast)
    assert not _fused(names), names
    chain = copy.deepcopy(ff)
    chain.forward = chain.ff.forward                 # the Sequential run directly
    out0, g0, _ = _ff_step(chain, x, autocast)
    assert out.dtype == out0.dtype and torch.equal(out, out0)
    for n in g0:
        assert (g[n] is None and g0[n] is None) or torch.equal(g[n], g0[n]), n


def test_block_accuracy_against_the_path_before(device, monkeypatch):
    """FeedForward(256, mult=3) (inner 512), M = 200: both paths against the same module in fp64.  Both round the GEMM
    operands identically and the fused one rounds strictly fewer intermediates, so its error may exceed the old one's only
    by coincidences of rounding: at most 1.5 x + 1e-6 on every output."""
    from amk import ops
    from amk.models import transformer

    torch.manual_seed(0)
    ff = transformer.FeedForward(256, mult=3).to(device)
    with torch.no_grad():
        ff.ff[2].gamma.copy_(0.5 + torch.rand(512))
    x = torch.randn(200, 256, device=device)
    ff64 = copy.deepcopy(ff).double().cpu()
    o64, g64, _ = _ff_step(ff64, x.double().cpu(), autocast=False)
    errs = {}
    for tag, on in (("fused", True), ("before", False)):
        monkeypatch.setattr(ops, "GEGLU_FFN_BF16", on)
        out, g, names = _ff_step(ff, x)
        assert bool(_fused(names)) == on
        got = {"out": out, "dx": g["x"], "dW1": g["ff.0.weight"], "dW2": g["ff.3.weight"], "dgamma": g["ff.2.gamma"]}
        want = {"out": o64, "dx": g64["x"], "dW1": g64["ff.0.weight"], "dW2": g64["ff.3.weight"], "dgamma": g64["ff.2.gamma"]}
        errs[tag] = {k: float((got[k].double().cpu() - want[k]).abs().max() / want[k].abs().max()) for k in got}
    print("max-normalised error against fp64:", errs)
    for k in errs["fused"]:
        assert errs["fused"][k] <= 1.5 * errs["before"][k] + 1e-6, (k, errs["fused"][k], errs["before"][k])


def test_op_reads_the_bf16_shadow(device, monkeypatch):
    """After one FlatAdam(bf16_shadow=True) step the op reads ff.0.weight._amk_bf16 / ff.3.weight._amk_bf16; after an
    in-place write it falls back to a cast."""
    from amk import ops
    from amk.dp import GradReducer
    from amk.models import transformer
    from amk.optim import FlatAdam

    monkeypatch.setattr(ops, "GEGLU_FFN_BF16", True)
    torch.manual_seed(0)
    ff = transformer.FeedForward(64, mult=3).to(device)
    red = GradReducer(ff.parameters(), bucket_bytes=64 << 10)
    opt = FlatAdam(red, lr=1e-3, bf16_shadow=True)
    x = torch.randn(2, 65, 64, device=device)
    red.begin(True)
    with torch.autocast("cuda", dtype=BF16):
        out = ff(x)
    out.float().pow(2).mean().backward()
    red.finish(detach_unused=False)
    opt.step(max_norm=1.0)
    w1, w2 = ff.ff[0].weight, ff.ff[3].weight
    assert ops._w16(w1) is w1._amk_bf16 and ops._w16(w2) is w2._amk_bf16

    def seen_by_the_op():
        seen = {}
        real = ops._w16

        def spy(t):
            r = real(t)
            seen[id(t)] = r
            return r
        monkeypatch.setattr(ops, "_w16", spy)
        try:
            with torch.autocast("cuda", dtype=BF16):
                o = ff(x)
            o.float().sum().backward()
        finally:
            monkeypatch.setattr(ops, "_w16", real)
        assert bool(torch.isfinite(o.float()).all())
        return seen[id(w1)], seen[id(w2)]

    a, b = seen_by_the_op()
    assert a is w1._amk_bf16 and b is w2._amk_bf16
    with torch.no_grad():
        w1.mul_(1.5)
        w2.mul_(0.5)
    a, b = seen_by_the_op()
    assert a is not w1._amk_bf16 and torch.equal(a, w1.detach().to(BF16))
    assert b is not w2._amk_bf16 and torch.equal(b, w2.detach().to(BF16))


# ---------------------------------------------------------------------------------------------- in the models
def test_decoder_with_the_switch_on_and_off(device, monkeypatch):
    """BidirectionalDecoder (inner 256, depth 2) under bf16 autocast with the switch on and off: both stay within the
    distance of the f32 pass that tests/test_autocast_gpu.py allows (3e-2 of max for the logits, 6e-2 for gradients)."""
    from amk import ops
    from amk.models.muse import BidirectionalDecoder

    torch.manual_seed(0)
    dec = BidirectionalDecoder(dim=128, codebook_size=64, n_heads=2, d_head=64, depth=2, mult=3, dropout=0.0, num_patches=96).to(device)
    assert dec.decoder.layers[0].feed_forward.ff[3].weight.shape[1] == 256
    ids = torch.randint(0, 65, (3, 96), device=device)
    ctx = torch.randn(3, 20, 128, device=device)
    cot = torch.randn(3, 96, 64, device=device)
    params = [p for p in dec.parameters() if p.requires_grad]
    out32 = dec(ids, context=ctx)
    g32 = torch.autograd.grad((out32 * cot).sum(), params, allow_unused=True)
    for on in (True, False):
        monkeypatch.setattr(ops, "GEGLU_FFN_BF16", on)
        ops.KERNEL_EVENTS = {}
        try:
            with torch.autocast("cuda", dtype=BF16):
                out16 = dec(ids, context=ctx)
            g16 = torch.autograd.grad((out16.float() * cot).sum(), params, allow_unused=True)
            torch.cuda.synchronize()
            ev = {k: len(v) for k, v in ops.KERNEL_EVENTS.items()}
        finally:
            ops.KERNEL_EVENTS = None
        if on:
            assert ev.get("geglu_ln_bf16_fwd M288 H256") == 2 and ev.get("geglu_ln_bf16_bwd M288 H256") == 2, ev
        else:
            assert not _fused(ev), ev
        err = float((out16.detach().float() - out32.detach()).abs().max() / out32.detach().abs().max())
        assert err < 3e-2, (on, err)
        for a, b in zip(g16, g32):
            if b is not None:
                assert a is not None and bool(torch.isfinite(a).all())
                assert float((a.float() - b).abs().max()) <= 6e-2 * float(b.abs().max()) + 1e-6, on


@pytest.mark.timeout(600)
def test_captured_masked_token_step_replays_like_eager(device, monkeypatch):
    """MaskedTokenTrainStep on a small MUSE with autocast=bfloat16, capturable=True and the fused FFN: three captured
    steps equal three eager steps to the bit (parameters and losses); an eager step runs the fused kernels once per layer."""
    from amk import ops
    from amk.models import MUSE, ViTVQGAN
    from amk.train import MaskedTokenTrainStep

    monkeypatch.setattr(ops, "GEGLU_FFN_BF16", True)
    monkeypatch.setattr(ops, "DETERMINISTIC_ATTENTION_BACKWARD", True)
    torch.manual_seed(0)
    vq = ViTVQGAN(dict(dim=64, img_size=32, patch_size=8, n_heads=1, d_head=64, depth=1, mlp_dim=64, dropout=0.0),
                  dict(codebook_size=64, codebook_dim=32))
    base = MUSE(dim=64, vq=vq, text_dim=24, n_heads=1, d_head=64, depth=2, mult=3).to(device)
    g = torch.Generator().manual_seed(5)
    text, imgs = torch.randn(3, 7, 24, generator=g).to(device), torch.rand(3, 3, 32, 32, generator=g).to(device)
    runs = []
    for graphed in (False, True):
        model = copy.deepcopy(base)
        ts = MaskedTokenTrainStep(model, lr=1e-3, warmup_steps=1, autocast=BF16, capturable=True, bucket_bytes=128 << 10)
        torch.manual_seed(11)
        if graphed:
            ts.capture(text, imgs, warmup=2)
        else:
            ops.KERNEL_EVENTS = {}
            try:
                ts.step(text, imgs)
                torch.cuda.synchronize()
                ev = {k: len(v) for k, v in ops.KERNEL_EVENTS.items()}
            finally:
                ops.KERNEL_EVENTS = None
            assert ev.get("geglu_ln_bf16_fwd M48 H128") == 2 and ev.get("geglu_ln_bf16_bwd M48 H128") == 2, ev
            ts.step(text, imgs)
        losses = []
        for i in range(3):
            torch.manual_seed(100 + i)           # the same masks in both runs, whatever the warm-up drew
            losses.append(ts.step(text, imgs).clone())
        if graphed:
            assert ts._graph is not None
        torch.cuda.synchronize()
        runs.append((losses, [p.detach().clone() for p in model.parameters()], ts.global_step))
    (l0, p0, s0), (l1, p1, s1) = runs
    assert s0 == s1 == 5
    assert all(bool(torch.isfinite(v)) for v in l0)
    for a, b in zip(l0, l1):
        assert torch.equal(a, b), (l0, l1)
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)


def test_zz_report_worst_ratios(capsys):
    with capsys.disabled():
        print("\ngeglu_ln_bf16 worst |got - ref| / bound:", {k: round(v, 4) for k, v in sorted(ref.WORST.items())})
    assert all(v <= 1.0 for v in ref.WORST.values())
