"""The bf16 grouped expert GEMMs of csrc/moe_bf16.hip and ops._RoutedLinearBF16 on the MI355X.

C ABI: each of the three entry points writes into a NaN canvas with guard rows; the guards and the rows no list names
must stay untouched, and every named element is held to the two tiers of tests/moe_bf16_ref.py (hard bound; for nt and
nn also 4 x the CPU emulation's q) against fp64 references on the bf16 values, over the case list of that file: counts
one below, at and one above the pair tile (64) and the weight gradient's pair step (32), widths one below, at and one
above the column tile (256), the weight gradient's tile (128) and the contraction step (32), empty experts, sparse and
skewed lists, padded strides, NULL bias / scale / dbias.  The host code has one kernel per entry point and never reads
the device's size, so there is no dispatch to cover beyond that list (test_case_list_covers_the_kernels).  All three
results repeat bit for bit, and a pair's nt / nn row does not depend on its position inside its expert.
Op level: ops.routed_linear as MoELayer calls it under bf16 autocast against the composed bounds, the dispatch back to
_RoutedLinear, the optimizer's bf16 shadow, and a captured train step of the reduced ViTMoE equal to the eager one.
AMK_MOE_BF16_BOUNDS_REPORT=<file>: the worst hard ratio and q / limit per kernel as JSON."""
import copy
import ctypes
import json
import os

import pytest
import torch

import moe_bf16_ref as ref
import moe_ref as mref
from test_moe_bf16_bounds import _inputs

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
GUARD = 3
SMALL_MOE = dict(dim=128, image_size=64, patch_size=16, n_heads=2, d_head=64, depth=2, n_experts=4, sel_experts=2,
                 dropout=0.0, num_classes=10)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nkernel: worst hard ratio, worst q / limit")
    for key, (ratio, q) in sorted(ref.WORST.items()):
        print(f"  {key:12s} {ratio:.4f}  {'-' if q is None else format(q, '.4f')}")
    path = os.environ.get("AMK_MOE_BF16_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(ref.WORST, f, indent=1)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def canvas(rows, width, dev):
    whole = torch.full((rows + 2 * GUARD, width), float("nan"), device=dev, dtype=torch.float32)
    return whole, whole[GUARD:GUARD + rows]


def guards_untouched(whole, rows):
    return bool(torch.isnan(torch.cat([whole[:GUARD], whole[GUARD + rows:]])).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _lib():
    from amk import lib as L_

    return L_, L_.load()


def run_grouped(kind, D, off, perm, P, E, N, Kd, a_div, vec):
    """One launch of amk_grouped_gemm_{nt,nn}_bf16 into a NaN canvas: (whole, inner)."""
    L_, L = _lib()
    src = D["A"] if kind == "nt" else D["Gm"]
    whole, Y = canvas(P, N if kind == "nt" else Kd, src.device)
    fn = L.amk_grouped_gemm_nt_bf16 if kind == "nt" else L.amk_grouped_gemm_nn_bf16
    L_.check(fn(_ptr(src), src.stride(0), a_div, _ptr(D["W"]), _ptr(vec), _ptr(off), _ptr(perm), P, E, N, Kd, _ptr(Y), _stream()),
             f"amk_grouped_gemm_{kind}_bf16")
    return whole, Y


def run_wgrad(D, off, perm, P, E, N, Kd, g_div, x_div, scale, want_db):
    L_, L = _lib()
    dev = D["Gm"].device
    wW, dW = canvas(E * N, Kd, dev)
    wb, db = canvas(E, N, dev)
    L_.check(L.amk_grouped_gemm_wgrad_bf16(_ptr(D["Gm"]), D["Gm"].stride(0), g_div, _ptr(D["X"]), D["X"].stride(0), x_div, _ptr(scale),
                                           _ptr(off), _ptr(perm), P, E, N, Kd, _ptr(dW), _ptr(db) if want_db else None, _stream()),
             "amk_grouped_gemm_wgrad_bf16")
    return wW, dW, wb, db


def _device_case(c, dev):
    D, (ids, off, perm), P = _inputs(c)
    return {k: v.to(dev) for k, v in D.items()}, off.to(dev), perm.to(dev), P


def test_case_list_covers_the_kernels(device):
    """Every edge and branch inside the three kernels is reached by the case list.  The host code of csrc/moe_bf16.hip
    picks no kernel by the device's CU count (one kernel per entry point, grids sized from the lists alone)."""
    missing = ref.missing_coverage()
    assert not missing, f"the case list does not reach: {sorted(missing)}"
    assert torch.cuda.get_device_properties(0).multi_processor_count > 0


@pytest.mark.parametrize("c", ref.CASES, ids=lambda c: c["id"])
def test_grouped_gemms(device, c):
    dev = device
    E, N, Kd, a_div, x_div = c["E"], c["N"], c["Kd"], c["a_div"], c["x_div"]
    D, off, perm, P = _device_case(c, dev)
    counts = (off[1:] - off[:-1]).tolist()
    for kind in ("nt", "nn"):
        vec = None if c["nulls"] else (D["bias"] if kind == "nt" else D["scale"])
        src = D["A"] if kind == "nt" else D["Gm"]
        whole, Y = run_grouped(kind, D, off, perm, P, E, N, Kd, a_div, vec)
        R = (ref.ref_nt if kind == "nt" else ref.ref_nn)(src, src.stride(0), a_div, D["W"], vec, off, perm, P, E, N, Kd)
        ref.assert_within(Y, R, "y", kind, f"{c['id']} {kind}")
        assert guards_untouched(whole, P), f"{c['id']} {kind}: a guard row was written"
        assert bool(torch.isnan(Y[~R["named_y"]]).all()), f"{c['id']} {kind}: a row the lists do not name was written"
        _, Y2 = run_grouped(kind, D, off, perm, P, E, N, Kd, a_div, vec)
        assert same_bits(Y, Y2), f"{c['id']} {kind}: two calls differ"
    empty = torch.tensor(counts, device=dev) == 0
    for use_scale in ((False,) if c["nulls"] else (True, False)):
        name = "wgrad" if use_scale else "wgrad_noscale"
        scale = D["scale"] if use_scale else None
        want_db = not (c["nulls"] or (c["pad"] and not use_scale))          # NULL dbias: with nulls, and once more
        wW, dW, wb, db = run_wgrad(D, off, perm, P, E, N, Kd, a_div, x_div, scale, want_db)
        R = ref.ref_wgrad(D["Gm"], D["Gm"].stride(0), a_div, D["X"], D["X"].stride(0), x_div, scale, off, perm, P, E, N, Kd)
        ref.assert_within(dW.view(E, N, Kd), R, "dw", "dw", f"{c['id']} {name}")
        assert guards_untouched(wW, E * N) and guards_untouched(wb, E), f"{c['id']} {name}: a guard row was written"
        assert bool((dW.view(E, N, Kd)[empty] == 0).all()), f"{c['id']} {name}: an expert without pairs is not exactly zero"
        _, dW2, _, db2 = run_wgrad(D, off, perm, P, E, N, Kd, a_div, x_div, scale, want_db)
        assert same_bits(dW, dW2), f"{c['id']} {name}: two calls differ in dW"
        if want_db:
            ref.assert_within(db, R, "db", "db", f"{c['id']} {name}")
            assert bool((db[empty] == 0).all()) and same_bits(db, db2), f"{c['id']} {name}: dbias of an empty expert / two calls"
        else:
            assert bool(torch.isnan(db).all()), f"{c['id']} {name}: dbias written although null was passed"


@pytest.mark.parametrize("N,Kd", [(136, 128), (64, 72), (128, 264), (264, 136)])
def test_position_free(device, N, Kd):
    """The rows of the pairs that two lists share (same expert, another position, another tile) are equal bit for bit."""
    ids, off, perm = ref.make_lists(ref.EDGE, seed=5)
    P, E = ids.numel(), len(ref.EDGE)
    keep = torch.rand(P, generator=torch.Generator().manual_seed(6)) < 0.7
    cnt2 = torch.bincount(ids[keep], minlength=E)
    off2 = torch.zeros(E + 1, dtype=torch.int32)
    off2[1:] = torch.cumsum(cnt2, 0)
    rows = torch.nonzero(keep).view(-1)
    perm2 = rows[torch.sort(ids[rows], stable=True)[1]].int()
    D = {k: v.to(device) for k, v in ref.make_data("binade", P, E, N, Kd, 2, 2, 9).items()}
    for kind in ("nt", "nn"):
        vec = D["bias"] if kind == "nt" else D["scale"]
        _, Y1 = run_grouped(kind, D, off.to(device), perm.to(device), P, E, N, Kd, 2, vec)
        _, Y2 = run_grouped(kind, D, off2.to(device), perm2.to(device), P, E, N, Kd, 2, vec)
        kd = keep.to(device)
        assert bool(torch.isnan(Y2[~kd]).all()) and not bool(torch.isnan(Y2[kd]).any())
        assert same_bits(Y1[kd], Y2[kd]), f"{kind} N{N} K{Kd}: a row depends on its position"


@pytest.mark.parametrize("what", ["N12", "Kd20", "misaligned", "stride68"])
def test_refusals(device, what):
    """The documented code and the library's message, before any device work: the canvas stays untouched."""
    L_, L = _lib()
    EINVAL, EUNSUPPORTED = -1, -2
    E, P = 3, 40
    N, Kd = (12 if what == "N12" else 64), (20 if what == "Kd20" else 64)
    ids, off, perm = ref.make_lists([10, 14, 16], seed=1)
    off, perm = off.to(device), perm.to(device)
    lda = 68 if what == "stride68" else 72
    buf = torch.zeros(P * 72 + 8, device=device, dtype=BF16)
    A = buf[1:] if what == "misaligned" else buf
    W = torch.zeros(E, N, Kd, device=device, dtype=BF16)
    scale = torch.ones(P, device=device)
    want = EUNSUPPORTED if what in ("N12", "Kd20") else EINVAL
    text = {"N12": "must be multiples of 8", "Kd20": "must be multiples of 8", "misaligned": "16-byte aligned", "stride68": "row stride 68"}[what]
    calls = {
        "amk_grouped_gemm_nt_bf16": lambda Y: L.amk_grouped_gemm_nt_bf16(_ptr(A), lda, 1, _ptr(W), None, _ptr(off), _ptr(perm), P, E, N, Kd, _ptr(Y), _stream()),
        "amk_grouped_gemm_nn_bf16": lambda Y: L.amk_grouped_gemm_nn_bf16(_ptr(A), lda, 1, _ptr(W), _ptr(scale), _ptr(off), _ptr(perm), P, E, N, Kd, _ptr(Y), _stream()),
        "amk_grouped_gemm_wgrad_bf16": lambda Y: L.amk_grouped_gemm_wgrad_bf16(_ptr(A), lda, 1, _ptr(A), lda, 1, _ptr(scale), _ptr(off), _ptr(perm),
                                                                             P, E, N, Kd, _ptr(Y), None, _stream()),
    }
    for name, call in calls.items():
        whole, Y = canvas(E * N, max(N, Kd), device)
        rc = call(Y)
        msg = L.amk_last_error().decode()
        assert rc == want, f"{name} {what}: code {rc}, message {msg!r}"
        assert msg.startswith(name + ":") and text in msg, f"{name} {what}: message {msg!r}"
        torch.cuda.synchronize()
        assert bool(torch.isnan(whole).all()), f"{name} {what}: the canvas was written"


# ---------------------------------------------------------------------------------------------- op level
def _op_inputs(U, D_, E, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(U, D_, generator=g).to(dev)
    W = (torch.randn(E, D_, D_, generator=g) / D_ ** 0.5).to(dev)
    bias = (torch.randn(E, D_, generator=g) / 4).to(dev)
    logits = torch.randn(U, E, generator=g).to(dev)
    d_out = torch.randn(U, D_, generator=g).to(dev)
    return x, W, bias, logits, d_out


def _run_op(fn, x, logits, W, bias, d_out, **kw):
    """(out, ids, dx, dlogits, dW, db, event names) of one forward + backward."""
    from amk import ops

    x, logits, W, bias = (t.detach().clone().requires_grad_(True) for t in (x, logits, W, bias))
    ops.KERNEL_EVENTS = {}
    try:
        out, ids = fn(x, logits, W, bias, **kw)
        out.backward(d_out)
        torch.cuda.synchronize()
        names = list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    return out.detach(), ids, x.grad, logits.grad, W.grad, bias.grad, names


def _f32_names(names):
    return [n for n in names if n.startswith(("grouped_nt P", "grouped_nn P", "grouped_wgrad P"))]


@pytest.mark.parametrize("U,D_,E,k", [(130, 64, 4, 2), (390, 264, 8, 2), (97, 128, 5, 3)])
def test_op_under_bf16_autocast(device, U, D_, E, k):
    """ops.routed_linear as MoELayer calls it: the composed bounds, the ids of _RoutedLinear, the bf16 kernels' events."""
    from amk import ops

    x, W, bias, logits, d_out = _op_inputs(U, D_, E, 21, device)
    with torch.autocast("cuda", dtype=BF16):
        out, ids, dx, dl, dW, db, names = _run_op(ops.routed_linear, x, logits, W, bias, d_out, k=k, x_div=k, weighted=True, outer=1)
    assert out.dtype == torch.float32 and dx.dtype == torch.float32 and dl.dtype == torch.float32
    assert dW.dtype == torch.float32 and db.dtype == torch.float32
    for kind in ("nt", "nn", "wgrad"):
        assert any(n.startswith(f"bf16_grouped_{kind} P") for n in names), names
    assert not _f32_names(names), names
    _, ids32 = ops._RoutedLinear.apply(x, logits, W, bias, k, k, True, 1)
    assert torch.equal(ids, ids32)
    route = ops.moe_route(logits, k)
    assert torch.equal(route["ids"], ids)
    R = ref.ref_op(x, logits, W, bias, d_out, route, k)
    for name, got in (("out", out), ("dx", dx), ("dlogits", dl), ("dw", dW), ("db", db)):
        ref.assert_bounded(got, R, name, f"op U{U} D{D_} E{E} k{k}")
    # no-grad forward (eval): the same path, the same bits
    ops.KERNEL_EVENTS = {}
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
            out2, _ = ops.routed_linear(x, logits, W, bias, k, k)
        assert any(n.startswith("bf16_grouped_nt P") for n in ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None
    assert same_bits(out, out2)
    # bf16 activations and logits, as the autocast Linear layers hand them over: gradients come back in bf16
    with torch.autocast("cuda", dtype=BF16):
        o16, _, dx16, dl16, dW16, _, _ = _run_op(ops.routed_linear, x.to(BF16), logits.to(BF16), W, bias, d_out, k=k, x_div=k)
    assert o16.dtype == torch.float32 and dx16.dtype == BF16 and dl16.dtype == BF16 and dW16.dtype == torch.float32
    route16 = ops.moe_route(logits.to(BF16).float(), k)
    R16 = ref.ref_op(x.to(BF16), logits.to(BF16), W, bias, d_out, route16, k)
    for name, got in (("out", o16), ("dx", dx16), ("dlogits", dl16), ("dw", dW16)):
        ref.assert_bounded(got, R16, name, f"op bf16 inputs U{U} D{D_}")


@pytest.mark.parametrize("variant", ["switch_off", "no_autocast", "N12", "unweighted", "outer2"])
def test_dispatch_keeps_todays_path(device, variant, monkeypatch):
    """Each of these takes _RoutedLinear with the f32 event names and equals it bit for bit on the upcast inputs."""
    import contextlib

    from amk import ops

    U, E, k = 128, 4, 2
    D_ = 12 if variant == "N12" else 64
    x, W, bias, logits, d_out = _op_inputs(U, D_, E, 22, device)
    kw = dict(k=k, x_div=k, weighted=variant != "unweighted", outer=2 if variant == "outer2" else 1)
    if variant == "outer2":
        d_out = d_out[:U // 2].contiguous()
    if variant == "switch_off":
        monkeypatch.setattr(ops, "MOE_BF16", False)
    amp = contextlib.nullcontext() if variant == "no_autocast" else torch.autocast("cuda", dtype=BF16)
    with amp:
        got = _run_op(ops.routed_linear, x, logits, W, bias, d_out, **kw)
        want = _run_op(lambda a, b, c, d, **q: ops._RoutedLinear.apply(a.float(), b.float(), c, d, q["k"], q["x_div"], q["weighted"], q["outer"]),
                       x, logits, W, bias, d_out, **kw)
    names = got[6]
    assert not any(n.startswith("bf16_grouped") for n in names), names
    assert {n.split(" ")[0] for n in _f32_names(names)} == {"grouped_nt", "grouped_nn", "grouped_wgrad"}, names
    for a, b in zip(got[:6], want[:6]):
        assert (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))


def test_model_reads_the_bf16_shadow(device):
    """MoELayer(256, 256, 8, 2) under autocast after one FlatAdam(bf16_shadow=True) step reads the optimizer's bf16 copy
    of the expert weights and stays inside the composed bounds; after an in-place write it falls back to a cast."""
    from amk import ops
    from amk.dp import GradReducer
    from amk.models import MoELayer
    from amk.optim import FlatAdam

    torch.manual_seed(0)
    m = MoELayer(256, 256, 8, 2).to(device)
    red = GradReducer(m.parameters(), bucket_bytes=256 << 10)
    opt = FlatAdam(red, lr=1e-3, bf16_shadow=True)
    x = torch.randn(2, 65, 256, generator=torch.Generator().manual_seed(1)).to(device)
    red.begin(True)
    with torch.autocast("cuda", dtype=BF16):
        out = m(x)
    out.float().pow(2).mean().backward()
    red.finish(detach_unused=False)
    opt.step(max_norm=1.0)
    Wp = m.experts_weight
    assert ops._w16(Wp) is Wp._amk_bf16

    def check(tag):
        seen = []
        real = ops._w16

        def spy(t):
            r = real(t)
            if t is Wp:
                seen.append(r)
            return r
        ops._w16 = spy
        try:
            xi = x.detach().clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=BF16):
                y = m(xi)
                logits = m.gate(xi).reshape(-1, 8)          # the bf16 logits the layer routed on
        finally:
            ops._w16 = real
        d_out = torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).to(device)
        for p in m.parameters():
            p.grad = None
        y.backward(d_out)
        assert len(seen) == 1
        route = ops.moe_route(logits.detach().float(), 2)
        assert torch.equal(route["ids"].view(2, 65, 2), m.last_selected_experts)
        R = ref.ref_op(xi.detach().reshape(-1, 256), logits.detach().float(), seen[0].float(), m.experts_bias.detach(),
                       d_out.reshape(-1, 256), route, 2)
        ref.assert_bounded(y.detach().reshape(-1, 256), R, "out", tag)
        ref.assert_bounded(m.experts_weight.grad, R, "dw", tag)
        ref.assert_bounded(m.experts_bias.grad, R, "db", tag)
        return seen[0]

    assert check("shadow") is Wp._amk_bf16
    with torch.no_grad():
        Wp.mul_(1.5)
    w = check("after an in-place write")
    assert w is not Wp._amk_bf16 and torch.equal(w, Wp.detach().to(BF16))


@pytest.mark.timeout(600)
def test_captured_autocast_step_replays_like_eager(device):
    """ClassifierTrainStep on the reduced ViTMoE with autocast=bfloat16, capturable=True: three captured steps equal three
    eager steps to the bit (parameters and losses), and an eager step runs the bf16 expert kernels."""
    from amk import ops
    from amk.models import ViTMoE
    from amk.train import ClassifierTrainStep

    old = ops.DETERMINISTIC_ATTENTION_BACKWARD
    ops.DETERMINISTIC_ATTENTION_BACKWARD = True
    try:
        torch.manual_seed(0)
        base = ViTMoE(**SMALL_MOE).to(device)
        g = torch.Generator().manual_seed(5)
        imgs, labels = torch.randn(8, 3, 64, 64, generator=g).to(device), torch.randint(0, 10, (8,), generator=g).to(device)
        runs = []
        for graphed in (False, True):
            model = copy.deepcopy(base)
            ts = ClassifierTrainStep(model, lr=1e-3, warmup_steps=2, total_steps=20, bucket_bytes=256 << 10, capturable=True,
                                     autocast=BF16)
            losses = []
            if graphed:
                ts.capture(imgs, labels, warmup=2)
            else:
                ops.KERNEL_EVENTS = {}
                try:
                    losses.append(ts.step(imgs, labels))
                    torch.cuda.synchronize()
                    names = list(ops.KERNEL_EVENTS)
                finally:
                    ops.KERNEL_EVENTS = None
                for kind in ("nt", "nn", "wgrad"):
                    assert any(n.startswith(f"bf16_grouped_{kind} P") for n in names), names
                losses.append(ts.step(imgs, labels))
            for _ in range(3):
                losses.append(ts.step(imgs, labels).clone())
            if graphed:
                assert ts._graph is not None
            torch.cuda.synchronize()
            runs.append((losses[-3:], [p.detach().clone() for p in model.parameters()], ts.global_step))
        (l0, p0, s0), (l1, p1, s1) = runs
        assert s0 == s1 == 5
        for a, b in zip(l0, l1):
            assert torch.isfinite(a) and torch.equal(a, b), (a, b)
        for a, b in zip(p0, p1):
            assert torch.equal(a, b)
    finally:
        ops.DETERMINISTIC_ATTENTION_BACKWARD = old
