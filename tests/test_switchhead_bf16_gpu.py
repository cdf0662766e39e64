"""SwitchHeadAttention's experts under bf16 autocast on the MI355X: the narrow grouped GEMMs and the bf16 per-expert
sums of csrc/moe_bf16.hip, ops._SharedRowExpertsBF16 / _SummedExpertsBF16, the model and a captured step.

C ABI: each entry point writes into a NaN canvas with guard rows; the guards and the rows no list names stay untouched
and every named element is held to the tiers of tests/switchhead_bf16_ref.py against fp64 references on the bf16
values, over the case list of that file (counts one below, at and one above the pair tile 256, a wave's 64 pairs and
the weight gradient's step 32, narrow widths 8 / 56 / 64, the other side around the weight gradient's wide tile 128 and
the contraction step 32, empty experts, sparse and distinct lists, padded strides, NULL bias / scale).  The wide entry
points on the same inputs are inside the same bounds.  Results repeat bit for bit; a pair's row does not depend on its
position.  Op level: the composed bounds, the dispatch back to the f32 Functions, the optimizer's bf16 shadow, and a
captured train step of a reduced ViTMoE equal to the eager one.
AMK_SWITCHHEAD_BF16_BOUNDS_REPORT=<file>: the worst ratios as JSON."""
import contextlib
import copy
import ctypes
import json
import os

import pytest
import torch

import switchhead_bf16_ref as ref
from test_switchhead_bf16_bounds import _inputs, _op_case

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
GUARD = 3
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nkernel: worst hard ratio, worst q / limit")
    for key, (ratio, q) in sorted(ref.WORST.items()):
        print(f"  {key:12s} {ratio:.4f}  {'-' if q is None else format(q, '.4f')}")
    path = os.environ.get("AMK_SWITCHHEAD_BF16_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(ref.WORST, f, indent=1)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def canvas(rows, width, dev, dtype=F32):
    whole = torch.full((rows + 2 * GUARD, width), float("nan"), device=dev, dtype=dtype)
    return whole, whole[GUARD:GUARD + rows]


def guards_untouched(whole, rows):
    return bool(torch.isnan(torch.cat([whole[:GUARD], whole[GUARD + rows:]])).all())


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    it = torch.int32 if a.element_size() == 4 else torch.int16
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _lib():
    from amk import lib as L_

    return L_, L_.load()


def run_grouped(kind, D, off, perm, P, E, N, Kd, a_div, vec, wide=False):
    """One launch of amk_grouped_gemm_{nt,nn}64_bf16 (wide: the 256-output entry point) into a NaN canvas."""
    L_, L = _lib()
    src = D["A"] if kind == "nt" else D["Gm"]
    whole, Y = canvas(P, N if kind == "nt" else Kd, src.device)
    name = f"amk_grouped_gemm_{kind}{'' if wide else '64'}_bf16"
    L_.check(getattr(L, name)(_ptr(src), src.stride(0), a_div, _ptr(D["W"]), _ptr(vec), _ptr(off), _ptr(perm), P, E, N, Kd, _ptr(Y),
                              _stream()), name)
    return whole, Y


def run_wgrad(D, off, perm, P, E, N, Kd, g_div, x_div, scale, wide=False):
    L_, L = _lib()
    wW, dW = canvas(E * N, Kd, D["Gm"].device)
    args = [_ptr(D["Gm"]), D["Gm"].stride(0), g_div, _ptr(D["X"]), D["X"].stride(0), x_div, _ptr(scale), _ptr(off), _ptr(perm),
            P, E, N, Kd, _ptr(dW)]
    if wide:
        L_.check(L.amk_grouped_gemm_wgrad_bf16(*args, None, _stream()), "amk_grouped_gemm_wgrad_bf16")
    else:
        L_.check(L.amk_grouped_gemm_wgrad64_bf16(*args, _stream()), "amk_grouped_gemm_wgrad64_bf16")
    return wW, dW


def run_sums(A, a_div, ids, scale, G, fan, E, d):
    L_, L = _lib()
    whole, Z = canvas(G, E * d, A.device, BF16)
    L_.check(L.amk_moe_expert_sums_bf16(_ptr(A), int(A.dtype == BF16), A.stride(0), a_div, _ptr(ids), _ptr(scale), G, fan, E, d,
                                        _ptr(Z), _stream()), "amk_moe_expert_sums_bf16")
    return whole, Z


def _device_case(c, dev):
    DD, (ids, off, perm), P = _inputs(c)
    return {o: {k: v.to(dev) for k, v in D.items()} for o, D in DD.items()}, off.to(dev), perm.to(dev), P


def test_case_list_covers_the_kernels(device):
    missing = ref.missing_coverage()
    assert not missing, f"the case list does not reach: {sorted(missing)}"


@pytest.mark.parametrize("c", ref.CASES, ids=lambda c: c["id"])
def test_narrow_grouped_gemms(device, c):
    E, d, w, a_div, x_div = c["E"], c["d"], c["w"], c["a_div"], c["x_div"]
    DD, off, perm, P = _device_case(c, device)
    empty = (off[1:] - off[:-1]) == 0
    for kind, D, (N, Kd) in (("nt", DD["v"], (d, w)), ("nn", DD["o"], (w, d))):
        vec = None if c["nulls"] else (D["bias"] if kind == "nt" else D["scale"])
        src = D["A"] if kind == "nt" else D["Gm"]
        whole, Y = run_grouped(kind, D, off, perm, P, E, N, Kd, a_div, vec)
        R = (ref.ref_nt if kind == "nt" else ref.ref_nn)(src, src.stride(0), a_div, D["W"], vec, off, perm, P, E, N, Kd)
        ref.assert_within(Y, R, "y", kind + "64", f"{c['id']} {kind}64")
        assert guards_untouched(whole, P), f"{c['id']} {kind}64: a guard row was written"
        assert bool(torch.isnan(Y[~R["named_y"]]).all()), f"{c['id']} {kind}64: a row the lists do not name was written"
        _, Y2 = run_grouped(kind, D, off, perm, P, E, N, Kd, a_div, vec)
        assert same_bits(Y, Y2), f"{c['id']} {kind}64: two calls differ"
        _, Yw = run_grouped(kind, D, off, perm, P, E, N, Kd, a_div, vec, wide=True)          # both are correct answers
        ref.assert_within(Yw, R, "y", kind + "64", f"{c['id']} {kind} (wide entry point)", key=kind + "_wide")
    for o, (N, Kd) in (("v", (d, w)), ("o", (w, d))):
        D = DD[o]
        for use_scale in ((False,) if c["nulls"] else (True, False)):
            what = f"{c['id']} wgrad64 N{N} K{Kd}{'' if use_scale else ' noscale'}"
            scale = D["scale"] if use_scale else None
            wW, dW = run_wgrad(D, off, perm, P, E, N, Kd, a_div, x_div, scale)
            R = ref.ref_wgrad(D["Gm"], D["Gm"].stride(0), a_div, D["X"], D["X"].stride(0), x_div, scale, off, perm, P, E, N, Kd)
            ref.assert_within(dW.view(E, N, Kd), R, "dw", "dw64", what)
            assert guards_untouched(wW, E * N), f"{what}: a guard row was written"
            assert bool((dW.view(E, N, Kd)[empty] == 0).all()), f"{what}: an expert without pairs is not exactly zero"
            _, dW2 = run_wgrad(D, off, perm, P, E, N, Kd, a_div, x_div, scale)
            assert same_bits(dW, dW2), f"{what}: two calls differ"
            _, dWw = run_wgrad(D, off, perm, P, E, N, Kd, a_div, x_div, scale, wide=True)
            ref.assert_within(dWw.view(E, N, Kd), R, "dw", "dw64", what + " (wide entry point)", key="dw_wide")


@pytest.mark.parametrize("c", ref.SUM_CASES, ids=lambda c: c["id"])
def test_expert_sums_bf16(device, c):
    L_, L = _lib()
    A, ids, scale = (None if t is None else t.to(device) for t in ref.sum_inputs(c))
    G, fan, E, d, a_div = c["G"], c["fan"], c["E"], c["d"], c["a_div"]
    whole, Z = run_sums(A, a_div, ids, scale, G, fan, E, d)
    R = ref.ref_expert_sums(A, A.stride(0), a_div, ids, scale, G, fan, E, d)
    ref.assert_within(Z, R, "z", "sums", c["id"])
    assert guards_untouched(whole, G) and not bool(torch.isnan(Z).any()), f"{c['id']}: guards written or Z not fully overwritten"
    assert bool((Z[R["S_z"] == 0] == 0).all()), f"{c['id']}: an expert no pair of the row chose is not exactly zero"
    _, Z2 = run_sums(A, a_div, ids, scale, G, fan, E, d)
    assert same_bits(Z, Z2), f"{c['id']}: two calls differ"
    if A.dtype == F32:      # the f32 kernel's sums, rounded once
        Z32 = torch.empty(G, E * d, device=device)
        L_.check(L.amk_moe_expert_sums(_ptr(A), A.stride(0), a_div, _ptr(ids), _ptr(scale), G, fan, E, d, _ptr(Z32), _stream()),
                 "amk_moe_expert_sums")
        assert same_bits(Z, Z32.to(BF16)), f"{c['id']}: not the f32 kernel's sums rounded to bf16"


@pytest.mark.parametrize("d,w", [(64, 128), (8, 136), (56, 264)])
def test_position_free(device, d, w):
    """The rows of the pairs that two lists share (same expert, another position, another tile) are equal bit for bit."""
    ids, off, perm = ref.make_lists(ref.EDGE, seed=5)
    P, E = ids.numel(), len(ref.EDGE)
    keep = torch.rand(P, generator=torch.Generator().manual_seed(6)) < 0.7
    cnt2 = torch.bincount(ids[keep], minlength=E)
    off2 = torch.zeros(E + 1, dtype=torch.int32)
    off2[1:] = torch.cumsum(cnt2, 0)
    rows = torch.nonzero(keep).view(-1)
    perm2 = rows[torch.sort(ids[rows], stable=True)[1]].int()
    kd = keep.to(device)
    for kind, (N, Kd) in (("nt", (d, w)), ("nn", (w, d))):
        D = {k: v.to(device) for k, v in ref.make_data("binade", P, E, N, Kd, 2, 2, 9).items()}
        vec = D["bias"] if kind == "nt" else D["scale"]
        _, Y1 = run_grouped(kind, D, off.to(device), perm.to(device), P, E, N, Kd, 2, vec)
        _, Y2 = run_grouped(kind, D, off2.to(device), perm2.to(device), P, E, N, Kd, 2, vec)
        assert bool(torch.isnan(Y2[~kd]).all()) and not bool(torch.isnan(Y2[kd]).any())
        assert same_bits(Y1[kd], Y2[kd]), f"{kind}64 d{d} w{w}: a row depends on its position"


@pytest.mark.parametrize("N,Kd", [(64, 136), (136, 56)])
def test_wgrad_is_free_of_the_other_experts(device, N, Kd):
    """dW[e] is a sum over e's pairs in list order, so a pair's position inside its expert is part of the result; what
    must not matter is everything else: with every other expert emptied (e's pairs now start the list), dW[e] keeps its
    bits and the emptied experts are exactly zero."""
    ids, off, perm = ref.make_lists(ref.EDGE, seed=5)
    P, E = ids.numel(), len(ref.EDGE)
    D = {k: v.to(device) for k, v in ref.make_data("binade", P, E, N, Kd, 2, 2, 9).items()}
    _, dW1 = run_wgrad(D, off.to(device), perm.to(device), P, E, N, Kd, 2, 2, D["scale"])
    o = off.long().tolist()
    for e in (2, 7, 10):                                   # 31, 65 and 257 pairs
        off2 = torch.zeros(E + 1, dtype=torch.int32)
        off2[e + 1:] = o[e + 1] - o[e]
        perm2 = perm[o[e]:o[e + 1]].clone()
        _, dW2 = run_wgrad(D, off2.to(device), perm2.to(device), P, E, N, Kd, 2, 2, D["scale"])
        dW1e, dW2e = dW1.view(E, N, Kd), dW2.view(E, N, Kd)
        assert same_bits(dW1e[e], dW2e[e]), f"wgrad64 N{N} K{Kd}: dW[{e}] depends on the other experts"
        rest = [j for j in range(E) if j != e]
        assert bool((dW2e[rest] == 0).all())


@pytest.mark.parametrize("what", ["N72", "N12", "misaligned", "stride68"])
def test_refusals(device, what):
    """The documented code and the library's message, before any device work: the canvas stays untouched."""
    L_, L = _lib()
    E, P = 3, 40
    nar = {"N72": 72, "N12": 12}.get(what, 64)
    ids, off, perm = ref.make_lists([10, 14, 16], seed=1)
    off, perm = off.to(device), perm.to(device)
    lda = 68 if what == "stride68" else 72
    buf = torch.zeros(P * 72 + 8, device=device, dtype=BF16)
    A = buf[1:] if what == "misaligned" else buf
    W = torch.zeros(E, 72, 72, device=device, dtype=BF16)
    scale = torch.ones(P, device=device)
    ids64 = torch.zeros(P, device=device, dtype=torch.int64)
    want = EUNSUPPORTED if what in ("N72", "N12") else EINVAL
    text = {"N72": "at most 64", "N12": "must be multiples of 8", "misaligned": "16-byte aligned", "stride68": "row stride 68"}[what]
    other = 72 if what == "N72" else 64      # wgrad64 refuses only when BOTH sides are above 64
    calls = {
        "amk_grouped_gemm_nt64_bf16": lambda Y: L.amk_grouped_gemm_nt64_bf16(_ptr(A), lda, 1, _ptr(W), None, _ptr(off), _ptr(perm), P, E, nar, 64, _ptr(Y), _stream()),
        "amk_grouped_gemm_nn64_bf16": lambda Y: L.amk_grouped_gemm_nn64_bf16(_ptr(A), lda, 1, _ptr(W), _ptr(scale), _ptr(off), _ptr(perm), P, E, 64, nar, _ptr(Y), _stream()),
        "amk_grouped_gemm_wgrad64_bf16": lambda Y: L.amk_grouped_gemm_wgrad64_bf16(_ptr(A), lda, 1, _ptr(A), lda, 1, _ptr(scale), _ptr(off), _ptr(perm),
                                                                                 P, E, nar, other, _ptr(Y), _stream()),
    }
    if what != "N72":       # the sums have no narrow side
        calls["amk_moe_expert_sums_bf16"] = lambda Y: L.amk_moe_expert_sums_bf16(_ptr(A), 1, lda, 1, _ptr(ids64), _ptr(scale), P // 4, 4, E, nar, _ptr(Y), _stream())
    for name, call in calls.items():
        whole, Y = canvas(E * 72, 72, device)
        rc = call(Y)
        msg = L.amk_last_error().decode()
        assert rc == want, f"{name} {what}: code {rc}, message {msg!r}"
        assert msg.startswith(name + ":") and text in msg, f"{name} {what}: message {msg!r}"
        torch.cuda.synchronize()
        assert bool(torch.isnan(whole).all()), f"{name} {what}: the canvas was written"


# ---------------------------------------------------------------------------------------------- op level
def _events(fn):
    """(result of fn, the event names it recorded)."""
    from amk import ops

    ops.KERNEL_EVENTS = {}
    try:
        r = fn()
        torch.cuda.synchronize()
        return r, list(ops.KERNEL_EVENTS)
    finally:
        ops.KERNEL_EVENTS = None


def _run(fn, a, logits, W, d_out, k, H, grads=(True, True, True)):
    """(out, ids, d a, d logits, d W, event names) of one forward + backward; d_out is cast to out's dtype."""
    a, logits, W = (t.detach().clone().requires_grad_(g) for t, g in zip((a, logits, W), grads))

    def go():
        out, ids = fn(a, logits, W, k, H)
        out.backward(d_out.to(out.dtype))
        return out, ids
    (out, ids), names = _events(go)
    return out.detach(), ids, a.grad, logits.grad, W.grad, names


F32_NAMES = ("grouped_nt P", "grouped_nn P", "grouped_wgrad P", "dense_z_gemm M", "moe_expert_sums G")


def _f32_names(names):
    return [n for n in names if n.startswith(F32_NAMES)]


def _to_dev(T, dev):
    return {k: v.to(dev) for k, v in T.items()}


@pytest.mark.parametrize("shape", ref.OP_SHAPES, ids=lambda s: "G%d_H%d_k%d_E%d_dim%d_d%d" % s)
def test_ops_under_bf16_autocast(device, shape):
    """Both Functions: the composed bounds, the ids of the f32 Functions, the bf16 kernels' events, the dtypes, and a
    no-grad forward with the same bits."""
    from amk import ops

    G, H, k, E, dim, d = shape
    T = _to_dev(_op_case(G, H, k, E, dim, d, 31), device)
    what = "G%d H%d k%d E%d dim%d d%d" % shape
    amp = lambda: torch.autocast("cuda", dtype=BF16)
    # V experts
    with amp():
        out, ids, dx, dl, dW, names = _run(ops.shared_row_experts, T["x"], T["logits"], T["Wv"], T["dv"], k, H)
    assert (out.dtype, dx.dtype, dl.dtype, dW.dtype) == (F32, F32, F32, F32)
    for n in ("bf16_grouped_nt P", "bf16_moe_expert_sums G", "bf16_dense_z_gemm M", "bf16_grouped_wgrad P"):
        assert any(e.startswith(n) for e in names), (n, names)
    assert not _f32_names(names), names
    _, ids32 = ops._SharedRowExperts.apply(T["x"], T["logits"], T["Wv"], k, H)
    assert torch.equal(ids, ids32)
    ids_k, gate = ops._topk(T["logits"], k)
    assert torch.equal(ids_k, ids)
    R = ref.ref_shared_row(T["x"], T["logits"], T["Wv"], T["dv"], ids, gate, k, H)
    for name, got in (("out", out), ("dx", dx), ("dlogits", dl), ("dw", dW)):
        ref.assert_bounded(got, R, name, f"V experts {what}")
    with torch.no_grad(), amp():
        (out2, _), names2 = _events(lambda: ops.shared_row_experts(T["x"], T["logits"], T["Wv"], k, H))
    assert same_bits(out, out2) and any(e.startswith("bf16_grouped_nt P") for e in names2) and not _f32_names(names2)
    # bf16 rows, logits and output gradient, as autocast Linear layers hand them over: gradients come back in bf16
    with amp():
        o16, i16, dx16, dl16, dW16, _ = _run(ops.shared_row_experts, T["x"].to(BF16), T["logits"].to(BF16), T["Wv"], T["dv"].to(BF16), k, H)
    assert (o16.dtype, dx16.dtype, dl16.dtype, dW16.dtype) == (F32, BF16, BF16, F32)
    i16k, gate16 = ops._topk(T["logits"].to(BF16).float(), k)
    assert torch.equal(i16k, i16)
    R16 = ref.ref_shared_row(T["x"].to(BF16), T["logits"].to(BF16), T["Wv"], T["dv"].to(BF16), i16, gate16, k, H)
    for name, got in (("out", o16), ("dx", dx16), ("dlogits", dl16), ("dw", dW16)):
        ref.assert_bounded(got, R16, name, f"V experts, bf16 inputs {what}")
    # output experts
    with amp():
        out, ids, da, dlo, dW, names = _run(ops.summed_experts, T["a"], T["logits"], T["Wo"], T["do"], k, H)
    assert (out.dtype, da.dtype, dW.dtype) == (BF16, F32, F32) and dlo is None
    for n in ("bf16_moe_expert_sums G", "bf16_dense_z_gemm M", "bf16_grouped_nn P", "bf16_grouped_wgrad P"):
        assert any(e.startswith(n) for e in names), (n, names)
    assert not _f32_names(names), names
    _, ids32 = ops._SummedExperts.apply(T["a"], T["logits"], T["Wo"], k, H)
    assert torch.equal(ids, ids32)
    Ro = ref.ref_summed(T["a"], T["logits"], T["Wo"], T["do"], ids, k, H)
    for name, got in (("out", out), ("da", da), ("dw", dW)):
        ref.assert_bounded(got, Ro, name, f"output experts {what}")
    with torch.no_grad(), amp():
        (out2, _), names2 = _events(lambda: ops.summed_experts(T["a"], T["logits"], T["Wo"], k, H))
    assert same_bits(out, out2) and any(e.startswith("bf16_dense_z_gemm M") for e in names2) and not _f32_names(names2)


@pytest.mark.parametrize("variant", ["switch_off", "no_autocast", "d96", "frozen_weight"])
def test_dispatch_keeps_todays_path(device, variant, monkeypatch):
    """Each of these takes the f32 Functions with the f32 event names and equals them bit for bit on the upcast inputs."""
    from amk import ops

    G, H, k, E, dim = 66, 4, 2, 4, 384
    d = 96 if variant == "d96" else 64
    T = _to_dev(_op_case(G, H, k, E, dim, d, 32), device)
    if variant == "switch_off":
        monkeypatch.setattr(ops, "SWITCHHEAD_BF16", False)
    grads = (True, True, variant != "frozen_weight")
    amp = contextlib.nullcontext() if variant == "no_autocast" else torch.autocast("cuda", dtype=BF16)
    for fn, F, a, W, d_out, kinds in ((ops.shared_row_experts, ops._SharedRowExperts, T["x"], T["Wv"], T["dv"], ("grouped_nt", "grouped_wgrad")),
                                      (ops.summed_experts, ops._SummedExperts, T["a"], T["Wo"], T["do"], ("grouped_nn", "grouped_wgrad"))):
        with amp:
            got = _run(fn, a, T["logits"], W, d_out, k, H, grads)
            want = _run(lambda p, q, r, kk, hh: F.apply(p.float(), q.float(), r, kk, hh), a, T["logits"], W, d_out, k, H, grads)
        names = got[5]
        assert not any(n.startswith("bf16_") for n in names), names
        assert {n.split(" ")[0] for n in _f32_names(names)} >= set(kinds) | {"dense_z_gemm", "moe_expert_sums"}, names
        for x, y in zip(got[:5], want[:5]):
            assert (x is None and y is None) or (x.dtype == y.dtype and torch.equal(x, y)), variant


# ---------------------------------------------------------------------------------------------- model
def _spy_ops(ops, rec):
    """Record what the two ops are handed and return inside the model, and the gradients that reach them."""
    real = {"v": ops.shared_row_experts, "o": ops.summed_experts, "attn": ops.attention}

    def attn(q, k, v, scale, **kw):
        rec.update({"q": q.detach(), "k": k.detach(), "scale": scale})
        return real["attn"](q, k, v, scale, **kw)
    ops.attention = attn

    def wrap(key):
        def f(a2, logits2, W, k, H):
            if a2.requires_grad:
                a2.register_hook(lambda g_: rec.__setitem__(key + "_da", g_.detach().clone()))
            if logits2.requires_grad:
                logits2.register_hook(lambda g_: rec.__setitem__(key + "_dl", g_.detach().clone()))
            out, ids = real[key](a2, logits2, W, k, H)
            out.register_hook(lambda g_: rec.__setitem__(key + "_dout", g_.detach().clone()))
            rec.update({key + "_a": a2.detach(), key + "_logits": logits2.detach(), key + "_out": out.detach(), key + "_ids": ids})
            return out, ids
        return f
    ops.shared_row_experts, ops.summed_experts = wrap("v"), wrap("o")
    return real


def test_model_under_autocast(device, monkeypatch):
    """SwitchHeadAttention(256, 4, 64, 4 experts, top 2) under bf16 autocast: the same selections with the switch on and
    off; the module's output, the gradient of every parameter and of the input inside the composed bounds of an fp64 run
    on the same bf16 values (tests/switchhead_bf16_ref.py, "The model"): the experts' weights through the two Functions,
    q and k through the f32 attention core's bound on the bounded v and d_o and the projection's library GEMM, W_s
    through that GEMM on dlogits, d x through both; W_d gets none."""
    from amk import ops
    from amk.models.attention import SwitchHeadAttention

    torch.manual_seed(0)
    m = SwitchHeadAttention(256, 4, 64, num_experts=4, sel_experts=2).to(device)
    x = torch.randn(2, 65, 256, generator=torch.Generator().manual_seed(1)).to(device)
    d_out = torch.randn(2, 65, 256, generator=torch.Generator().manual_seed(2)).to(device)
    H, k, E = 4, 2, 4

    def step(rec=None):
        real = _spy_ops(ops, rec) if rec is not None else None
        try:
            for p in m.parameters():
                p.grad = None
            xi = x.detach().clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=BF16):
                (y, names) = _events(lambda: m(xi))
            y.backward(d_out.to(y.dtype))
            torch.cuda.synchronize()
        finally:
            if real is not None:
                ops.shared_row_experts, ops.summed_experts, ops.attention = real["v"], real["o"], real["attn"]
        return y.detach(), {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}, names, \
            (m.last_selected_v.clone(), m.last_selected_out.clone()), xi.grad

    rec = {}
    y, grads, names, sel, dxi = step(rec)
    assert any(n.startswith("bf16_grouped_nt P") for n in names) and not _f32_names(names), names
    assert y.dtype == BF16 and grads["W_d.0.weight"] is None
    ids_v, gate = ops._topk(rec["v_logits"].float(), k)
    assert torch.equal(ids_v, rec["v_ids"]) and torch.equal(sel[0].reshape(-1, k), ids_v)
    Rv = ref.ref_shared_row(rec["v_a"], rec["v_logits"], m.experts_v_weight.detach(), rec["v_dout"], rec["v_ids"], gate, k, H)
    ref.assert_bounded(rec["v_out"], Rv, "out", "model, V experts")
    ref.assert_bounded(rec["v_da"], Rv, "dx", "model, V experts")
    ref.assert_bounded(rec["v_dl"], Rv, "dlogits", "model, V experts")
    ref.assert_bounded(grads["experts_v_weight"], Rv, "dw", "model, V experts")
    Ro = ref.ref_summed(rec["o_a"], rec["o_logits"], m.experts_out_weight.detach(), rec["o_dout"], rec["o_ids"], k, H)
    ref.assert_bounded(y.reshape(-1, 256), Ro, "out", "model")
    ref.assert_bounded(rec["o_da"], Ro, "da", "model, output experts")
    ref.assert_bounded(grads["experts_out_weight"], Ro, "dw", "model, output experts")
    # behind the two Functions.  The f32 attention core reads the projection's bf16 q and k exactly, v within the V experts'
    # bound and d_o within the output experts' da bound; dq, dk and dlogits go back to the stacked projection in bf16
    B_, T, dh = 2, 65, 64
    heads = lambda t: t.reshape(B_, T, H, dh).permute(0, 2, 1, 3)
    Ra = ref.attention_backward(rec["q"], rec["k"], heads(Rv["out"]), heads(Rv["bound_out"]), heads(Ro["da"]), heads(Ro["bound_da"]),
                                rec["scale"])
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B_ * T, H * dh)
    x16 = x.reshape(-1, 256).to(BF16)
    M = x16.shape[0]
    g16 = {}                                            # what the projection's backward reads: (reference, bound) per block
    for n in ("dq", "dk"):
        r, b = rows(Ra[n]), rows(Ra["bound_" + n])
        g16[n] = (r, b + ref.U * (r.abs() + b))
    g16["dl"] = (Rv["dlogits"].view(M, H * E), Rv["bound_dlogits"].view(M, H * E))
    for n, key in (("q.0.weight", "dq"), ("k.0.weight", "dk"), ("W_s.0.weight", "dl")):
        r, b = ref.lib_wgrad(*g16[key], x16)
        ref.assert_bounded(grads[n], {"w": r, "bound_w": b}, "w", f"model, {n}")
    # d x = dx of the V experts + (dq | dk | dlogits)16 @ W16 by the library (bf16 out), added in f32
    W16 = torch.cat([m.q[0].weight, m.k[0].weight, m.W_s[0].weight], 0).detach().to(BF16)
    z, Bz = (torch.cat([g16[n][i] for n in ("dq", "dk", "dl")], 1) for i in (0, 1))
    r, b = ref.lib_gemm(z, Bz, W16)
    r, b = r + Rv["dx"], b + Rv["bound_dx"]
    ref.assert_bounded(dxi.reshape(M, 256), {"dx": r, "bound_dx": b + ref.U32 * (r.abs() + b)}, "dx", "model, d x")
    monkeypatch.setattr(ops, "SWITCHHEAD_BF16", False)
    y0, grads0, names0, sel0, _ = step()
    assert _f32_names(names0) and not any(n.startswith("bf16_") for n in names0), names0
    assert torch.equal(sel[0], sel0[0]) and torch.equal(sel[1], sel0[1])


def test_model_reads_the_bf16_shadow(device):
    """After one FlatAdam(bf16_shadow=True) step both expert weights are read through the optimizer's bf16 copy; after an
    in-place write through a cast."""
    from amk import ops
    from amk.dp import GradReducer
    from amk.models.attention import SwitchHeadAttention
    from amk.optim import FlatAdam

    torch.manual_seed(0)
    m = SwitchHeadAttention(256, 4, 64, num_experts=4, sel_experts=2).to(device)
    red = GradReducer(m.parameters(), bucket_bytes=256 << 10)
    opt = FlatAdam(red, lr=1e-3, bf16_shadow=True)
    x = torch.randn(2, 65, 256, generator=torch.Generator().manual_seed(1)).to(device)
    red.begin(True)
    with torch.autocast("cuda", dtype=BF16):
        out = m(x)
    out.float().pow(2).mean().backward()
    red.finish(detach_unused=False)
    opt.step(max_norm=1.0)
    Wv, Wo = m.experts_v_weight, m.experts_out_weight

    def seen_by_forward():
        seen, real = {}, ops._w16

        def spy(t):
            r = real(t)
            for name, p in (("v", Wv), ("o", Wo)):
                if t is p:
                    seen[name] = r
            return r
        ops._w16 = spy
        try:
            with torch.autocast("cuda", dtype=BF16):
                m(x)
        finally:
            ops._w16 = real
        return seen

    seen = seen_by_forward()
    assert seen["v"] is Wv._amk_bf16 and seen["o"] is Wo._amk_bf16
    with torch.no_grad():
        Wv.mul_(1.5)
        Wo.mul_(0.5)
    seen = seen_by_forward()
    assert seen["v"] is not Wv._amk_bf16 and torch.equal(seen["v"], Wv.detach().to(BF16))
    assert seen["o"] is not Wo._amk_bf16 and torch.equal(seen["o"], Wo.detach().to(BF16))


@pytest.mark.parametrize("on", [True, False])
def test_vit_moe_hands_switchhead_bf16_rows(device, on, monkeypatch):
    """In ViTMoE's encoder norm1 feeds only SwitchHead: under bf16 autocast its output arrives in bf16 when the switch is
    on (no cast pass in front of the projections and the experts) and in f32 when it is off -- and in f32 where
    SwitchHead keeps the f32 experts (dim 128: the routed form), switch on or off."""
    from amk import ops
    from amk.models import ViTMoE

    monkeypatch.setattr(ops, "SWITCHHEAD_BF16", on)
    torch.manual_seed(0)
    model = ViTMoE(dim=256, image_size=64, patch_size=16, n_heads=2, d_head=64, depth=2, n_experts=4, sel_experts=2, dropout=0.0,
                   num_classes=10).to(device)
    seen, real = [], ops.shared_row_experts
    monkeypatch.setattr(ops, "shared_row_experts", lambda x2, *a: (seen.append(x2.dtype), real(x2, *a))[1])
    with torch.autocast("cuda", dtype=BF16):
        model(torch.randn(2, 3, 64, 64, device=device)).float().sum().backward()
    assert seen == [BF16 if on else F32] * 2
    small = ViTMoE(dim=128, image_size=64, patch_size=16, n_heads=2, d_head=64, depth=1, n_experts=4, sel_experts=2, dropout=0.0,
                   num_classes=10).to(device)
    rows = []
    hook = small.encoder.layers[0].self_attn.register_forward_pre_hook(lambda mod, a, kw: rows.append(kw["x"].dtype), with_kwargs=True)
    with torch.autocast("cuda", dtype=BF16):
        small(torch.randn(2, 3, 64, 64, device=device))
    hook.remove()
    assert rows == [F32]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in model.named_parameters() if "W_d" not in n)


@pytest.mark.timeout(600)
def test_captured_autocast_step_replays_like_eager(device):
    """ClassifierTrainStep on a reduced ViTMoE of dim 256 (SwitchHead's distinct form applies) with autocast=bfloat16,
    capturable=True: captured steps equal eager steps to the bit, and an eager step runs SwitchHead's bf16 kernels."""
    from amk import ops
    from amk.models import ViTMoE
    from amk.train import ClassifierTrainStep

    cfg = dict(dim=256, image_size=64, patch_size=16, n_heads=2, d_head=64, depth=2, n_experts=4, sel_experts=2, dropout=0.0,
               num_classes=10)
    assert ops.distinct_experts_ok(256, 64, 2 * 2, 4)
    old = ops.DETERMINISTIC_ATTENTION_BACKWARD
    ops.DETERMINISTIC_ATTENTION_BACKWARD = True
    try:
        torch.manual_seed(0)
        base = ViTMoE(**cfg).to(device)
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
                loss, names = _events(lambda: ts.step(imgs, labels))
                losses.append(loss)
                for n in ("bf16_grouped_nt P", "bf16_grouped_nn P", "bf16_grouped_wgrad P"):
                    assert any(e.startswith(n) and e.endswith("(distinct rows)") for e in names), (n, names)
                for n in ("bf16_moe_expert_sums G", "bf16_dense_z_gemm M"):
                    assert any(e.startswith(n) for e in names), (n, names)
                assert not _f32_names(names), names
                losses.append(ts.step(imgs, labels))
            for _ in range(2):
                losses.append(ts.step(imgs, labels).clone())
            if graphed:
                assert ts._graph is not None
            torch.cuda.synchronize()
            runs.append((losses[-2:], [p.detach().clone() for p in model.parameters()], ts.global_step))
        (l0, p0, s0), (l1, p1, s1) = runs
        assert s0 == s1 == 4
        for a, b in zip(l0, l1):
            assert torch.isfinite(a) and torch.equal(a, b), (a, b)
        for a, b in zip(p0, p1):
            assert torch.equal(a, b)
    finally:
        ops.DETERMINISTIC_ATTENTION_BACKWARD = old
