"""The routed-expert ops of amk/ops.py pinned to the C ABI on the MI355X.

Each case runs the public op (routed_linear, shared_row_experts, summed_experts) forward and backward, then rebuilds
every output and gradient here as the sequence of C-ABI calls and torch products the op stands for -- sharing nothing
with ops.py but _ptr, _stream, moe_route, _topk and _route_distinct -- and asserts bit equality of out, ids, dx,
dlogits, dW and db, the dtypes handed back, and the names of the timed stages in the order they are emitted.  The
stages a case expects are written out per case; nothing here asks ops.py which path it would take.

Sizes: 150 units over 4 experts (8 for the SwitchHead forms) with top-2, expert 0 favoured: it gets more than 64
pairs, so a second row tile, and the last tile is partial.  The logits of a row are distinct levels 0.5 apart plus
noise below 0.1, so no ties in f32 or in bf16."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
K = 2


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() != 2 else torch.int16)


def assert_same(got, want, what):
    if want is None or got is None:
        assert got is None and want is None, f"{what}: {'missing' if got is None else 'unexpected'}"
        return
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} != {want.dtype} {tuple(want.shape)}"
    assert torch.equal(_bits(got), _bits(want)), f"{what}: bits differ"


def _logits(U, E, seed, dev, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(U, E, generator=g)
    s[:, 0] += 0.6
    level = s.argsort(1).argsort(1).to(F32)
    lg = (0.5 * level + 0.1 * torch.rand(U, E, generator=g)).to(dtype)
    assert int((lg.float().sort(1).values.diff(dim=1) == 0).sum()) == 0
    return lg.to(dev)


def _rand(shape, seed, dev, dtype=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(dtype).to(dev)


def _tiles_ok(offsets):
    c = int((offsets[1:] - offsets[:-1]).max())
    assert c > 64 and c % 64, f"largest expert has {c} pairs: want a second, partial row tile"


def _run(fn, args, d_out, amp, grads):
    """The public op under `amp`; args is a list of tensors / None, grads the indices of those that train."""
    from amk import ops

    leaves = [None if t is None else t.detach().clone().requires_grad_(i in grads) for i, t in enumerate(args)]
    ops.KERNEL_EVENTS = {}
    try:
        with amp:
            out, ids = fn(*leaves)
        out.backward(d_out)
        torch.cuda.synchronize()
        # KERNEL_EVENTS keys launches by label: a repeated label counts under its first appearance, so the order is pinned
        # up to that (no case here repeats one)
        names = [n for n, pairs in ops.KERNEL_EVENTS.items() for _ in pairs]
    finally:
        ops.KERNEL_EVENTS = None
    return out.detach(), ids, [None if t is None else t.grad for t in leaves], names


def _abi():
    from amk import lib, ops

    L = lib.load()

    def call(name, *a):
        lib.check(getattr(L, name)(*[ops._ptr(x) if isinstance(x, torch.Tensor) or x is None else x for x in a], ops._stream()), name)

    return ops, call


def _new(dev, *shape, dtype=F32):
    return torch.empty(shape, device=dev, dtype=dtype)


# ---------------------------------------------------------------------------- routed_linear, f32
def rebuild_routed_f32(x, logits, W, bias, x_div, weighted, outer, fwd, bwd, d_out):
    """fwd: 'dense' | 'combine'; bwd: 'dense' | 'combine' | 'skip' (no dx)."""
    ops, call = _abi()
    dev = x.device
    U, E = logits.shape
    N, Kd = W.shape[1], W.shape[2]
    P, G, fan = U * K, U // outer, outer * K
    r = ops.moe_route(logits, K)
    ids, gate, off, perm = r["ids"], r["gate"], r["offsets"], r["perm"]
    _tiles_ok(off)
    scale = gate if weighted else None
    Y = None
    if fwd == "dense":
        Z = _new(dev, G, E * Kd)
        call("amk_moe_expert_sums", x, x.stride(0), x_div, ids, None, G, fan, E, Kd, Z)
        out = Z @ W.permute(0, 2, 1).reshape(E * Kd, N)
    else:
        Y = _new(dev, P, N)
        call("amk_grouped_gemm_nt", x, Kd, x_div, W, bias, off, perm, P, E, N, Kd, Y)
        out = _new(dev, G, N)
        call("amk_moe_combine", Y, ids, scale, G, outer, K, N, out)
    dlogits = None
    if weighted:
        dlogits = _new(dev, U, E)
        call("amk_moe_gate_grad", d_out, Y, ids, gate, P, K, E, N, fan, dlogits)
    if bwd == "skip":
        dx = None
    elif bwd == "dense":
        Z = _new(dev, x.shape[0], E * N)
        call("amk_moe_expert_sums", d_out, d_out.stride(0), fan, ids, scale, x.shape[0], x_div, E, N, Z)
        dx = Z @ W.view(E * N, Kd)
    else:
        dxp = _new(dev, P, Kd)
        call("amk_grouped_gemm_nn", d_out, N, fan, W, scale, off, perm, P, E, N, Kd, dxp)
        dx = torch.empty_like(x)
        call("amk_moe_combine", dxp, ids, None, x.shape[0], x_div // K, K, Kd, dx)
    dW = torch.empty_like(W)
    db = _new(dev, E, N) if bias is not None else None
    call("amk_grouped_gemm_wgrad", d_out, N, fan, x, Kd, x_div, scale, off, perm, P, E, N, Kd, dW, db)
    return out, ids, dx, dlogits, dW, db


def _routed_events(U, E, N, Kd, outer, x_div, fwd, bwd):
    P, G, fan = U * K, U // outer, outer * K
    ev = [f"moe_route U{U} E{E} k{K}"]
    if fwd == "dense":
        ev += [f"moe_expert_sums G{G} fan{fan} E{E} d{Kd}", f"dense_z_gemm M{G} N{N} K{E * Kd}"]
    else:
        ev += [f"grouped_nt P{P} N{N} K{Kd}", f"moe_combine G{G} N{N} x{fan}"]
    if bwd == "dense":
        ev += [f"moe_expert_sums G{P // x_div} fan{x_div} E{E} d{N}", f"dense_z_gemm M{P // x_div} N{Kd} K{E * N}"]
    elif bwd == "combine":
        ev += [f"grouped_nn P{P} N{N} K{Kd}"]
    return ev + [f"grouped_wgrad P{P} N{N} K{Kd}"]


# id: (N, Kd, weighted, bias, outer, x trains, forward stages, backward stages)
ROUTED_F32 = {
    "narrow": (40, 24, True, True, 1, True, "combine", "combine"),
    "wide_col_tail": (136, 64, True, True, 1, True, "combine", "combine"),
    "dense_fwd": (256, 64, False, False, 2, True, "dense", "combine"),
    "dense_bwd": (64, 256, False, False, 2, True, "combine", "dense"),
    "unweighted_bias": (40, 24, False, True, 1, True, "combine", "combine"),
    "no_dx": (40, 24, True, True, 1, False, "combine", "skip"),
}


@pytest.mark.parametrize("case", list(ROUTED_F32))
def test_routed_linear_f32(device, case):
    from amk import ops

    N, Kd, weighted, has_bias, outer, x_trains, fwd, bwd = ROUTED_F32[case]
    U, E = 150, 4
    x, logits = _rand((U, Kd), 1, device), _logits(U, E, 2, device)
    W = _rand((E, N, Kd), 3, device, scale=Kd ** -0.5)
    bias = _rand((E, N), 4, device) if has_bias else None
    d_out = _rand((U // outer, N), 5, device)
    grads = ({0} if x_trains else set()) | {1, 2, 3}
    out, ids, (dx, dlogits, dW, db), names = _run(
        lambda a, b, c, d: ops.routed_linear(a, b, c, d, K, K, weighted, outer), [x, logits, W, bias], d_out,
        contextlib.nullcontext(), grads)
    assert names == _routed_events(U, E, N, Kd, outer, K, fwd, bwd)
    want = rebuild_routed_f32(x, logits, W, bias, K, weighted, outer, fwd, bwd, d_out)
    for what, g, w in zip(("out", "ids", "dx", "dlogits", "dW", "db"), (out, ids, dx, dlogits, dW, db), want):
        assert_same(g, w, f"{case} {what}")


def test_routed_linear_sum_in_gemm_stages(device, monkeypatch):
    """AMK_MOE_SUM_IN_GEMM=1: the sums over a row's pairs are f32 atomics in the GEMM's epilogue, so the bits depend on
    the order of arrival; the stages are pinned."""
    from amk import ops

    monkeypatch.setattr(ops, "MOE_SUM_IN_GEMM", True)
    U, E, N, Kd, outer, x_div = 150, 4, 128, 128, 2, 4
    P = U * K
    x, logits = _rand((P // x_div, Kd), 1, device), _logits(U, E, 2, device)
    W = _rand((E, N, Kd), 3, device, scale=Kd ** -0.5)
    d_out = _rand((U // outer, N), 5, device)
    out, _, (dx, dlogits, dW), names = _run(lambda a, b, c: ops.routed_linear(a, b, c, None, K, x_div, False, outer),
                                            [x, logits, W], d_out, contextlib.nullcontext(), {0, 1, 2})
    assert names == [f"moe_route U{U} E{E} k{K}", f"grouped_nt_acc P{P} N{N} K{Kd}", f"grouped_nn_acc P{P} N{N} K{Kd}",
                     f"grouped_wgrad P{P} N{N} K{Kd}"]
    assert out.shape == (U // outer, N) and dx.shape == x.shape and dlogits is None and dW.shape == W.shape


# ---------------------------------------------------------------------------- routed_linear, bf16 autocast
def rebuild_routed_bf16(x, logits, W, bias, x_div, d_out):
    ops, call = _abi()
    dev = x.device
    U, E = logits.shape
    N, Kd = W.shape[1], W.shape[2]
    P = U * K
    x16, w16 = x.to(BF16), W.to(BF16)
    r = ops.moe_route(logits.float(), K)
    ids, gate, off, perm = r["ids"], r["gate"], r["offsets"], r["perm"]
    _tiles_ok(off)
    Y = _new(dev, P, N)
    call("amk_grouped_gemm_nt_bf16", x16, x16.stride(0), x_div, w16, bias, off, perm, P, E, N, Kd, Y)
    out = _new(dev, U, N)
    call("amk_moe_combine", Y, ids, gate, U, 1, K, N, out)
    d16 = d_out.to(BF16)
    dlogits = _new(dev, U, E)
    call("amk_moe_gate_grad", d_out, Y, ids, gate, P, K, E, N, K, dlogits)
    dxp = _new(dev, P, Kd)
    call("amk_grouped_gemm_nn_bf16", d16, N, K, w16, gate, off, perm, P, E, N, Kd, dxp)
    dx = _new(dev, *x.shape)
    call("amk_moe_combine", dxp, ids, None, x.shape[0], x_div // K, K, Kd, dx)
    dW, db = _new(dev, E, N, Kd), _new(dev, E, N)
    call("amk_grouped_gemm_wgrad_bf16", d16, N, K, x16, x16.stride(0), x_div, gate, off, perm, P, E, N, Kd, dW, db)
    return out, ids, dx.to(x.dtype), dlogits.to(logits.dtype), dW, db


@pytest.mark.parametrize("x_dtype", [F32, BF16], ids=["x_f32", "x_bf16"])
def test_routed_linear_bf16_autocast(device, x_dtype):
    from amk import ops

    U, E, N, Kd = 150, 4, 40, 24
    P = U * K
    x, logits = _rand((U, Kd), 1, device, x_dtype), _logits(U, E, 2, device, BF16)
    W, bias = _rand((E, N, Kd), 3, device, scale=Kd ** -0.5), _rand((E, N), 4, device)
    d_out = _rand((U, N), 5, device)
    out, ids, (dx, dlogits, dW, db), names = _run(lambda a, b, c, d: ops.routed_linear(a, b, c, d, K, K), [x, logits, W, bias],
                                                  d_out, torch.autocast("cuda", dtype=BF16), {0, 1, 2, 3})
    assert names == [f"moe_route U{U} E{E} k{K}", f"bf16_grouped_nt P{P} N{N} K{Kd}", f"moe_combine G{U} N{N} x{K}",
                     f"bf16_grouped_nn P{P} N{N} K{Kd}", f"bf16_grouped_wgrad P{P} N{N} K{Kd}"]
    assert (out.dtype, ids.dtype, dx.dtype, dlogits.dtype, dW.dtype, db.dtype) == (F32, torch.int64, x_dtype, BF16, F32, F32)
    want = rebuild_routed_bf16(x, logits, W, bias, K, d_out)
    for what, g, w in zip(("out", "ids", "dx", "dlogits", "dW", "db"), (out, ids, dx, dlogits, dW, db), want):
        assert_same(g, w, f"{what}")


# ---------------------------------------------------------------------------- SwitchHead's two forms
DIM, D_HEAD, H, E_SH, G_SH = 256, 32, 2, 8, 75
U_SH, FAN, PAIRS = G_SH * H, H * K, G_SH * H * K


def rebuild_shared_rows(x, logits, W, d_out, bf16):
    ops, call = _abi()
    dev = x.device
    E, N, Kd = W.shape
    ids, gate = ops._topk(logits.float() if bf16 else logits, K)
    off, perm = ops._route_distinct(ids, G_SH, FAN, E)
    _tiles_ok(off)
    V, out = _new(dev, G_SH * E, N), _new(dev, U_SH, N)
    if bf16:
        x16, w16 = x.to(BF16), W.to(BF16)
        call("amk_grouped_gemm_nt64_bf16", x16, x16.stride(0), E, w16, None, off, perm, G_SH * E, E, N, Kd, V)
    else:
        call("amk_grouped_gemm_nt", x, Kd, E, W, None, off, perm, G_SH * E, E, N, Kd, V)
    call("amk_moe_combine_rows", V, ids, gate, U_SH, 1, K, N, FAN, E, out)
    dlogits, dW = _new(dev, U_SH, E), _new(dev, E, N, Kd)
    call("amk_moe_gate_grad_rows", d_out, V, ids, gate, PAIRS, K, E, N, K, FAN, dlogits)
    if bf16:
        Z16 = _new(dev, G_SH, E * N, dtype=BF16)
        call("amk_moe_expert_sums_bf16", d_out, 0, d_out.stride(0), K, ids, gate, G_SH, FAN, E, N, Z16)
        dx = (Z16 @ w16.view(E * N, Kd)).to(x.dtype)
        call("amk_grouped_gemm_wgrad64_bf16", Z16, N, 1, x16, x16.stride(0), E, None, off, perm, G_SH * E, E, N, Kd, dW)
    else:
        Z = _new(dev, G_SH, E * N)
        call("amk_moe_expert_sums", d_out, d_out.stride(0), K, ids, gate, G_SH, FAN, E, N, Z)
        dx = Z @ W.view(E * N, Kd)
        call("amk_grouped_gemm_wgrad", Z, N, 1, x, Kd, E, None, off, perm, G_SH * E, E, N, Kd, dW, None)
    return out, ids, dx, dlogits.to(logits.dtype), dW


def rebuild_summed(a, logits, W, d_out, bf16):
    ops, call = _abi()
    dev = a.device
    E, N, Kd = W.shape
    ids, _ = ops._topk(logits.float() if bf16 else logits, K)
    if bf16:
        w16 = W.to(BF16)
        Z = _new(dev, G_SH, E * Kd, dtype=BF16)
        call("amk_moe_expert_sums_bf16", a, 0, a.stride(0), K, ids, None, G_SH, FAN, E, Kd, Z)
        out = Z @ w16.permute(0, 2, 1).reshape(E * Kd, N)
    else:
        Z = _new(dev, G_SH, E * Kd)
        call("amk_moe_expert_sums", a, a.stride(0), K, ids, None, G_SH, FAN, E, Kd, Z)
        out = Z @ W.permute(0, 2, 1).reshape(E * Kd, N)
    off, perm = ops._route_distinct(ids, G_SH, FAN, E)
    _tiles_ok(off)
    D, da, dW = _new(dev, G_SH * E, Kd), _new(dev, U_SH, Kd), _new(dev, E, N, Kd)
    if bf16:
        d16 = d_out.to(BF16)
        call("amk_grouped_gemm_nn64_bf16", d16, d16.stride(0), E, w16, None, off, perm, G_SH * E, E, N, Kd, D)
    else:
        call("amk_grouped_gemm_nn", d_out, N, E, W, None, off, perm, G_SH * E, E, N, Kd, D)
    call("amk_moe_combine_rows", D, ids, None, U_SH, 1, K, Kd, FAN, E, da)
    if bf16:
        call("amk_grouped_gemm_wgrad64_bf16", d16, d16.stride(0), E, Z, Kd, 1, None, off, perm, G_SH * E, E, N, Kd, dW)
    else:
        call("amk_grouped_gemm_wgrad", d_out, N, E, Z, Kd, 1, None, off, perm, G_SH * E, E, N, Kd, dW, None)
    return out, ids, da, None, dW


def _shared_events(N, Kd, E, p):
    return [f"moe_topk U{U_SH} E{E} k{K} + distinct lists", f"{p}grouped_nt P{PAIRS} N{N} K{Kd} (distinct rows)",
            f"{p}moe_expert_sums G{G_SH} fan{FAN} E{E} d{N}", f"{p}dense_z_gemm M{G_SH} N{Kd} K{E * N}",
            f"{p}grouped_wgrad P{PAIRS} N{N} K{Kd} (distinct rows)"]


def _summed_events(N, Kd, E, p):
    return [f"moe_topk U{U_SH} E{E} k{K}", f"{p}moe_expert_sums G{G_SH} fan{FAN} E{E} d{Kd}", f"{p}dense_z_gemm M{G_SH} N{N} K{E * Kd}",
            f"{p}grouped_nn P{PAIRS} N{N} K{Kd} (distinct rows)", f"{p}grouped_wgrad P{PAIRS} N{N} K{Kd} (distinct rows)"]


# id: (autocast, the weight trains, the bf16 Functions run)
SWITCHHEAD = {"f32": (False, True, False), "bf16_autocast": (True, True, True), "frozen_weight": (True, False, False)}


@pytest.mark.parametrize("case", list(SWITCHHEAD))
@pytest.mark.parametrize("form", ["shared_row_experts", "summed_experts"])
def test_switchhead_forms(device, form, case):
    from amk import ops

    autocast, w_trains, bf16 = SWITCHHEAD[case]
    assert ops.distinct_experts_ok(DIM, D_HEAD, FAN, E_SH) and ops.switchhead_bf16_shapes(DIM, D_HEAD, FAN, E_SH)
    shared = form == "shared_row_experts"
    N, Kd = (D_HEAD, DIM) if shared else (DIM, D_HEAD)
    a = _rand((G_SH if shared else U_SH, Kd), 1, device)
    logits = _logits(U_SH, E_SH, 2, device)
    W = _rand((E_SH, N, Kd), 3, device, scale=Kd ** -0.5)
    d_out = _rand((U_SH if shared else G_SH, N), 5, device, BF16 if bf16 and not shared else F32)
    amp = torch.autocast("cuda", dtype=BF16) if autocast else contextlib.nullcontext()
    out, ids, (da, dlogits, dW), names = _run(lambda p, q, r: getattr(ops, form)(p, q, r, K, H), [a, logits, W], d_out, amp,
                                              {0, 1} | ({2} if w_trains else set()))
    assert names == (_shared_events if shared else _summed_events)(N, Kd, E_SH, "bf16_" if bf16 else "")
    assert out.dtype == (BF16 if bf16 and not shared else F32) and da.dtype == F32
    want = (rebuild_shared_rows if shared else rebuild_summed)(a, logits, W, d_out, bf16)
    if not w_trains:
        assert dW is None
        want = want[:4] + (None,)
    for what, g, w in zip(("out", "ids", "dx", "dlogits", "dW"), (out, ids, da, dlogits, dW), want):
        assert_same(g, w, f"{form} {case} {what}")
