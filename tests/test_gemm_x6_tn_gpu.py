"""The split-bf16 weight gradient (csrc/gemm_x6_tn.hip, dense.gemm_x6_tn) against fp64 under the per-element bounds of
tests/gemm_x6_tn_ref.py, at the smallest shapes where it can go wrong: M = 1, 31, 33 (the 32-row step), 127, 333 and the
first M the host code cuts into two chunks; gradients 4 x 4, 68 x 36, 132 x 52 (a second, partial n tile) and 200 x 256 on the
four-wave kernel, 708 x 260 (twelve tiles: partial n and k tiles) on the eight-wave one; two row segments 128 + 68; y as a
column slice; caller buffers pre-filled with NaN.  Then the autograd Functions ops puts on it, against fp64 autograd."""
import ctypes
import functools

import pytest
import torch

import dense_f32_ref as R32
import gemm_x6_tn_ref as T

pytestmark = pytest.mark.gpu

NK = ((4, 4), (68, 36), (132, 52), (200, 256))
MS = (1, 31, 33, 127, 333, T.first_chunked_m(4, 4))
NK8 = (708, 260)
MS8 = (1, 33, 333, T.first_chunked_m(*NK8))


@functools.lru_cache(maxsize=None)
def case(family, M, N, K, N2, cus):
    """(inputs on the CPU, reference with bounds): built once, shared, never written."""
    D = R32.make_tn(family, M, N, K, seed=7 * M + N + K, N2=N2)
    return D, T.ref_tn(D["y"], D["x"], y2=D.get("y2"), geo=T.geometry(M, N + N2, K, cus))


def cus_of(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def check(got, R, name, what):
    nbad, ratio = T.outside(got, R, name)
    print(f"{what} {name}: worst |err| / bound = {ratio:.3f}")
    assert nbad == 0, f"{what} {name}: {nbad} elements outside the bound, worst ratio {ratio:.3f}"


def nan(*shape, device):
    return torch.full(shape, float("nan"), device=device)


def run_case(device, family, M, N, K, N2=0):
    """Both bias settings, fresh and caller-owned (NaN-filled) buffers, twice: every element inside the bound, the buffers
    overwritten, the runs bitwise equal."""
    from amk import dense

    cus = cus_of(device)
    D, R = case(family, M, N, K, N2, cus)
    assert dense.x6_tn_chunks(M, N + N2, K) == T.geometry(M, N + N2, K, cus)[0]
    y, x = D["y"].to(device), D["x"].to(device)
    y2 = D["y2"].to(device) if N2 else None
    what = f"{family} M{M} N{N}+{N2} K{K}"
    dw, dw2, db = dense.gemm_x6_tn(y, x, y2=y2, want_bias=True)
    check(dw, R, "dw", what)
    check(db, R, "db", what)
    if N2:
        check(dw2, R, "dw2", what)
    o, o2, ob = nan(N, K, device=device), (nan(N2, K, device=device) if N2 else None), nan(N + N2, device=device)
    r = dense.gemm_x6_tn(y, x, y2=y2, want_bias=True, out=o, out2=o2, bias_out=ob)
    assert r[0] is o and r[1] is o2 and r[2] is ob
    assert torch.equal(o, dw) and torch.equal(ob, db) and (not N2 or torch.equal(o2, dw2)), f"{what}: not reproducible"
    e, e2, none = dense.gemm_x6_tn(y, x, y2=y2)
    assert none is None and torch.equal(e, dw) and (not N2 or torch.equal(e2, dw2)), f"{what}: dW depends on want_bias"


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K", NK)
def test_every_family_inside_the_bound(device, M, N, K):
    for family in T.FAMILIES:
        run_case(device, family, M, N, K)


@pytest.mark.parametrize("M", MS8)
def test_eight_wave_tile(device, M):
    assert T.tile_k(*NK8) == 256
    for family in T.FAMILIES:
        run_case(device, family, M, *NK8)


@pytest.mark.parametrize("M", (33, MS[-1]))
@pytest.mark.parametrize("K", (36, 256))
def test_two_row_segments(device, M, K):
    for family in T.FAMILIES:
        run_case(device, family, M, 128, K, N2=68)


def test_y_as_a_column_slice(device):
    """y and y2 as column slices of one wider tensor (the dq | dkv views): row stride != width."""
    from amk import dense

    M, K = 333, 52
    cus = cus_of(device)
    D, R = case("unit", M, 128, K, 68, cus)
    wide = torch.randn(M, 128 + 68 + 12, device=device)
    wide[:, 4:132], wide[:, 132:200] = D["y"].to(device), D["y2"].to(device)
    y, y2 = wide[:, 4:132], wide[:, 132:200]
    assert y.stride(0) == 208 and y.data_ptr() % 16 == 0 and y2.data_ptr() % 16 == 0
    dw, dw2, db = dense.gemm_x6_tn(y, D["x"].to(device), y2=y2, want_bias=True)
    for name, got in (("dw", dw), ("dw2", dw2), ("db", db)):
        check(got, R, name, "column slices")
    same = dense.gemm_x6_tn(D["y"].to(device), D["x"].to(device), y2=D["y2"].to(device), want_bias=True)
    assert all(torch.equal(a, b) for a, b in zip((dw, dw2, db), same))
    D1, R1 = case("unit", M, 68, K, 0, cus)
    wide[:, 8:76] = D1["y"].to(device)
    dw, _, db = dense.gemm_x6_tn(wide[:, 8:76], D1["x"].to(device), want_bias=True)
    check(dw, R1, "dw", "one column slice")
    check(db, R1, "db", "one column slice")


def test_unsupported_shapes(device):
    """Outside the preconditions the C ABI answers AMK_EUNSUPPORTED (and launches nothing), and ops keeps such a gradient
    on dense.gemm_tn."""
    from amk import lib, ops

    L = lib.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    y, x, c = torch.zeros(8, 8, device=device), torch.zeros(8, 8, device=device), nan(8, 8, device=device)
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rc(M=8, N=8, K=8, ldy=8, ldx=8, ldc=8, yp=None, split=0):
        return L.amk_gemm_x6_tn(yp or P(y), ldy, null, 0, split, P(x), ldx, P(c), ldc, null, 0, null, M, N, K, null, 0, st)

    assert rc() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(c).any()
    c.fill_(float("nan"))
    assert rc(N=6) == -2 and rc(K=6) == -2 and rc(ldy=6) == -2 and rc(ldx=10) == -2 and rc(ldc=9) == -2
    assert rc(yp=ctypes.c_void_p(y.data_ptr() + 4)) == -2
    assert rc(M=1 << 28, ldy=8) == -2, "an operand of 2 GiB or more"
    assert rc(M=0) == -1 and rc(split=4) == -1
    torch.cuda.synchronize()
    assert torch.isnan(c).all(), "a refused call must write nothing"
    assert ops._x6_tn_ok(8, 8, 8, 8, 8) and not ops._x6_tn_ok(8, 6, 8, 8, 8) and not ops._x6_tn_ok(8, 8, 6, 8, 8)
    assert not ops._x6_tn_ok(8, 8, 8, 6, 8) and not ops._x6_tn_ok(1 << 28, 8, 8, 8, 8)


# ------------------------------------------------------------------------------------------ the autograd Functions
def _layers(device):
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g)
    M, Dm, H = 200, 132, 68
    x = r(2, M // 2, Dm).to(device).requires_grad_(True)
    P = {k: torch.nn.Parameter(v.to(device)) for k, v in dict(
        w=r(132, Dm) * 0.2, b=r(132), wa=r(128, Dm) * 0.2, wb=r(256, Dm) * 0.2, w12=r(2 * H, Dm) * 0.2, b12=r(2 * H) * 0.1,
        w3=r(Dm, H) * 0.2, b3=r(Dm)).items()}
    return x, P


def _loss(x, P, lin, lin2, ffn):
    y = lin(x, P["w"], P["b"])
    q, kv = lin2(x, P["wa"], P["wb"])
    f = ffn(x, P["w12"], P["b12"], P["w3"], P["b3"])
    return y.pow(2).sum() + (q.sum(-1, keepdim=True) * kv).pow(2).sum() * 1e-3 + f.pow(2).sum()


def _ffn64(x, w12, b12, w3, b3):
    F = torch.nn.functional
    a, b = F.linear(x, w12, b12).chunk(2, -1)
    return F.linear(F.silu(a) * b, w3, b3)


def _counted(monkeypatch):
    from amk import dense

    calls, orig = [], dense.gemm_x6_tn
    monkeypatch.setattr(dense, "gemm_x6_tn", lambda *a, **k: (calls.append(a[0].shape), orig(*a, **k))[1])
    return calls


def _planes_on(device, P):
    from test_gemm_x6_fused_gpu import _with_planes

    _with_planes(device, P["w"], P["wa"], P["wb"], P["w3"], transposed=False)
    _with_planes(device, P["w12"], gate=P["w12"], transposed=False)


@pytest.mark.parametrize("form_on", [True, False])
def test_functions_against_fp64_autograd(device, monkeypatch, form_on):
    """_X6Linear, _X6Linear2 and _X6SwiGLUFFN: with the "dw" form on, the five weight-gradient launches of the backward run on
    dense.gemm_x6_tn and every gradient agrees with fp64 autograd at the f32 level; with it off the kernel is never called."""
    from amk import ops
    from util import assert_close

    monkeypatch.setattr(ops, "GEMM_MODE", "auto")
    monkeypatch.setattr(ops, "X6_LINEAR", True)
    monkeypatch.setattr(ops, "X6_AUTO_FORMS", frozenset(("fwd", "dw") if form_on else ("fwd",)))
    x, P = _layers(device)
    names = sorted(P)
    F = torch.nn.functional
    x64, P64 = x.detach().double().requires_grad_(True), {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    want = torch.autograd.grad(_loss(x64, P64, F.linear, lambda x, a, b: (F.linear(x, a), F.linear(x, b)), _ffn64),
                               [x64] + [P64[n] for n in names])
    _planes_on(device, P)
    calls = _counted(monkeypatch)
    got = torch.autograd.grad(_loss(x, P, ops.linear, ops.linear2, ops.swiglu_ffn), [x] + [P[n] for n in names])
    assert len(calls) == (4 if form_on else 0), calls   # Linear, q | kv (one launch), w3, w12
    for n, a, b in zip(["dx"] + names, got, want):
        assert_close(a, b, 3e-6, n)


def test_unsupported_gradient_takes_the_f32_kernel(device, monkeypatch):
    from amk import dense, ops

    monkeypatch.setattr(ops, "GEMM_MODE", "auto")
    monkeypatch.setattr(ops, "X6_LINEAR", True)
    monkeypatch.setattr(ops, "X6_AUTO_FORMS", frozenset(("fwd", "dw")))
    monkeypatch.setattr(ops, "_x6_tn_ok", lambda *a: False)
    x, P = _layers(device)
    _planes_on(device, P)
    calls, f32 = _counted(monkeypatch), []
    orig = dense.gemm_tn
    monkeypatch.setattr(dense, "gemm_tn", lambda *a, **k: (f32.append(1), orig(*a, **k))[1])
    _loss(x, P, ops.linear, ops.linear2, ops.swiglu_ffn).backward()
    assert not calls and len(f32) == 4


def test_bucket_views_receive_the_same_bits(device, monkeypatch):
    """GradReducer(direct_grads=True): the gradients written straight into the bucket views equal, bit for bit, the
    tensors the same backward returns to autograd without a reducer."""
    from amk import ops
    from amk.dp import GradReducer

    monkeypatch.setattr(ops, "GEMM_MODE", "auto")
    monkeypatch.setattr(ops, "X6_LINEAR", True)
    monkeypatch.setattr(ops, "X6_AUTO_FORMS", frozenset(("fwd", "dw")))
    x, P = _layers(device)
    names = sorted(P)
    _planes_on(device, P)
    plain = torch.autograd.grad(_loss(x, P, ops.linear, ops.linear2, ops.swiglu_ffn), [P[n] for n in names])
    red = GradReducer([P[n] for n in names], direct_grads=True)
    if not red.direct_grads:
        pytest.skip("AMK_DIRECT_GRADS=0 in the environment")
    _planes_on(device, P)   # (the reducer may have moved the parameters: fresh planes for their current versions)
    calls = _counted(monkeypatch)
    red.begin(sync=True)
    _loss(x, P, ops.linear, ops.linear2, ops.swiglu_ffn).backward()
    red.finish(detach_unused=False)
    assert len(calls) == 4
    assert sum(sum(bk.direct) for bk in red.buckets) == len(names)
    views = {v.data_ptr() for bk in red.buckets for v in bk.views}
    for n, g in zip(names, plain):
        assert P[n].grad.data_ptr() in views, n
        assert torch.equal(P[n].grad, g), n
