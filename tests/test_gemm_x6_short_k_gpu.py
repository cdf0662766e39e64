"""The row-block-stationary kernel of csrc/gemm_x6.hip for K <= 256 (gemm_x6_short_k_kernel: amk_gemm_x6_nt,
amk_gemm_x6_nt_swiglu and the two-weight amk_gemm_x6_nt_cols2) against fp64 under the per-element bounds of
tests/gemm_x6_ref.py, and bit for bit against the tile kernel (amk_gemm_x6_short_k(0)), at the smallest shapes where its
structure can go wrong: the 128-row block edge and a ragged last block (M = 1, 63, 65, 130, 333), one partial 32-step, a
partial last 64-k stage, the patch-embedding width and the maximum (K = 4, 36, 192, 256), a single partial column tile, a
ragged last tile and several tiles (N = 4, 132, 516; H = 8, 72, 200), the step's own tile counts at few rows, a strided A.
Every call goes through the C entry points into outputs with 64 sentinel rows behind them, which must stay untouched."""
import contextlib

import pytest
import torch

import dense_f32_ref as R32
import gemm_x6_ref as ref
from test_gemm_x6_fused_gpu import _with_planes, check, dev, make_planes

pytestmark = pytest.mark.gpu

MS = (1, 63, 65, 130, 333)
KS = (4, 36, 192, 256)
SENTINEL = -12345.5
PAD_ROWS = 64


@contextlib.contextmanager
def short_k(on):
    from amk import lib

    L = lib.load()
    old = L.amk_gemm_x6_short_k(int(on))
    try:
        assert L.amk_gemm_x6_short_k(-1) == int(on)
        yield
    finally:
        L.amk_gemm_x6_short_k(old)


def _padded(M, N, device):
    return torch.full((M + PAD_ROWS, N), SENTINEL, device=device)


def _untouched(buf, M, what):
    assert bool((buf[M:] == SENTINEL).all()), f"{what}: rows past M were written"
    return buf[:M]


def raw_nt(a, planes, N, bias=None):
    from amk import dense, lib

    M, K = a.shape
    c = _padded(M, N, a.device)
    rc = lib.load().amk_gemm_x6_nt(dense._p(a), a.stride(0), dense._p(planes), dense._p(bias), dense._p(c), N, M, N, K, dense._stream())
    lib.check(rc, "amk_gemm_x6_nt")
    return _untouched(c, M, "nt")


def raw_swiglu(a, planes, H, bias, keep_ab):
    """(gate, ab): without keep_ab the (a | b) buffer is NOT handed over and must come back as it was."""
    from amk import dense, lib

    M, K = a.shape
    g, ab = _padded(M, H, a.device), _padded(M, 2 * H, a.device)
    rc = lib.load().amk_gemm_x6_nt_swiglu(dense._p(a), a.stride(0), dense._p(planes), dense._p(bias), dense._p(g), H,
                                          dense._p(ab if keep_ab else None), 2 * H, M, H, K, dense._stream())
    lib.check(rc, "amk_gemm_x6_nt_swiglu")
    if not keep_ab:
        assert bool((ab == SENTINEL).all()), "(a | b) was written without keep_ab"
        return _untouched(g, M, "gate"), None
    return _untouched(g, M, "gate"), _untouched(ab, M, "(a | b)")


def raw_cols2(a, p1, N1, p2, N2, expect=0):
    from amk import dense, lib

    M, K = a.shape
    c1, c2 = _padded(M, N1, a.device), _padded(M, N2, a.device)
    rc = lib.load().amk_gemm_x6_nt_cols2(dense._p(a), a.stride(0), dense._p(p1), dense._p(p2), dense._p(c1), N1, dense._p(c2), N2,
                                         M, N1, N2, K, dense._stream())
    if expect:
        assert rc == expect
        return None
    lib.check(rc, "amk_gemm_x6_nt_cols2")
    return _untouched(c1, M, "cols2 first"), _untouched(c2, M, "cols2 second")


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_plain_form(device, M, K):
    for N in (4, 132, 516):
        for family in ref.FAMILIES:
            D = dev(R32.make_nt(family, M, N, K, 31), device)
            (pl,) = make_planes(device, [D["w"].cpu()])
            for bias in (None, D["bias"]):
                want, bound = ref.ref_nt(D["a"], D["w"], bias)
                with short_k(True):
                    got = raw_nt(D["a"], pl.w, N, bias)
                with short_k(False):
                    old = raw_nt(D["a"], pl.w, N, bias)
                check(got, want, bound, f"nt {family} N={N} bias={bias is not None}")
                assert torch.equal(got, old), f"nt {family} N={N} bias={bias is not None}: differs from the tile kernel"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_gate_form(device, M, K):
    for H in (8, 72, 200):
        for family in ref.FAMILIES:
            D = dev(R32.make_swiglu(family, M, H, K, 32), device)
            (pl,) = make_planes(device, [D["w"].cpu()], gates=(0,))
            g, gb, ab, abb = ref.ref_nt_swiglu(D["a"], D["w"], D["bias"])
            with short_k(True):
                gate, kept = raw_swiglu(D["a"], pl.w, H, D["bias"], True)
                only, _ = raw_swiglu(D["a"], pl.w, H, D["bias"], False)
                nob, _ = raw_swiglu(D["a"], pl.w, H, None, False)
            with short_k(False):
                gate0, kept0 = raw_swiglu(D["a"], pl.w, H, D["bias"], True)
                only0, _ = raw_swiglu(D["a"], pl.w, H, D["bias"], False)
                nob0, _ = raw_swiglu(D["a"], pl.w, H, None, False)
            check(gate, g, gb, f"gate {family} H={H}")
            check(kept, ab, abb, f"(a | b) {family} H={H}")
            check(only, g, gb, f"gate alone {family} H={H}")
            g0, gb0, _, _ = ref.ref_nt_swiglu(D["a"], D["w"], None)
            check(nob, g0, gb0, f"gate without bias {family} H={H}")
            for x, y, what in ((gate, gate0, "gate"), (kept, kept0, "(a | b)"), (only, only0, "gate alone"), (nob, nob0, "no bias")):
                assert torch.equal(x, y), f"{what} {family} H={H}: differs from the tile kernel"


def test_workload_widths_at_few_rows(device):
    """22 plane tiles of w12 (H = 1368) and the 12 column tiles of q | kv (N = 512 + 1024) at K = 256, M = 130."""
    M, K, H = 130, 256, 1368
    D = dev(R32.make_swiglu("unit", M, H, K, 33), device)
    (pg,) = make_planes(device, [D["w"].cpu()], gates=(0,))
    E = dev(R32.make_nt("unit", M, 1536, K, 34), device)
    pq, pkv, pall = make_planes(device, [E["w"][:512].cpu(), E["w"][512:].cpu(), E["w"].cpu()])
    with short_k(True):
        new = raw_swiglu(D["a"], pg.w, H, D["bias"], True) + (raw_swiglu(D["a"], pg.w, H, D["bias"], False)[0],
                                                               raw_nt(E["a"], pall.w, 1536, E["bias"])) + raw_cols2(E["a"], pq.w, 512, pkv.w, 1024)
    with short_k(False):
        old = raw_swiglu(D["a"], pg.w, H, D["bias"], True) + (raw_swiglu(D["a"], pg.w, H, D["bias"], False)[0],
                                                               raw_nt(E["a"], pall.w, 1536, E["bias"]),
                                                               raw_nt(E["a"], pq.w, 512), raw_nt(E["a"], pkv.w, 1024))
    for i, (x, y) in enumerate(zip(new, old)):
        assert torch.equal(x, y), f"output {i} differs from the tile kernel"
    g, gb, ab, abb = ref.ref_nt_swiglu(D["a"], D["w"], D["bias"])
    check(new[0], g, gb, "gate at the step's width")
    check(new[1], ab, abb, "(a | b) at the step's width")


@pytest.mark.parametrize("N1,N2", ((4, 8), (132, 260), (512, 1024)))
@pytest.mark.parametrize("K", (36, 256))
@pytest.mark.parametrize("M", (1, 130))
def test_two_weight_launch(device, M, K, N1, N2):
    for family in ref.FAMILIES:
        D = dev(R32.make_nt(family, M, N1 + N2, K, 35), device)
        p1, p2 = make_planes(device, [D["w"][:N1].cpu(), D["w"][N1:].cpu()])
        with short_k(False):
            want = raw_nt(D["a"], p1.w, N1), raw_nt(D["a"], p2.w, N2)
        for on in (True, False):
            with short_k(on):
                got = raw_cols2(D["a"], p1.w, N1, p2.w, N2)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{family} switch={on}"
        ref1, b1 = ref.ref_nt(D["a"], D["w"][:N1])
        check(got[0], ref1, b1, f"cols2 first {family}")


def test_two_weight_launch_past_256(device):
    """K = 260: AMK_EUNSUPPORTED from the C entry; _X6Linear2 takes the two launches."""
    from amk import dense, ops

    M, K, N1, N2 = 130, 260, 128, 256
    D = dev(R32.make_nt("unit", M, N1 + N2, K, 36), device)
    wa, wb = D["w"][:N1].contiguous(), D["w"][N1:].contiguous()
    pa, pb = _with_planes(device, wa, wb)
    for on in (True, False):
        with short_k(on):
            assert raw_cols2(D["a"], pa.w, N1, pb.w, N2, expect=-2) is None
            a, b = ops._X6Linear2.apply(D["a"], wa, wb, pa, pb)
        assert torch.equal(a, dense.gemm_x6_nt(D["a"], pa.w, N1)) and torch.equal(b, dense.gemm_x6_nt(D["a"], pb.w, N2))


def test_strided_rows_and_fallbacks(device):
    from amk import dense

    D = dev(R32.make_swiglu("unit", 130, 68, 36, 37), device)
    wide = torch.randn(130, 100, device=device)
    wide[:, 8:44] = D["a"]
    a = wide[:, 8:44]
    assert a.stride(0) == 100 and a.data_ptr() % 16 == 0
    plg, pln = make_planes(device, [D["w"].cpu(), D["w"].cpu()], gates=(0,))
    out = {}
    for on in (True, False):
        with short_k(on):
            out[on] = (raw_nt(a, pln.w, 136, D["bias"]), raw_nt(D["a"], pln.w, 136, D["bias"]),
                       raw_swiglu(a, plg.w, 68, D["bias"], True)[0], raw_swiglu(D["a"], plg.w, 68, D["bias"], True)[0],
                       raw_cols2(a, pln.w, 136, pln.w, 136)[1], raw_nt(D["a"], pln.w, 136))
        assert torch.equal(out[on][0], out[on][1]) and torch.equal(out[on][2], out[on][3]) and torch.equal(out[on][4], out[on][5])
    for x, y in zip(out[True], out[False]):
        assert torch.equal(x, y)
    want, bound = ref.ref_nt(D["a"], D["w"], D["bias"])
    check(out[True][0], want, bound, "strided nt")
    # the forms the short-K kernel does not take run the tile kernel whatever the switch says
    E = dev(R32.make_nt("unit", 130, 132, 260, 38), device)
    (p260,) = make_planes(device, [E["w"].cpu()])
    F = dev(R32.make_nn("unit", 130, 132, 32, 39, K2=36), device)
    pa, pb = make_planes(device, [F["w"].cpu(), F["w2"].cpu()])
    res = {}
    for on in (True, False):
        with short_k(on):
            res[on] = (raw_nt(E["a"], p260.w, 132, E["bias"]), dense.gemm_x6_nt(F["a"], pa.wt, 132, a2=F["a2"], planes2=pb.wt))
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    want, bound = ref.ref_nt(E["a"], E["w"], E["bias"])
    check(res[True][0], want, bound, "K = 260")


def test_rows_past_m_stay_untouched(device):
    """A ragged row block (M = 130: 2 rows of the second block) in every form; raw_* assert the 64 sentinel rows."""
    D = dev(R32.make_swiglu("unit", 130, 72, 256, 40), device)
    plg, pln = make_planes(device, [D["w"].cpu(), D["w"].cpu()], gates=(0,))
    with short_k(True):
        raw_nt(D["a"], pln.w, 144, D["bias"])
        raw_swiglu(D["a"], plg.w, 72, D["bias"], True)
        raw_swiglu(D["a"], plg.w, 72, D["bias"], False)
        raw_cols2(D["a"], pln.w, 144, pln.w, 144)


def test_functions_bit_equal_with_the_switch_off(device):
    """_X6Linear2 and _X6SwiGLUFFN on kept planes: forward outputs and every gradient, switch on against off."""
    from amk import ops

    M, Dm, H = 130, 256, 72
    g = torch.Generator().manual_seed(41)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(M, Dm).to(device).requires_grad_(True)
    P = {k: v.to(device).requires_grad_(True) for k, v in dict(
        wa=r(128, Dm) * 0.1, wb=r(256, Dm) * 0.1, w12=r(2 * H, Dm) * 0.1, b12=r(2 * H) * 0.1, w3=r(Dm, H) * 0.2, b3=r(Dm)).items()}
    pa, pb, p3 = _with_planes(device, P["wa"], P["wb"], P["w3"])
    (p12,) = _with_planes(device, P["w12"], gate=P["w12"])
    names = sorted(P)

    def run():
        q, kv = ops._X6Linear2.apply(x, P["wa"], P["wb"], pa, pb)
        f = ops._X6SwiGLUFFN.apply(x, P["w12"], P["b12"], P["w3"], P["b3"], p12, p3)
        loss = (q.sum(-1, keepdim=True) * kv).pow(2).sum() * 1e-3 + f.pow(2).sum()
        return [q, kv, f] + list(torch.autograd.grad(loss, [x] + [P[n] for n in names]))

    with short_k(True):
        new = run()
    with short_k(False):
        old = run()
    for n, a, b in zip(["q", "kv", "f", "dx"] + names, new, old):
        assert torch.equal(a, b), n
