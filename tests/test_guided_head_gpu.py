"""amk_cfg_layernorm_bf16 and amk_gemm_bf16_f32out on the GPU, element by element against the fp64 references and bounds
of tests/guided_head_ref.py: the LayerNorm at the NCH switch points of the mixed LayerNorm's dispatch and a row count
that leaves a partial last workgroup, with f32 rows, bf16 rows and without the second row, at guidance scales 3, 1 and 0;
the GEMM at the tile and k-step edges of the bf16 GEMM tests, with and without a bias, into a canvas wider than the
result.  Plus the refusals (nothing written) and ops.guided_logits's launches.

The GEMM has two stores, chosen by AMK_GEMM16_F32OUT at every call (csrc/gemm_bf16.hip:574-599): unset, the result goes
through LDS; "direct", every lane stores 16 bytes straight from its accumulators (gemm_bf16_kernel<false, 4>).  The GEMM
test and the op test run under both: the tests of the default store keep their names, their twins end in _direct_store.
Shapes, families, bounds and the canvas check are the same -- with ldc = N + 12 the canvas is where a direct store that
ran past a row's end would show."""
import ctypes

import pytest
import torch

import guided_head_ref as ref

pytestmark = pytest.mark.gpu

# (3, 1028): NCH = 8 of AMK_MX_DISPATCH (csrc/mixed_bf16.hip:300-307), which no other width here selects
LN_SHAPES = [(1, 4), (5, 252), (257, 260), (64, 1024), (3, 4096), (3, 1028)]
GEMM_SHAPES = [(1, 136, 1368), (127, 8, 24), (128, 1024, 8), (129, 120, 40), (383, 264, 96)]
EINVAL, EUNSUPPORTED = -1, -2
STORE_ENV = "AMK_GEMM16_F32OUT"


def _set_store(monkeypatch, store):
    """store None: the variable unset (the default store through LDS); "direct": the direct store."""
    if store is None:
        monkeypatch.delenv(STORE_ENV, raising=False)
    else:
        monkeypatch.setenv(STORE_ENV, store)


def _P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _L():
    from amk import lib

    return lib.load()


def _cfg_ln(device, hc, hn, gamma, beta, s, bf16, n_bf16=None):
    """The kernel's y (M, D) bf16 through the C ABI, written into a NaN canvas with one more row (which must stay NaN).
    bf16: the dtype of both rows; n_bf16: that of the second row where it differs."""
    from amk import lib

    n_bf16 = bf16 if n_bf16 is None else n_bf16
    M, D = hc.shape
    c = hc.to(device=device, dtype=torch.bfloat16 if bf16 else torch.float32)
    n = hn.to(device=device, dtype=torch.bfloat16 if n_bf16 else torch.float32) if hn is not None else None
    g, b = gamma.to(device), beta.to(device)
    y = torch.full((M + 1, D), float("nan"), device=device, dtype=torch.bfloat16)
    rc = _L().amk_cfg_layernorm_bf16(_P(c), int(bf16), _P(n), int(n_bf16), _P(g), _P(b), s, M, D, ref.LN_EPS, _P(y), _S())
    lib.check(rc, "amk_cfg_layernorm_bf16")
    torch.cuda.synchronize()
    assert torch.isnan(y[M].float()).all(), "wrote past its M rows"
    return y[:M]


@pytest.mark.parametrize("M,D", LN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("family", ref.LN_FAMILIES)
@pytest.mark.parametrize("inputs", ["f32", "bf16", "one"])
def test_cfg_layernorm_bounds(device, family, M, D, inputs):
    bf16 = inputs == "bf16"
    hc, hn, gamma, beta = ref.make_cfg_ln(family, M, D, 100 + D, bf16=bf16)
    if inputs == "one":
        hn = None
    one = _cfg_ln(device, hc, None, gamma, beta, 3.0, bf16)
    for s in (3.0, 1.0, 0.0):
        y = _cfg_ln(device, hc, hn, gamma, beta, s, bf16)
        ok = ref.inside(y, ref.ref_cfg_ln(hc, hn, gamma, beta, s))
        assert ok.all(), f"{family} M{M} D{D} {inputs} s={s}: {int((~ok).sum())} of {ok.numel()} elements outside the interval"
        if s == 1.0 or hn is None:
            assert torch.equal(y, one), f"s={s}: not bitwise the one-input kernel"


@pytest.mark.parametrize("M,D", LN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("c_bf16", [True, False], ids=["bf16_f32", "f32_bf16"])
def test_cfg_layernorm_bounds_rows_of_two_dtypes(device, M, D, c_bf16):
    """The two rows in different dtypes -- cfg_ln_bf16_kernel<NCH, true, false, true> and <NCH, false, true, true>, the
    `cb` / `nb` branches of csrc/mixed_bf16.hip:349-350, which rows of one dtype never take -- at every NCH, held to the
    same intervals: both rows hold bf16 values, so the reference is that of the bf16 case."""
    for family in ref.LN_FAMILIES[:2]:
        hc, hn, gamma, beta = ref.make_cfg_ln(family, M, D, 100 + D, bf16=True)
        for s in (3.0, 0.0):
            y = _cfg_ln(device, hc, hn, gamma, beta, s, c_bf16, n_bf16=not c_bf16)
            ok = ref.inside(y, ref.ref_cfg_ln(hc, hn, gamma, beta, s))
            assert ok.all(), f"{family} M{M} D{D} s={s}: {int((~ok).sum())} of {ok.numel()} elements outside the interval"
            assert torch.equal(y, _cfg_ln(device, hc, hn, gamma, beta, s, True)), "not bitwise the kernel on two bf16 rows"


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_cfg_layernorm_row_is_independent_of_m(device, bf16):
    hc, hn, gamma, beta = ref.make_cfg_ln("outlier_rows", 257, 260, 7, bf16=bf16)
    full = _cfg_ln(device, hc, hn, gamma, beta, 3.0, bf16)
    row0 = _cfg_ln(device, hc[:1], hn[:1], gamma, beta, 3.0, bf16)
    assert torch.equal(full[:1], row0)


def _gemm(device, a, w, bias, pad=0, poison=float("nan")):
    """c (M, N) f32 through the C ABI into a canvas with `pad` more columns and one more row, all poisoned."""
    from amk import lib

    M, K = a.shape
    N = w.shape[0]
    ad, wd = a.to(device=device, dtype=torch.bfloat16), w.to(device=device, dtype=torch.bfloat16)
    bd = bias.to(device) if bias is not None else None
    c = torch.full((M + 1, N + pad), poison, device=device, dtype=torch.float32)
    rc = _L().amk_gemm_bf16_f32out(_P(ad), K, _P(wd), K, _P(bd), _P(c), N + pad, M, N, K, _S())
    lib.check(rc, "amk_gemm_bf16_f32out")
    torch.cuda.synchronize()
    return c


def _gemm_cases(fn):
    for mark in (pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"]),
                 pytest.mark.parametrize("family", ref.GEMM_FAMILIES),
                 pytest.mark.parametrize("M,N,K", GEMM_SHAPES, ids=lambda v: str(v))):
        fn = mark(fn)
    return fn


@_gemm_cases
def test_gemm_f32out_bounds(device, monkeypatch, family, M, N, K, with_bias):
    _gemm_f32out_bounds(device, monkeypatch, None, family, M, N, K, with_bias)


@_gemm_cases
def test_gemm_f32out_bounds_direct_store(device, monkeypatch, family, M, N, K, with_bias):
    _gemm_f32out_bounds(device, monkeypatch, "direct", family, M, N, K, with_bias)


def _gemm_f32out_bounds(device, monkeypatch, store, family, M, N, K, with_bias):
    _set_store(monkeypatch, store)
    a, w, b = ref.make_gemm(family, M, N, K, 300 + K)
    bias = b if with_bias else None
    c = _gemm(device, a, w, bias, pad=12)
    rest = torch.ones_like(c, dtype=torch.bool)
    rest[:M, :N] = False
    assert torch.isnan(c[rest]).all(), f"store {store}: wrote outside its result region (ldc > N)"
    bad = ref.outside_gemm(c[:M, :N], ref.ref_gemm_f32(a, w, bias))
    assert bad == 0, f"{family} {M}x{N}x{K} store {store}: {bad} elements outside n u32 S"


def test_refusals_write_nothing(device):
    L = _L()
    f32 = dict(device=device, dtype=torch.float32)
    g, b = torch.ones(64, **f32), torch.zeros(64, **f32)
    h = torch.randn(4, 64, **f32)
    y = torch.full((4, 64), float("nan"), device=device, dtype=torch.bfloat16)
    null = ctypes.c_void_p(0)
    assert L.amk_cfg_layernorm_bf16(_P(h), 0, null, 0, _P(g), _P(b), 3.0, 4, 62, 1e-5, _P(y), _S()) == EUNSUPPORTED       # D % 4
    assert L.amk_cfg_layernorm_bf16(_P(h), 0, null, 0, _P(g), _P(b), 3.0, 4, 4100, 1e-5, _P(y), _S()) == EUNSUPPORTED     # D > 4096
    off = ctypes.c_void_p(h.data_ptr() + 4)
    assert L.amk_cfg_layernorm_bf16(off, 0, null, 0, _P(g), _P(b), 3.0, 3, 60, 1e-5, _P(y), _S()) == EINVAL              # misaligned
    assert L.amk_cfg_layernorm_bf16(_P(h), 0, off, 0, _P(g), _P(b), 3.0, 3, 60, 1e-5, _P(y), _S()) == EINVAL
    a = torch.randn(8, 48, device=device).bfloat16()
    w = torch.randn(16, 48, device=device).bfloat16()
    c = torch.full((8, 16), float("nan"), **f32)
    assert L.amk_gemm_bf16_f32out(_P(a), 48, _P(w), 48, null, _P(c), 16, 8, 16, 44, _S()) == EUNSUPPORTED               # K % 8
    assert L.amk_gemm_bf16_f32out(_P(a), 48, _P(w), 48, null, _P(c), 16, 8, 12, 48, _S()) == EUNSUPPORTED               # N % 8
    assert L.amk_gemm_bf16_f32out(_P(a), 48, _P(w), 48, null, _P(c), 18, 8, 16, 48, _S()) == EUNSUPPORTED               # ldc % 4
    assert L.amk_gemm_bf16_f32out(ctypes.c_void_p(a.data_ptr() + 2), 48, _P(w), 48, null, _P(c), 16, 7, 16, 40, _S()) == EINVAL
    assert L.amk_gemm_bf16_f32out(_P(a), 48, _P(w), 48, null, ctypes.c_void_p(c.data_ptr() + 4), 16, 7, 8, 48, _S()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(y.float()).all() and torch.isnan(c).all(), "a refused call wrote"


def test_guided_logits_op(device, monkeypatch):
    _guided_logits_op(device, monkeypatch, None)


def test_guided_logits_op_direct_store(device, monkeypatch):
    _guided_logits_op(device, monkeypatch, "direct")


def _guided_logits_op(device, monkeypatch, store):
    """Under autocast: exactly the two kernels, the result bitwise the two C calls' and within the bounds; outside autocast
    the gate is False."""
    from amk import ops

    _set_store(monkeypatch, store)

    M, D, V = 150, 64, 256
    hc, hn, gamma, beta = ref.make_cfg_ln("unit", M, D, 60)
    w = (torch.randn(V, D, generator=torch.Generator().manual_seed(61)) * 0.05).to(device)
    hcd, hnd, gd, bd = (t.to(device) for t in (hc, hn, gamma, beta))
    assert not ops.guided_logits_ok(hcd, w)
    ops.KERNEL_EVENTS = {}
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            assert ops.guided_logits_ok(hcd, w)
            assert not ops.guided_logits_ok(hcd, w.bfloat16()) and not ops.guided_logits_ok(hc, w.cpu())
            got = ops.guided_logits(hcd.view(3, 50, D), gd, bd, w, null_h=hnd.view(3, 50, D), cfg_scale=3.0)
            plain = ops.guided_logits(hcd, gd, bd, w, w16=w.bfloat16())
        torch.cuda.synchronize()
        names = sorted(ops.KERNEL_EVENTS)
        counts = [len(ops.KERNEL_EVENTS[n]) for n in names]
    finally:
        ops.KERNEL_EVENTS = None
    assert names == [f"cfg_layernorm_bf16 M{M} D{D}", f"gemm_bf16_f32out N{V} K{D}"] and counts == [2, 2], (names, counts)
    assert got.dtype == torch.float32 and got.shape == (3, 50, V) and plain.shape == (M, V)
    u = _cfg_ln(device, hc, hn, gamma, beta, 3.0, False)
    assert ref.inside(u, ref.ref_cfg_ln(hc, hn, gamma, beta, 3.0)).all()
    w16 = w.bfloat16()
    c = _gemm(device, u.float().cpu(), w16.float().cpu(), None)[:M]
    assert torch.equal(got.view(M, V), c)
    assert ref.outside_gemm(c, ref.ref_gemm_f32(u.float().cpu(), w16.float().cpu())) == 0
    assert torch.equal(plain, _gemm(device, _cfg_ln(device, hc, None, gamma, beta, 1.0, False).float().cpu(), w16.float().cpu(), None)[:M])
