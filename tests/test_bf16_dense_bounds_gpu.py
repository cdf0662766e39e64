"""The bf16 GEMMs (csrc/gemm_bf16.hip) and the mixed-precision element-wise kernels (csrc/mixed_bf16.hip) held element
by element to the error bounds of tests/bf16_dense_ref.py, at the edges the source defines: 128-row and 128-column
tiles (64 gate columns with the SwiGLU epilogue) over 32-deep K steps padded to an even count, the TN kernel's 64-row
steps, chunks and both tile_k instantiations, the AMK_MX_DISPATCH widths of the mixed LayerNorm and the row wrap of its
capped grids, the element-wise SwiGLU past its 8192-block grid; on unit, outlier-row, binade, cancelling and saturating
inputs (LayerNorm: offset, constant and spike rows too).  The f32 outputs keep the global 2e-5 check as well.
Plus what a tolerance cannot see: every C entry point writing exactly its result region of a NaN canvas with an extra
row and a leading dimension wider than the result (bitwise the amk.dense / amk.ops result), row results independent
of the tile position and the neighbouring rows (bitwise), and ops.swiglu_ffn, ops.linear and
ops.add_layer_norm(branch=True) under autocast bitwise the sequence of calls they document, forward and every gradient.
Wall time on an MI355X about 20 s, mostly the fp64 references on the CPU.

AMK_BF16_DENSE_BOUND_REPORT=<file>: write the worst |got - ref| / bound per kernel output over this module to that JSON
file."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import bf16_dense_ref as ref
from util import rel_err

pytestmark = pytest.mark.gpu
GF, LF = ref.GEMM_FAMILIES, ref.LN_FAMILIES


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("AMK_BF16_DENSE_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(ref.WORST, f, indent=1, sort_keys=True)


def _P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _L():
    from amk import lib

    return lib.load()


def _chk(rc, what):
    from amk import lib

    lib.check(rc, what)


def _b16(t, device):
    return t.to(device=device, dtype=torch.bfloat16)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows(M, block=4096):
    return [(r, min(M, r + block)) for r in range(0, M, block)]


# ---------------------------------------------------------------------------------------------- NT / NN
GEMM_CASES = [(1, 136, 1368), (127, 8, 24), (128, 1024, 8), (129, 120, 40), (383, 264, 96), (1000, 128, 256),
              (129, 136, 32), (383, 1024, 64)]


@pytest.mark.parametrize("i,M,N,K", [(i,) + c for i, c in enumerate(GEMM_CASES)], ids=lambda x: str(x))
@pytest.mark.parametrize("nn", [False, True], ids=["nt", "nn"])
def test_gemm_bounds(device, i, M, N, K, nn):
    from amk import dense

    fam = GF[(i + 2 * nn) % len(GF)]
    a, w, b = ref.make_gemm(fam, M, N, K, 40 + i, nn=nn)
    b = None if nn or i % 2 else b
    if nn:
        out = dense.gemm_nn_bf16(_b16(a, device), _b16(w, device))
    else:
        out = dense.gemm_nt_bf16(_b16(a, device), _b16(w, device), None if b is None else b.to(device))
    assert out.dtype == torch.bfloat16 and out.shape == (M, N)
    ref.assert_within({"c": out}, ref.ref_gemm(a, w, b, nn), ("c",), f"{'nn' if nn else 'nt'} {fam} {M}x{N}x{K}",
                      key="nn" if nn else "nt")


# ---------------------------------------------------------------------------------------------- SwiGLU forward / backward
SW_CASES = [(1, 8, 40), (127, 56, 24), (128, 64, 256), (129, 72, 8), (383, 104, 96), (1000, 1368, 256), (300, 104, 1368)]


def _check_swiglu_fwd(device, fam, M, H, K, keep, seed):
    from amk import dense

    a, w12, b12 = ref.make_swiglu(fam, M, H, K, seed)
    g, ab = dense.gemm_nt_swiglu_bf16(_b16(a, device), _b16(w12, device), b12.to(device), keep_ab=keep)
    assert g.shape == (M, H) and (ab is not None) == keep
    assert not torch.isnan(g).any(), "a saturated gate must give +-0, not NaN"
    for r0, r1 in _rows(M):
        R = ref.ref_swiglu_fwd(a[r0:r1], w12, b12)
        got = {"g": g[r0:r1]}
        if keep:
            got["ab"] = ab[r0:r1]
        ref.assert_within(got, R, tuple(got), f"swiglu fwd {fam} {M}x{H}x{K} rows {r0}:{r1}", key="swiglu_fwd")
    return a, g


@pytest.mark.parametrize("i,M,H,K", [(i,) + c for i, c in enumerate(SW_CASES)], ids=lambda x: str(x))
def test_swiglu_fwd_bounds(device, i, M, H, K):
    fam = GF[i % len(GF)]
    _check_swiglu_fwd(device, fam, M, H, K, i % 3 != 1, 60 + i)


@pytest.mark.parametrize("M,H,K", [(300, 104, 40), (129, 1368, 256)])
def test_swiglu_fwd_saturate(device, M, H, K):
    """Gates over +-300: exp2 overflows to inf below a = -88.7 and the gate must come out +-0 there."""
    a, g = _check_swiglu_fwd(device, "saturate", M, H, K, True, 7)
    pre = ref.ref_swiglu_fwd(a, *ref.make_swiglu("saturate", M, H, K, 7)[1:])["ab"][:, :H]
    assert (pre < -100).any() and (g.cpu()[pre < -100] == 0).all()


def _check_swiglu_bwd(device, fam, M, H, K, seed):
    from amk import dense

    dy, w3, ab = ref.make_swiglu_bwd(fam, M, H, K, seed)
    dab = dense.gemm_nn_swiglu_bwd_bf16(_b16(dy, device), _b16(w3, device), _b16(ab, device))
    assert dab.shape == (M, 2 * H) and not torch.isnan(dab).any()
    for r0, r1 in _rows(M):
        ref.assert_within({"dab": dab[r0:r1]}, ref.ref_swiglu_bwd(dy[r0:r1], w3, ab[r0:r1]), ("dab",),
                          f"swiglu bwd {fam} {M}x{H}x{K} rows {r0}:{r1}", key="swiglu_bwd")


SWB_CASES = [(1, 8, 24), (127, 56, 40), (128, 64, 8), (129, 72, 256), (383, 104, 96), (1000, 1368, 256), (300, 104, 1368)]


@pytest.mark.parametrize("i,M,H,K", [(i,) + c for i, c in enumerate(SWB_CASES)], ids=lambda x: str(x))
def test_swiglu_bwd_bounds(device, i, M, H, K):
    _check_swiglu_bwd(device, GF[(i + 3) % len(GF)], M, H, K, 80 + i)


def test_swiglu_step_size(device):
    """The step's own shape (M = 32768 tokens, D = 256, H = 1368), both directions."""
    _check_swiglu_fwd(device, "outlier_rows", 32768, 1368, 256, True, 3)
    _check_swiglu_bwd(device, "unit", 32768, 1368, 256, 4)


# ---------------------------------------------------------------------------------------------- TN
TN_CASES = [(1, 8, 8), (63, 120, 136), (64, 128, 128), (65, 136, 264), (1000, 256, 256), (1000, 1024, 512),
            (40000, 128, 128), (40000, 264, 136), (4096, 2736, 256)]


def _tn_kernel_names(device, y, x):
    from torch.profiler import ProfilerActivity, profile

    from amk import dense

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = dense.gemm_tn_bf16(y, x, want_bias=True)
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if "gemm_tn_bf16_kernel" in e.name]


@pytest.mark.parametrize("i,M,N,K", [(i,) + c for i, c in enumerate(TN_CASES)], ids=lambda x: str(x))
def test_tn_bounds(device, i, M, N, K):
    fam = GF[i % 4]
    y, x = ref.make_tn(fam, M, N, K, 100 + i)
    (dw, db), names = _tn_kernel_names(device, _b16(y, device), _b16(x, device))
    tk = ref.tn_tile_k(N, K)
    assert names and all(f"<2, {tk // 64}>" in n or f"ILi2ELi{tk // 64}E" in n for n in names), (tk, names)
    R = ref.ref_tn(y, x, _cus())
    ref.assert_within({"dw": dw, "db": db}, R, ("dw", "db"), f"tn {fam} {M}x{N}x{K}", key="tn")
    assert rel_err(dw, R["dw"]) < 2e-5 and rel_err(db, R["db"]) < 2e-5


def test_tn_covers_both_tile_widths():
    wide = [c for c in TN_CASES if ref.tn_tile_k(c[1], c[2]) == 256]
    narrow = [c for c in TN_CASES if ref.tn_tile_k(c[1], c[2]) == 128 and c[2] >= 256]
    assert wide and narrow


# ---------------------------------------------------------------------------------------------- mixed LayerNorm
LN_DS = (4, 252, 256, 260, 512, 516, 1024, 2048, 2052, 4096)


def _ln_abi(device, x, res, gamma, beta, dy, dh_in, x_bf16, extra=0):
    """Forward + backward through the C ABI; extra > 0: into NaN canvases with `extra` more rows.
    -> ({h, y, mean, rstd, dh, dh16, dgamma, dbeta}, canvases)"""
    L = _L()
    M, D = x.shape
    xd = _b16(x, device) if x_bf16 else x.to(device)
    rd = res.to(device) if res is not None else None
    g, b = gamma.to(device), beta.to(device)
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), device=device, dtype=dt)
    h, y, mean, rstd = nan(M + extra, D), nan(M + extra, D, dt=torch.bfloat16), nan(M + extra), nan(M + extra)
    _chk(L.amk_add_layernorm_mixed_fwd(_P(xd), int(x_bf16), _P(rd), _P(g), _P(b), M, D, ref.LN_EPS, _P(h), _P(y), _P(mean),
                                       _P(rstd), _S()), "mixed ln fwd")
    out = {"h": h[:M], "y": y[:M], "mean": mean[:M], "rstd": rstd[:M]}
    canv = {"h": h, "y": y, "mean": mean, "rstd": rstd}
    if dy is not None:
        dyb = dy.dtype == torch.bfloat16
        dyd = dy.to(device)
        dhi = dh_in.to(device) if dh_in is not None else None
        P = L.amk_rowsum_num_partials(M)
        dh, dh16, part = nan(M + extra, D), nan(M + extra, D, dt=torch.bfloat16), nan(P + extra, 2, D)
        _chk(L.amk_add_layernorm_mixed_bwd(_P(dyd), int(dyb), _P(h), _P(dhi), _P(g), _P(mean), _P(rstd), M, D, _P(dh),
                                           _P(dh16), _P(part), _S()), "mixed ln bwd")
        dgb = part[:P].sum(0)
        out.update({"dh": dh[:M], "dh16": dh16[:M], "dgamma": dgb[0], "dbeta": dgb[1]})
        canv.update({"dh": dh, "dh16": dh16, "part": part})
    torch.cuda.synchronize()
    return out, canv


def _ln_cases():
    out = []
    for i, D in enumerate(LN_DS):
        out.append((i, 96 + 37 * (i % 3), D, LF[i % len(LF)], (bool(i % 2), i % 4 < 2), i % 3 != 0, i % 4 != 3))
    out += [(20, 66000, 4, "unit", (True, True), True, True), (21, 9000, 256, "offset", (False, True), False, True),
            (22, 300, 1024, "spike", (True, True), True, False), (23, 200, 512, "constant", (True, False), True, True),
            (24, 150, 2052, "offset", (True, True), True, True)]
    # instances the list above leaves out (AMK_MX_DISPATCH's NCH, csrc/mixed_bf16.hip:300-307, with the forward's x / residual
    # flags, :322-325, and the backward's dy / dh_in flags, :371-374), each at the smallest width of its NCH and few rows:
    # forward <16, bf16 x, no residual>; backward with an f32 dy <1, no dh_in>, <2, dh_in>, <4, no>, <8, dh_in>, <8, no>, <16, no>
    # (no `constant` rows with a residual: their dgamma is identically zero and the test's relative figure has no scale)
    out += [(25, 37, 2052, "unit", (True, False), False, False), (26, 37, 4, "spike", (False, True), False, False),
            (27, 37, 260, "offset", (True, True), False, True), (28, 37, 516, "unit", (False, False), False, False),
            (29, 37, 1028, "spike", (True, True), False, True), (30, 37, 1028, "unit", (False, True), False, False)]
    return out


@pytest.mark.parametrize("case", _ln_cases(), ids=lambda c: f"{c[0]}-M{c[1]}D{c[2]}-{c[3]}-x{'b' if c[4][0] else 'f'}"
                         f"{'-res' if c[4][1] else ''}-dy{'b' if c[5] else 'f'}{'-dhin' if c[6] else ''}")
def test_ln_mixed_bounds(device, case):
    i, M, D, fam, (x_bf16, residual), dy_bf16, with_dh_in = case
    x, res, gamma, beta, cy, ch = ref.make_ln(fam, M, D, 200 + i, x_bf16=x_bf16)
    res = res if residual else None
    dy = cy.bfloat16() if dy_bf16 else cy
    dh_in = ch if with_dh_in else None
    got, _ = _ln_abi(device, x, res, gamma, beta, dy, dh_in, x_bf16)
    R = ref.ref_ln(x, res, gamma, beta, cy, dh_in)
    ref.assert_within(got, R, ("h", "y", "mean", "rstd", "dh", "dh16", "dgamma", "dbeta"), f"mixed ln {fam} M{M} D{D}",
                      key="ln_mixed")
    # (offset rows: the f32 h at 1e3 carries 1e3 u32 = 6e-5 of a spread of 1, so dgamma = sum dy xhat cannot meet 2e-5 of
    # its maximum there; the per-element bound above accounts for that rounding)
    for n in ("h", "dh", "dbeta") + (("dgamma",) if fam != "offset" else ()):
        assert rel_err(got[n], R[n]) < 2e-5, n


# ---------------------------------------------------------------------------------------------- mixed SwiGLU
MX_CASES = [(7, 8), (130, 64), (1000, 1368), (3000, 3000), (64, 104)]


@pytest.mark.parametrize("i,M,H", [(i,) + c for i, c in enumerate(MX_CASES)], ids=lambda x: str(x))
def test_swiglu_mixed_bounds(device, i, M, H):
    fam = GF[i % len(GF)]
    ab, cot = ref.make_ab_cot(fam, M, H, 300 + i)
    L = _L()
    abd, cd = _b16(ab, device), _b16(cot, device)
    g, dab = torch.empty(M, H, device=device, dtype=torch.bfloat16), torch.empty(M, 2 * H, device=device, dtype=torch.bfloat16)
    _chk(L.amk_swiglu_bf16_fwd(_P(abd), M, H, _P(g), _S()), "swiglu fwd")
    _chk(L.amk_swiglu_bf16_bwd(_P(abd), _P(cd), M, H, _P(dab), _S()), "swiglu bwd")
    assert M * H // 4 > 8192 * 256 or i != 3, "the case past the grid cap"
    ref.assert_within({"g": g, "dab": dab}, ref.ref_swiglu_mixed(ab, cot), ("g", "dab"), f"mixed swiglu {fam} {M}x{H}",
                      key="swiglu_mixed")


# ---------------------------------------------------------------------------------------------- sentinel canvas
def _canvas(rows, cols, dtype, device):
    return torch.full((rows, cols), float("nan"), device=device, dtype=dtype)


def _exact_region(canvas, result, what):
    M, N = result.shape
    assert torch.equal(canvas[:M, :N], result), f"{what}: result region differs from the amk.dense / amk.ops result"
    rest = torch.ones_like(canvas, dtype=torch.bool)
    rest[:M, :N] = False
    assert torch.isnan(canvas[rest].float()).all(), f"{what}: wrote outside its result region"


def test_canvas_gemm(device):
    from amk import dense

    L = _L()
    M, N, K, H = 300, 136, 72, 104
    a, w, b = ref.make_gemm("unit", M, N, K, 1)
    ad, wd, bd = _b16(a, device), _b16(w, device), b.to(device)
    c = _canvas(M + 1, N + 24, torch.bfloat16, device)
    _chk(L.amk_gemm_bf16(0, 0, _P(ad), K, _P(wd), K, _P(bd), _P(c), N + 24, _P(None), 0, M, N, K, _S()), "nt")
    _exact_region(c, dense.gemm_nt_bf16(ad, wd, bd), "nt")
    wn = wd.t().contiguous()
    c = _canvas(M + 1, N + 8, torch.bfloat16, device)
    _chk(L.amk_gemm_bf16(1, 0, _P(ad), K, _P(wn), N, _P(None), _P(c), N + 8, _P(None), 0, M, N, K, _S()), "nn")
    _exact_region(c, dense.gemm_nn_bf16(ad, wn), "nn")
    a, w12, b12 = ref.make_swiglu("unit", M, H, K, 2)
    ad, w12d, b12d = _b16(a, device), _b16(w12, device), b12.to(device)
    g_ref, ab_ref = dense.gemm_nt_swiglu_bf16(ad, w12d, b12d, keep_ab=True)
    for keep in (True, False):
        c = _canvas(M + 1, 2 * H + 16, torch.bfloat16, device) if keep else None
        g = _canvas(M + 1, H + 8, torch.bfloat16, device)
        _chk(L.amk_gemm_bf16(0, 1, _P(ad), K, _P(w12d), K, _P(b12d), _P(c), 2 * H + 16, _P(g), H + 8, M, 2 * H, K, _S()), "epi 1")
        _exact_region(g, g_ref, f"swiglu g keep={keep}")
        if keep:
            _exact_region(c, ab_ref, "swiglu (a | b)")
    dy, w3, ab = ref.make_swiglu_bwd("unit", M, H, K, 3)
    dyd, w3d, abd = _b16(dy, device), _b16(w3, device), _b16(ab, device)
    c = _canvas(M + 1, 2 * H + 16, torch.bfloat16, device)
    _chk(L.amk_gemm_bf16_swiglu_bwd(_P(dyd), K, _P(w3d), H, _P(abd), 2 * H, _P(c), 2 * H + 16, M, H, K, _S()), "epi 2")
    _exact_region(c, dense.gemm_nn_swiglu_bwd_bf16(dyd, w3d, abd), "swiglu bwd")


@pytest.mark.parametrize("M,N,K", [(1000, 136, 264), (40000, 128, 128)])
def test_canvas_tn(device, M, N, K):
    from amk import dense

    L = _L()
    y, x = ref.make_tn("unit", M, N, K, 4)
    yd, xd = _b16(y, device), _b16(x, device)
    c, db = _canvas(N + 1, K + 8, torch.float32, device), _canvas(1, N + 1, torch.float32, device)
    nb = L.amk_gemm_tn_bf16_ws_bytes(M, N, K)
    ws = torch.empty(max(nb, 16) // 4, device=device, dtype=torch.float32)
    _chk(L.amk_gemm_tn_bf16(_P(yd), N, _P(xd), K, _P(c), K + 8, _P(db), M, N, K, _P(ws), nb, _S()), "tn")
    dw_ref, db_ref = dense.gemm_tn_bf16(yd, xd, want_bias=True)
    _exact_region(c, dw_ref, "tn dw")
    _exact_region(db, db_ref.view(1, N), "tn db")


def test_canvas_ln_and_swiglu_mixed(device):
    """The mixed LayerNorm and SwiGLU through the C ABI into canvases with an extra row, bitwise the ops path (which
    takes the same kernels under autocast: ops.add_layer_norm(branch=True), ops.swiglu)."""
    from amk import ops

    M, D = 300, 260
    x, res, gamma, beta, cy, ch = ref.make_ln("unit", M, D, 5, x_bf16=True)
    got, canv = _ln_abi(device, x, res, gamma, beta, cy.bfloat16(), ch, True, extra=1)
    for n in ("h", "dh"):
        _exact_region(canv[n], got[n], "ln " + n)
    for n in ("y", "dh16"):
        _exact_region(canv[n], got[n], "ln " + n)
    _exact_region(canv["mean"].view(-1, 1), got["mean"].view(-1, 1), "ln mean")
    _exact_region(canv["rstd"].view(-1, 1), got["rstd"].view(-1, 1), "ln rstd")
    P = canv["part"].shape[0] - 1
    assert torch.isnan(canv["part"][P]).all() and not torch.isnan(canv["part"][:P]).any()
    xd, rd = _b16(x, device).requires_grad_(True), res.to(device).requires_grad_(True)
    wd, bd = gamma.to(device).requires_grad_(True), beta.to(device).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h, y = ops.add_layer_norm(xd, rd, wd, bd, 1e-5, branch=True)
    assert torch.equal(h, got["h"]) and torch.equal(y, got["y"])
    gx, gr, gw, gb = torch.autograd.grad((h, y), (xd, rd, wd, bd), (ch.to(device), cy.bfloat16().to(device)))
    assert torch.equal(gx, got["dh16"]) and torch.equal(gr, got["dh"])
    assert torch.equal(gw, got["dgamma"]) and torch.equal(gb, got["dbeta"])

    L = _L()
    H = 104
    ab, cot = ref.make_ab_cot("unit", M, H, 6)
    abd, cd = _b16(ab, device), _b16(cot, device)
    g, dab = _canvas(M + 1, H, torch.bfloat16, device), _canvas(M + 1, 2 * H, torch.bfloat16, device)
    _chk(L.amk_swiglu_bf16_fwd(_P(abd), M, H, _P(g), _S()), "swiglu fwd")
    _chk(L.amk_swiglu_bf16_bwd(_P(abd), _P(cd), M, H, _P(dab), _S()), "swiglu bwd")
    x = abd.clone().requires_grad_(True)
    g_ops = ops.swiglu(x)
    (dab_ops,) = torch.autograd.grad(g_ops, x, cd)
    _exact_region(g, g_ops, "mixed swiglu g")
    _exact_region(dab, dab_ops, "mixed swiglu dab")


# ---------------------------------------------------------------------------------------------- row invariance
def test_row_invariance(device):
    """Rows 37 .. 186 of a 300-row problem computed on their own (other tile positions, no neighbours): bitwise the same."""
    from amk import dense

    r0, r1 = 37, 187
    M, N, K, H = 300, 136, 72, 104
    a, w, b = ref.make_gemm("binade", M, N, K, 8)
    ad, wd, bd = _b16(a, device), _b16(w, device), b.to(device)
    assert torch.equal(dense.gemm_nt_bf16(ad, wd, bd)[r0:r1], dense.gemm_nt_bf16(ad[r0:r1], wd, bd)), "nt"
    wn = wd.t().contiguous()
    assert torch.equal(dense.gemm_nn_bf16(ad, wn)[r0:r1], dense.gemm_nn_bf16(ad[r0:r1], wn)), "nn"
    a, w12, b12 = ref.make_swiglu("outlier_rows", M, H, K, 9)
    ad, w12d, b12d = _b16(a, device), _b16(w12, device), b12.to(device)
    g, ab = dense.gemm_nt_swiglu_bf16(ad, w12d, b12d)
    g2, ab2 = dense.gemm_nt_swiglu_bf16(ad[r0:r1], w12d, b12d)
    assert torch.equal(g[r0:r1], g2) and torch.equal(ab[r0:r1], ab2), "swiglu fwd"
    dy, w3, abb = ref.make_swiglu_bwd("unit", M, H, K, 10)
    dyd, w3d, abd = _b16(dy, device), _b16(w3, device), _b16(abb, device)
    assert torch.equal(dense.gemm_nn_swiglu_bwd_bf16(dyd, w3d, abd)[r0:r1],
                       dense.gemm_nn_swiglu_bwd_bf16(dyd[r0:r1], w3d, abd[r0:r1])), "swiglu bwd"
    D = 260
    x, res, gamma, beta, cy, ch = ref.make_ln("offset", M, D, 11)
    full, _ = _ln_abi(device, x, res, gamma, beta, cy.bfloat16(), ch, True)
    part, _ = _ln_abi(device, x[r0:r1], res[r0:r1], gamma, beta, cy[r0:r1].bfloat16(), ch[r0:r1], True)
    for n in ("h", "y", "mean", "rstd", "dh", "dh16"):
        assert torch.equal(full[n][r0:r1], part[n]), "ln " + n


# ---------------------------------------------------------------------------------------------- composition
def test_swiglu_ffn_composition(device):
    """ops.swiglu_ffn under autocast is bitwise the calls _SwiGLUFFNMixed documents: gemm_nt_swiglu_bf16 + the library's
    F.linear forward; gemm_tn_bf16 (dW3, db3), gemm_nn_swiglu_bwd_bf16, gemm_tn_bf16 (dW12, db12), dab @ W12 backward."""
    from amk import dense, ops

    D, H = 256, 1368
    x, w12, b12 = ref.make_swiglu("outlier_rows", 2 * 150, H, D, 12)
    x = x.view(2, 150, D).to(device).requires_grad_(True)
    w12, b12 = w12.to(device).requires_grad_(True), (b12 * 0.1).to(device).requires_grad_(True)
    w3 = (torch.randn(D, H, generator=torch.Generator().manual_seed(13)) * H ** -0.5).to(device).requires_grad_(True)
    b3 = (torch.randn(D, generator=torch.Generator().manual_seed(14)) * 0.1).to(device).requires_grad_(True)
    cot = torch.randn(2, 150, D, generator=torch.Generator().manual_seed(15)).bfloat16().to(device)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = ops.swiglu_ffn(x, w12, b12, w3, b3)
    got = torch.autograd.grad(y, (x, w12, b12, w3, b3), cot)
    with torch.no_grad():
        x16, w12h, w3h = x.bfloat16().reshape(-1, D), w12.bfloat16(), w3.bfloat16()
        g, ab = dense.gemm_nt_swiglu_bf16(x16, w12h, b12)
        y_ref = F.linear(g, w3h, b3.bfloat16()).view(2, 150, D)
        dy2 = cot.reshape(-1, D)
        dw3, db3 = dense.gemm_tn_bf16(dy2, g, want_bias=True)
        dab = dense.gemm_nn_swiglu_bwd_bf16(dy2, w3h, ab)
        dw12, db12 = dense.gemm_tn_bf16(dab, x16, want_bias=True)
        dx = dab.mm(w12h).view(2, 150, D).float()
    assert torch.equal(y, y_ref)
    for n, u, v in zip(("dx", "dw12", "db12", "dw3", "db3"), got, (dx, dw12, db12, dw3, db3)):
        assert u.dtype == v.dtype and torch.equal(u, v), n


def test_linear_composition(device):
    """ops.linear under autocast: F.linear on the bf16 casts, dY W16 for the input gradient (the library, as autocast
    runs them), gemm_tn_bf16 for the weight and bias gradients -- bitwise."""
    from amk import dense, ops

    a, w, b = ref.make_gemm("binade", 300, 136, 72, 16)
    x = a.view(3, 100, 72).to(device).requires_grad_(True)
    wd, bd = w.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
    cot = torch.randn(3, 100, 136, generator=torch.Generator().manual_seed(17)).bfloat16().to(device)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = ops.linear(x, wd, bd)
    gx, gw, gb = torch.autograd.grad(y, (x, wd, bd), cot)
    with torch.no_grad():
        x16, w16 = x.bfloat16(), wd.bfloat16()
        assert torch.equal(y, F.linear(x16, w16, bd.bfloat16()))
        dy2 = cot.reshape(-1, 136)
        assert torch.equal(gx, dy2.mm(w16).view(3, 100, 72).float())
        dw, db = dense.gemm_tn_bf16(dy2, x16.reshape(-1, 72), want_bias=True)
    assert torch.equal(gw, dw) and torch.equal(gb, db)


@pytest.mark.parametrize("used", ["both", "h_only", "y_only"])
def test_add_layer_norm_composition(device, used):
    """ops.add_layer_norm(branch=True) under autocast against the C ABI calls, with y unused (dy None: dx = bf16(dh_in),
    dres = dh_in) and h unused (dh None: the kernel without dh_in)."""
    from amk import ops

    M, D = 200, 516
    x, res, gamma, beta, cy, ch = ref.make_ln("outlier_rows", M, D, 18, x_bf16=True)
    xd, rd = _b16(x, device).requires_grad_(True), res.to(device).requires_grad_(True)
    wd, bd = gamma.to(device).requires_grad_(True), beta.to(device).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h, y = ops.add_layer_norm(xd, rd, wd, bd, 1e-5, branch=True)
    dy = cy.bfloat16() if used != "h_only" else None
    dh_in = ch if used != "y_only" else None
    outs = [t for t, c in ((h, dh_in), (y, dy)) if c is not None]
    cots = [c.to(device) for c in (dh_in, dy) if c is not None]
    gx, gr, gw, gb = torch.autograd.grad(outs, (xd, rd, wd, bd), cots, allow_unused=True)
    abi, _ = _ln_abi(device, x, res, gamma, beta, dy, dh_in, True)
    assert torch.equal(h, abi["h"]) and torch.equal(y, abi["y"])
    if used == "h_only":
        assert torch.equal(gx, ch.to(device).bfloat16()) and torch.equal(gr, ch.to(device))
        assert gw is None and gb is None
    else:
        assert torch.equal(gx, abi["dh16"]) and torch.equal(gr, abi["dh"])
        assert torch.equal(gw, abi["dgamma"]) and torch.equal(gb, abi["dbeta"])
        R = ref.ref_ln(x, res, gamma, beta, cy, dh_in)
        ref.assert_within(abi, R, ("y", "dh", "dh16", "dgamma", "dbeta"), f"add_layer_norm {used}", key="ln_mixed")
