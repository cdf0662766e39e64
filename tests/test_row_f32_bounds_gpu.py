"""The f32 row kernels -- csrc/layernorm.hip (add + LayerNorm forward / backward, colsum), csrc/elementwise.hip (SwiGLU,
GEGLU) and csrc/optim.hip (squared-norm partials + flat Adam / AdamW) -- held element by element to the bounds of
tests/row_f32_ref.py, through the raw C ABI, at the edges the source defines: every NCH class of the LayerNorm on both
sides of its width, the backward's rows-per-wave loop with the 2048-partial cap (M = 8195), the forward's grid-stride
(M = 65541), the gates' grid-stride (2 101 248 float4 items), a second inner iteration of the squared-norm kernel (1029
segments) and the update's grid-stride (8200 segments); on the families of row_f32_ref (large means, zero variance,
spikes, rows and segments over many binades, the zeros of silu' and gelu', the GELU tail, expf overflow, tiny and huge
gradients).  Plus what a tolerance cannot see: outputs on canvases poisoned with 3e38 and guarded on both sides, rows
independent of their neighbours (bitwise), two runs agreeing bitwise, the gradient left exactly zero, a parameter
without a gradient untouched, the bf16 shadow exactly p'.to(bfloat16); and the ops on misaligned views and on gate
widths that have no kernel.

AMK_ROW_F32_BOUND_REPORT=<file>: write the worst |got - ref| / bound per kernel output over this module to that JSON
file."""
import ctypes
import json
import os

import pytest
import torch

import row_f32_ref as ref
from util import assert_close

pytestmark = pytest.mark.gpu
POISON = 3e38
GUARD = 4                      # rows (or elements of a vector) of poison on either side of every result


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    worst = {k: v for k, v in ref.WORST.items() if k.startswith("row32.")}
    print("worst |got - ref| / bound:", {k: round(v, 4) for k, v in sorted(worst.items())})
    path = os.environ.get("AMK_ROW_F32_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(worst, f, indent=1, sort_keys=True)


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


def _within(got, R, names, what, key):
    res = ref.assert_within(got, R, names, what, key="row32." + key)
    print(what, {n: round(w, 4) for n, (_, w) in res.items()})


class Canvas:
    """(rows, cols) result region inside a buffer of 3e38 with GUARD rows before and after it."""

    def __init__(self, rows, cols, device, dtype=torch.float32):
        self.full = torch.full((rows + 2 * GUARD, cols), POISON, device=device, dtype=dtype)
        self.view = self.full[GUARD:GUARD + rows]
        self.poison = float(self.full[0, 0])          # (3e38 as this dtype holds it)

    def check(self, what):
        assert bool((self.full[:GUARD] == self.poison).all() and (self.full[-GUARD:] == self.poison).all()), \
            f"{what}: wrote outside its result region"
        assert bool(torch.isfinite(self.view.float()).all() and (self.view != self.poison).all()), \
            f"{what}: result region not fully written, or not finite"


# ---------------------------------------------------------------------------------------------- LayerNorm
def _ln_abi(device, inp):
    """amk_add_layernorm_fwd + _bwd into canvases -> ({h, y, mean, rstd, dh, dgamma, dbeta}, canvases, P)."""
    L = _L()
    x, res, gamma, beta, dy, dh_in = (None if t is None else t.to(device) for t in inp)
    M, D = x.shape
    c = {n: Canvas(M, D, device) for n in ("y", "dh") + (("h",) if res is not None else ())}
    c.update({n: Canvas(M, 1, device) for n in ("mean", "rstd")})
    v = {n: k.view for n, k in c.items()}
    _chk(L.amk_add_layernorm_fwd(_P(x), _P(res), _P(gamma), _P(beta), M, D, ref.LN_EPS, _P(v.get("h")), _P(v["y"]),
                                 _P(v["mean"]), _P(v["rstd"]), _S()), "amk_add_layernorm_fwd")
    P = L.amk_rowsum_num_partials(M)
    c["part"] = Canvas(P, 2 * D, device)
    h = v["h"] if res is not None else x
    _chk(L.amk_add_layernorm_bwd(_P(dy), _P(h), _P(dh_in), _P(gamma), _P(v["mean"]), _P(v["rstd"]), M, D, _P(v["dh"]),
                                 _P(c["part"].view), _S()), "amk_add_layernorm_bwd")
    dgb = c["part"].view.view(P, 2, D).sum(0)              # as ops._ln_param_grads sums the partial rows
    out = {n: (t[:, 0] if n in ("mean", "rstd") else t) for n, t in v.items()}
    out.update({"dgamma": dgb[0], "dbeta": dgb[1]})
    torch.cuda.synchronize()
    return out, c, P


def _ln_inputs(fam, M, D, with_res, with_dh):
    x, res, gamma, beta, cy, ch = ref.make_ln(fam, M, D, 1000 + M + D)
    return (x, res if with_res else None, gamma, beta, cy, ch if with_dh else None)


@pytest.mark.parametrize("fam,M,D,with_res,with_dh", ref.ln_cases(), ids=lambda v: str(v))
def test_ln_bounds(device, fam, M, D, with_res, with_dh):
    inp = _ln_inputs(fam, M, D, with_res, with_dh)
    got, canv, P = _ln_abi(device, inp)
    assert P == ref.ln_parts(M)
    for n, c in canv.items():
        c.check(f"ln {n}")                               # (part: exactly P rows written)
    names = (("h",) if with_res else ()) + ref.LN_FWD + ref.LN_BWD
    R = ref.ref_ln(*inp)
    _within(got, R, names, f"ln {fam} M{M} D{D} res{int(with_res)} dh_in{int(with_dh)}", "ln")
    if fam == "constant":                                # variance 0: y = beta and rstd = eps^-1/2 up to the bounds
        y, rstd = got["y"].double().cpu(), got["rstd"].double().cpu()
        assert bool(((y - inp[3].double()).abs() <= R["bound_y"]).all())
        assert bool(((rstd - ref.LN_EPS ** -0.5).abs() <= R["bound_rstd"]).all())
    again, _, _ = _ln_abi(device, inp)
    for n in names:
        assert torch.equal(got[n], again[n]), f"ln {n}: two runs differ"


@pytest.mark.parametrize("M,D,r0,r1", [(37, 260, 5, 23), (8195, 8, 4099, 4200), (9, 2052, 8, 9)])
def test_ln_row_independence(device, M, D, r0, r1):
    inp = _ln_inputs("binade", M, D, True, True)
    full, _, _ = _ln_abi(device, inp)
    sl = tuple(t[r0:r1].contiguous() if t.dim() == 2 else t for t in inp)
    part, _, _ = _ln_abi(device, sl)
    for n in ("h", "y", "mean", "rstd", "dh"):
        assert torch.equal(full[n][r0:r1], part[n]), f"ln {n}: rows {r0}:{r1} alone differ"


# ---------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("M,N", ref.COL_SHAPES, ids=lambda v: str(v))
def test_colsum_bounds(device, M, N):
    L = _L()
    for fam in ref.COL_FAMILIES:
        x = ref.make_colsum(fam, M, N, 7 + M + N)
        xd = x.to(device)
        P = L.amk_rowsum_num_partials(M)
        assert P == ref.ln_parts(M)
        outs = []
        for _ in range(2):
            part = Canvas(P, N, device)
            _chk(L.amk_colsum(_P(xd), M, N, _P(part.view), _S()), "amk_colsum")
            part.check("colsum")
            outs.append(part.view.sum(0))
        assert torch.equal(outs[0], outs[1])
        _within({"colsum": outs[0]}, ref.ref_colsum(x), ("colsum",), f"colsum {fam} {M}x{N}", "colsum")


@pytest.mark.parametrize("M,N", [(8195, 256), (70, 2736)])
def test_ops_colsum(device, M, N):
    from amk import ops

    x = ref.make_colsum("binade", M, N, 3)
    got = ops.colsum(x.to(device))
    if N <= 1024:
        _within({"colsum": got}, ref.ref_colsum(x), ("colsum",), f"ops.colsum {M}x{N}", "colsum")
    else:                                                 # torch's reduction
        assert_close(got, x.double().sum(0), 2e-5, "ops.colsum fallback")


# ---------------------------------------------------------------------------------------------- gates
def _gate_abi(device, kind, ab, cot):
    L = _L()
    M, H = cot.shape
    abd, cd = ab.to(device), cot.to(device)
    out, dab = Canvas(M, H, device), Canvas(M, 2 * H, device)
    _chk(getattr(L, f"amk_{kind}_fwd")(_P(abd), M, H, _P(out.view), _S()), kind + " fwd")
    _chk(getattr(L, f"amk_{kind}_bwd")(_P(abd), _P(cd), M, H, _P(dab.view), _S()), kind + " bwd")
    out.check(kind + " out")
    dab.check(kind + " dab")
    return {"out": out.view, "da": dab.view[:, :H], "db": dab.view[:, H:]}


def _gate_check(device, kind, fam, M, H):
    ab, cot = ref.make_gate(fam, M, H, 31 + M + H)
    got = _gate_abi(device, kind, ab, cot)
    again = _gate_abi(device, kind, ab, cot)
    for n in ref.GATE_OUT:
        assert torch.equal(got[n], again[n]), f"{kind} {n}: two runs differ"
    _within(got, ref.REF_GATE[kind](ab, cot), ref.GATE_OUT, f"{kind} {fam} {M}x{H}", kind)


@pytest.mark.parametrize("kind", ["swiglu", "geglu"])
@pytest.mark.parametrize("M,H", ref.GATE_SHAPES, ids=lambda v: str(v))
def test_gate_bounds(device, kind, M, H):
    for fam in ref.GATE_FAMILIES:
        _gate_check(device, kind, fam, M, H)


@pytest.mark.parametrize("kind", ["swiglu", "geglu"])
@pytest.mark.parametrize("fam", ["unit", "saturate"])
def test_gate_grid_stride(device, kind, fam):
    M, H = ref.GATE_STRIDE_SHAPE
    assert M * (H // 4) > 8192 * 256
    _gate_check(device, kind, fam, M, H)


def _ops_gate(device, kind, x):
    """ops.swiglu / ops.geglu on x (a device tensor, any layout) -> {out, da, db} and the (M, 2H) / (M, H) inputs."""
    from amk import ops

    H = x.shape[-1] // 2
    cot = 2.0 * torch.randn(x.shape[:-1] + (H,), generator=torch.Generator().manual_seed(5))
    xr = x.detach().requires_grad_(True)
    out = getattr(ops, kind)(xr)
    (dx,) = torch.autograd.grad(out, xr, cot.to(device))
    got = {"out": out.reshape(-1, H), "da": dx[..., :H].reshape(-1, H), "db": dx[..., H:].reshape(-1, H)}
    return got, x.detach().cpu().reshape(-1, 2 * H), cot.reshape(-1, H)


@pytest.mark.parametrize("kind", ["swiglu", "geglu"])
def test_ops_gate_layouts(device, kind):
    """A (B, T, 2H) input, a non-contiguous one and a contiguous view at a storage offset of one element."""
    B, T, H = 3, 11, 20
    ab, _ = ref.make_gate("unit", B * T, H, 77)
    x3 = ab.view(B, T, 2 * H).to(device)
    wide = torch.zeros(B, T, 2 * H + 8, device=device)
    wide[..., 3:3 + 2 * H] = x3
    flat = torch.zeros(1 + B * T * 2 * H, device=device)
    flat[1:] = x3.reshape(-1)
    off = flat[1:].view(B, T, 2 * H)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0 and not wide[..., 3:3 + 2 * H].is_contiguous()
    for what, x in (("3d", x3), ("strided", wide[..., 3:3 + 2 * H]), ("offset", off)):
        got, ab2, cot = _ops_gate(device, kind, x)
        _within(got, ref.REF_GATE[kind](ab2, cot), ref.GATE_OUT, f"ops.{kind} {what}", kind)


@pytest.mark.parametrize("kind", ["swiglu", "geglu"])
@pytest.mark.parametrize("H", [6, 10])
def test_ops_gate_widths_without_a_kernel(device, kind, H):
    ab, _ = ref.make_gate("unit", 14, H, 78)
    got, ab2, cot = _ops_gate(device, kind, ab.view(2, 7, 2 * H).to(device))
    R = ref.REF_GATE[kind](ab2, cot)
    for n in ref.GATE_OUT:                                # torch computes these: the existing tolerance
        assert_close(got[n], R[n], 2e-5, f"ops.{kind} H={H} {n}")


# ---------------------------------------------------------------------------------------------- ops on misaligned views
def _offset_view(t, device):
    flat = torch.zeros(1 + t.numel(), device=device)
    flat[1:] = t.reshape(-1).to(device)
    v = flat[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("with_res", [False, True])
def test_ops_layer_norm_on_misaligned_views(device, with_res):
    from amk import ops

    M, D = 37, 260
    inp = _ln_inputs("offset", M, D, with_res, True)
    x, res, gamma, beta, cy, ch = inp
    xd, gd, bd = (_offset_view(t, device).requires_grad_(True) for t in (x, gamma, beta))
    cyd, chd = _offset_view(cy, device), _offset_view(ch, device)
    if with_res:
        rd = _offset_view(res, device).requires_grad_(True)
        h, y = ops.add_layer_norm(xd, rd, gd, bd, ref.LN_EPS)
        gx, gr, gg, gb = torch.autograd.grad((h, y), (xd, rd, gd, bd), (chd, cyd))
        assert torch.equal(gx, gr)
        got = {"h": h, "y": y, "dh": gx, "dgamma": gg, "dbeta": gb}
    else:
        y = ops.layer_norm(xd, gd, bd, ref.LN_EPS)
        gx, gg, gb = torch.autograd.grad(y, (xd, gd, bd), cyd)
        got = {"y": y, "dh": gx, "dgamma": gg, "dbeta": gb}
        inp = (x, None, gamma, beta, cy, None)
    _within(got, ref.ref_ln(*inp), tuple(got), f"ops layer_norm misaligned res{int(with_res)}", "ln")


def test_ops_colsum_on_a_misaligned_view(device):
    from amk import ops

    x = ref.make_colsum("unit", 70, 260, 4)
    _within({"colsum": ops.colsum(_offset_view(x, device))}, ref.ref_colsum(x), ("colsum",), "ops.colsum misaligned", "colsum")


# ---------------------------------------------------------------------------------------------- Adam
def _guarded(t, device, dtype=None):
    """t on the device followed by one guard segment of poison -> (buffer, view)."""
    buf = torch.full((t.numel() + ref.SEG,), POISON, device=device, dtype=dtype or t.dtype)
    buf[: t.numel()] = t.to(device)
    return buf, buf[: t.numel()]


def _adam_abi(device, pr, hp, shadow):
    """amk_sumsq_partials per bucket into one partials array, then amk_adam_flat_step(_shadow) per bucket."""
    L = _L()
    tab = ref.adam_table(pr, hp)
    if not hp["table"]:
        tab[:, 3] = 123.0                                 # the launch-argument form must not read the table's factor
    tabd = tab.to(device)
    nb = len(pr["nsegs"])
    pbuf, partials = _guarded(torch.zeros(nb * ref.NPART), device)
    norm = torch.full((1,), POISON, device=device)
    bufs, o = [], 0
    for ns in pr["nsegs"]:
        sl = slice(o * ref.SEG, (o + ns) * ref.SEG)
        b = {k: _guarded(pr[k][sl], device) for k in ("p", "g", "m", "v")}
        if shadow:
            b["p16"] = _guarded(pr["p"][sl].to(torch.bfloat16), device)
        b["seg"] = pr["seg_param"][o:o + ns].to(device)
        bufs.append(b)
        o += ns
    for k, b in enumerate(bufs):
        _chk(L.amk_sumsq_partials(_P(b["g"][1]), b["g"][1].numel(), _P(partials[k * ref.NPART:]), _S()), "amk_sumsq_partials")
    dec = (2 if hp["table"] else 0) | (1 if hp["adamw"] else 0)
    for k, b in enumerate(bufs):
        args = (_P(b["p"][1]), _P(b["g"][1]), _P(b["m"][1]), _P(b["v"][1]), b["p"][1].numel(), _P(b["seg"]), _P(tabd),
                _P(partials), partials.numel(), hp["max_norm"], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], dec,
                _P(norm) if k == 0 else _P(None))
        rc = L.amk_adam_flat_step_shadow(*args, _P(b["p16"][1]), _S()) if shadow else L.amk_adam_flat_step(*args, _S())
        _chk(rc, "amk_adam_flat_step")
    torch.cuda.synchronize()
    for b in bufs:
        for k, (buf, view) in ((k, v) for k, v in b.items() if k != "seg"):
            guard = buf[view.numel():]
            assert bool((guard == guard[0]).all()) and float(guard[0]) > 1e38, f"adam: wrote past the end of {k}"
    assert bool((pbuf[nb * ref.NPART:] == POISON).all())
    cat = lambda k: torch.cat([b[k][1] for b in bufs])  # noqa: E731
    out = {"norm": norm, "p": cat("p"), "m": cat("m"), "v": cat("v"), "g": cat("g")}
    if shadow:
        out["p16"] = cat("p16")
    return out


@pytest.mark.parametrize("i,case", list(enumerate(ref.adam_cases())), ids=lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c))
def test_adam_bounds(device, i, case):
    pr, hp = ref.adam_problem(*case)
    shadow = bool(i % 2)
    got = _adam_abi(device, pr, hp, shadow)
    _within(got, ref.ref_adam(pr, hp), ref.ADAM_OUT, f"adam {case} shadow{int(shadow)}", "adam")
    assert float(got["g"].abs().max()) == 0.0, "the gradient is left zeroed, a parameter without one included"
    idle = ~pr["active"][pr["seg_param"].long().repeat_interleave(ref.SEG)]
    assert bool(idle.any())                               # (the second bucket always holds one)
    for k in ("p", "m", "v"):
        assert torch.equal(got[k].cpu()[idle], pr[k][idle]), f"{k} of the parameter without a gradient changed"
    if shadow:
        assert torch.equal(got["p16"], got["p"].to(torch.bfloat16))
    again = _adam_abi(device, pr, hp, shadow)
    for k in got:
        assert torch.equal(got[k], again[k]), f"adam {k}: two runs differ"


def test_flat_adam_large_bucket(device):
    """FlatAdam over one bucket of 8200 segments (the update kernel's grid-stride, two inner iterations of the norm):
    one step against the fp64 reference under the bounds of the raw kernels."""
    from amk.dp import GradReducer
    from amk.optim import FlatAdam

    nseg = 8200
    n = nseg * ref.SEG
    gen = torch.Generator().manual_seed(9)
    p0, w = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    big = torch.nn.Parameter(p0.to(device))
    red = GradReducer([big])
    assert len(red.buckets) == 1 and red.buckets[0].flat.numel() == n
    # (hyper-parameters that f32 holds exactly: FlatAdam fills its table from the Python floats, the kernel sees floats)
    lr, b1, b2, eps, wd = 2.0 ** -10, 0.875, 1 - 2.0 ** -10, 2.0 ** -27, 0.0625
    opt = FlatAdam(red, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, decoupled=True)
    red.begin(True)
    (big * w.to(device)).sum().backward()
    red.finish(detach_unused=False)
    g = red.buckets[0].flat.clone().cpu()
    assert torch.equal(g, w)
    max_norm = float(w.double().norm()) / 3
    norm = opt.step(max_norm=max_norm)
    pr = dict(p=p0, g=g, m=torch.zeros(n), v=torch.zeros(n), nsegs=[nseg], seg_param=torch.zeros(nseg, dtype=torch.int32),
              active=torch.tensor([True]), t=torch.tensor([1]))
    hp = ref.adam_hyper(adamw=True, wd=wd, table=FlatAdam.TABLE_WD, max_norm=max_norm, lr=lr, beta1=b1, beta2=b2, eps=eps)
    st = opt.state_of(big)
    got = {"norm": norm, "p": big.detach().view(-1), "m": st["exp_avg"].view(-1), "v": st["exp_avg_sq"].view(-1)}
    _within(got, ref.ref_adam(pr, hp), ref.ADAM_OUT, "FlatAdam 8200 segments", "adam")
    assert float(red.buckets[0].flat.abs().max()) == 0.0
