"""tests/row_f32_ref.py without a GPU: the f32 CPU emulations of csrc/layernorm.hip, csrc/elementwise.hip and
csrc/optim.hip (the kernels' summation order, with and without fused multiply-adds) stay at or below HALF of every
per-element bound on every family and case the GPU tests run; the fp64 reference rounded to f32 sits within a stated
fraction of the bound; defects planted in the fp64 specification land outside the bounds, so the bounds are not vacuous;
and the C ABI's refusals, which need no device memory."""
import ctypes
import math

import pytest
import torch

import row_f32_ref as ref

F32, F64 = torch.float32, torch.float64
U32 = ref.U32
_KEEP = {}


def _cached(key, make):
    """The last few (inputs, reference) pairs, shared between the tests and never modified."""
    if key not in _KEEP:
        if len(_KEEP) >= 6:
            _KEEP.pop(next(iter(_KEEP)))
        _KEEP[key] = make()
    return _KEEP[key]


def _worst(got, R, names):
    q = ref.ratios(got, R, names)
    assert all(nbad == 0 for nbad, _ in q.values()), q
    return {n: w for n, (_, w) in q.items()}


def _rounded(R, names):
    return {n: R[n].to(F32) for n in names}


# ---------------------------------------------------------------------------------------------- LayerNorm
def _ln(fam, M, D, with_res, with_dh):
    def make():
        x, res, gamma, beta, cy, ch = ref.make_ln(fam, M, D, 1000 + M + D)
        inp = (x, res if with_res else None, gamma, beta, cy, ch if with_dh else None)
        return inp, ref.ref_ln(*inp)
    return _cached(("ln", fam, M, D, with_res, with_dh), make)


def _ln_names(with_res):
    return (("h",) if with_res else ()) + ref.LN_FWD + ref.LN_BWD


@pytest.mark.parametrize("fam,M,D,with_res,with_dh", ref.ln_cases(), ids=lambda v: str(v))
def test_ln_emulation_under_half(fam, M, D, with_res, with_dh):
    inp, R = _ln(fam, M, D, with_res, with_dh)
    names = _ln_names(with_res)
    for fma in (False, True):
        q = _worst(ref.emulate_ln(*inp, fma=fma), R, names)
        print("ln", fam, M, D, "fma" if fma else "mul+add", {k: round(v, 4) for k, v in q.items()})
        assert max(q.values()) <= 0.5, q
    # the reference rounded to f32: one rounding (u32 |x|) against the 2 u32 |x| or more that every output's bound holds
    q = _worst(_rounded(R, names), R, names)
    assert all(v <= 0.5 for k, v in q.items()), q
    for n in names:
        assert bool(torch.isfinite(R["bound_" + n]).all())


def _ln_spec(inp, mut=None):
    """The fp64 specification of the two kernels with one defect planted."""
    x, res, gamma, beta, dy, dh_in = (None if t is None else t.to(F64) for t in inp)
    M, D = x.shape
    h = x + res if res is not None else x
    st = h[:, :-4] if mut == "chunk_dropped" and D > 4 else h
    mean = st.mean(1, keepdim=True)
    var = ((st - mean) ** 2).mean(1, keepdim=True)
    if mut == "unbiased_variance":
        var = var * D / (D - 1)
    if mut == "one_pass_f32":
        h32 = h.to(F32)
        var = ((h32 * h32).mean(1, keepdim=True) - h32.mean(1, keepdim=True) ** 2).clamp_min(0).to(F64)
    rstd = 1.0 / torch.sqrt(var + (1e-6 if mut == "eps_1e-6" else ref.LN_EPS))
    xh = (h - mean) * rstd
    gy = dy * gamma
    c1, c2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    if mut == "c2_dropped":
        c2 = 0 * c2
    dh = rstd * (gy - c1 - xh * c2) + (dh_in if dh_in is not None else 0.0)
    last = M - 1 if mut == "last_row_missing" else M
    return {"h": h, "y": xh * gamma + beta, "mean": mean[:, 0], "rstd": rstd[:, 0], "dh": dh,
            "dgamma": (dy * xh)[:last].sum(0), "dbeta": dy.sum(0)}


LN_MUTS = ["unbiased_variance", "eps_1e-6", "one_pass_f32", "chunk_dropped", "last_row_missing", "c2_dropped"]


def _outside(spec, R, names):
    return [(n, w) for n, (nbad, w) in ref.ratios(spec, R, names).items() if nbad]


@pytest.mark.parametrize("mut", LN_MUTS)
def test_ln_planted_defects(mut):
    hit = []
    for fam, M, D, with_res, with_dh in ref.ln_cases():
        if M > 100 or (mut == "one_pass_f32" and fam != "offset"):
            continue
        inp, R = _ln(fam, M, D, True, with_dh)
        names = _ln_names(True)
        assert max(_worst(_ln_spec(inp), R, names).values()) < 1e-6
        hit += [(fam, M, D) + o for o in _outside(_ln_spec(inp, mut), R, names)]
    assert hit, f"{mut}: inside every bound on every case"
    print(mut, [(f, M, D, n, float("%.3g" % w)) for f, M, D, n, w in hit[:6]])


# ---------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("fam", ref.COL_FAMILIES)
@pytest.mark.parametrize("M,N", ref.COL_SHAPES, ids=lambda v: str(v))
def test_colsum_emulation_under_half(fam, M, N):
    x = ref.make_colsum(fam, M, N, 7 + M + N)
    R = ref.ref_colsum(x)
    q = _worst(ref.emulate_colsum(x), R, ("colsum",))
    print("colsum", fam, M, N, round(q["colsum"], 4))
    assert q["colsum"] <= 0.5
    assert _worst(_rounded(R, ("colsum",)), R, ("colsum",))["colsum"] <= 1 / ref.colsum_chain(M)
    assert _worst({"colsum": x.to(F64).sum(0)}, R, ("colsum",))["colsum"] < 1e-6


def test_colsum_planted_defect():
    """The last row dropped.  (Where the chain is long and the rows cancel -- 8195 rows of +-1e4 over 2048 partials -- the
    bound exceeds a single row, as it has to: the defect must show on the other cases.)"""
    hit = []
    for fam in ref.COL_FAMILIES:
        for M, N in ref.COL_SHAPES[1:]:
            x = ref.make_colsum(fam, M, N, 7 + M + N)
            hit += [(fam, M, N) + o for o in _outside({"colsum": x[:-1].to(F64).sum(0)}, ref.ref_colsum(x), ("colsum",))]
    assert {h[:3] for h in hit} >= {("unit", M, N) for M, N in ref.COL_SHAPES[1:]}, hit


# ---------------------------------------------------------------------------------------------- gates
def _gate(kind, fam, M, H):
    def make():
        ab, cot = ref.make_gate(fam, M, H, 31 + M + H)
        return (ab, cot), ref.REF_GATE[kind](ab, cot)
    return _cached((kind, fam, M, H), make)


GATE_CASES = [(f, M, H) for M, H in ref.GATE_SHAPES for f in ref.GATE_FAMILIES] + \
    [(f, 64, ref.GATE_STRIDE_SHAPE[1]) for f in ("unit", "saturate")]     # (element-wise: 64 of the 2052 rows do here)


@pytest.mark.parametrize("kind", ["swiglu", "geglu"])
@pytest.mark.parametrize("fam,M,H", GATE_CASES, ids=lambda v: str(v))
def test_gate_emulation_under_half(kind, fam, M, H):
    (ab, cot), R = _gate(kind, fam, M, H)
    got = ref.emulate_gate(kind, ab, cot)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    q = _worst(got, R, ref.GATE_OUT)
    print(kind, fam, M, H, {k: round(v, 4) for k, v in q.items()})
    assert max(q.values()) <= 0.5, q
    # the reference rounded once: u32 |x| against at least 2 u32 |x| of products in every bound
    assert max(_worst(_rounded(R, ref.GATE_OUT), R, ref.GATE_OUT).values()) <= 0.5
    for n in ref.GATE_OUT:
        assert bool(torch.isfinite(R["bound_" + n]).all())


def test_gate_families_reach_their_edges():
    ab, _ = ref.make_gate("saturate", 33, 96, 31 + 33 + 96)
    a = ab[:, :96]
    for lo, hi in ((-88.9, -88.72), (-88.72, -88.5), (88.5, 88.72), (88.72, 88.9), (-104.2, -104.0), (103.8, 104.0)):
        assert bool(((a > lo) & (a < hi)).any()), (lo, hi)
    assert float(a.min()) == -300.0 and float(a.max()) == 300.0
    z, _ = ref.make_gate("zero", 7, 20, 1)
    sign = torch.signbit(z[:, :20])
    assert bool((z[:, :20] == 0).all()) and bool(sign.any()) and not bool(sign.all())


def _gate_spec(kind, ab, cot, mut=None):
    AB, G = ab.to(F64), cot.to(F64)
    H = G.shape[1]
    A, B = (AB[:, H:], AB[:, :H]) if mut == "halves_swapped" else (AB[:, :H], AB[:, H:])
    if kind == "swiglu":
        s = torch.sigmoid(A)
        sp = s if mut == "silu_grad_without_a_term" else s * (1 + A * (1 - s))
        return {"out": A * s * B, "da": G * B * sp, "db": G * A * s}
    c = 0.7071 if mut == "sqrt_half_truncated" else 1 / math.sqrt(2.0)
    if mut == "tanh_gelu":
        k = math.sqrt(2 / math.pi)
        u = k * (A + 0.044715 * A ** 3)
        th = torch.tanh(u)
        gelu, gp = 0.5 * A * (1 + th), 0.5 * (1 + th) + 0.5 * A * (1 - th * th) * k * (1 + 3 * 0.044715 * A * A)
    else:
        one_erf = torch.special.erfc(-A * c)
        gelu, gp = 0.5 * A * one_erf, 0.5 * one_erf + A * torch.exp(-(A * c) ** 2) * c / math.sqrt(math.pi)
    return {"out": gelu * B, "da": G * B * gp, "db": G * gelu}


@pytest.mark.parametrize("kind,mut", [("geglu", "tanh_gelu"), ("swiglu", "silu_grad_without_a_term"),
                                      ("swiglu", "halves_swapped"), ("geglu", "halves_swapped"),
                                      ("geglu", "sqrt_half_truncated")])
def test_gate_planted_defects(kind, mut):
    hit = []
    for fam in ref.GATE_FAMILIES:
        for M, H in ref.GATE_SHAPES[1:]:
            (ab, cot), R = _gate(kind, fam, M, H)
            assert max(_worst(_gate_spec(kind, ab, cot), R, ref.GATE_OUT).values()) < 1e-6
            hit += [(fam, M, H) + o for o in _outside(_gate_spec(kind, ab, cot, mut), R, ref.GATE_OUT)]
    assert hit, f"{kind} {mut}: inside every bound on every case"
    print(kind, mut, [(f, M, H, n, float("%.3g" % w)) for f, M, H, n, w in hit[:6]])


# ---------------------------------------------------------------------------------------------- Adam
def _adam(case):
    def make():
        pr, hp = ref.adam_problem(*case)
        return (pr, hp), ref.ref_adam(pr, hp)
    return _cached(("adam",) + tuple(case), make)


@pytest.mark.parametrize("case", ref.adam_cases(), ids=lambda c: "-".join(map(str, c)))
def test_adam_emulation_under_half(case):
    (pr, hp), R = _adam(case)
    for fma in (False, True):
        q = _worst(ref.emulate_adam(pr, hp, fma=fma), R, ref.ADAM_OUT)
        print("adam", case, "fma" if fma else "mul+add", {k: round(v, 4) for k, v in q.items()})
        assert max(q.values()) <= 0.5, q
    # the reference rounded once: u32 |x| against the 2 u32 |x| every bound holds for the last rounding alone
    q = _worst(_rounded(R, ref.ADAM_OUT), R, ref.ADAM_OUT)
    assert max(q.values()) <= 0.5 and q["norm"] <= 1 / 11, q
    for n in ref.ADAM_OUT:
        assert bool(torch.isfinite(R["bound_" + n]).all())
    if case[4] == 1:
        assert float(R["norm"]) > hp["max_norm"] > 0
    if case[4] == 2:
        assert 0 < float(R["norm"]) < hp["max_norm"]


def _adam_spec(pr, hp, mut=None):
    P, G, M_, V = (pr[k].to(F64) for k in ("p", "g", "m", "v"))
    idx = pr["seg_param"].long().repeat_interleave(ref.SEG)
    act = pr["active"][idx]
    t = pr["t"].to(F64)[idx] - (1 if mut == "bias_correction_of_t-1" else 0)
    b1, b2, eps, lr, wd = hp["beta1"], hp["beta2"], hp["eps"], hp["lr"], hp["wd"]
    N = torch.sqrt((G * G).sum())
    c = 1.0
    if hp["max_norm"] > 0:
        c = min(1.0, float(hp["max_norm"] / (N + (0.0 if mut == "clip_without_1e-6" else ref.EPS_CLIP))))
    adamw = hp["adamw"] != (mut == "decay_exchanged")
    gg, pp = G * c, P
    if wd != 0 and adamw:
        pp = P - lr * wd * P
    elif wd != 0:
        gg = (G + wd * P) * c if mut == "clip_after_l2" else gg + wd * P
    mm = M_ + (1 - b1) * (gg - M_)
    vv = b2 * V + (1 - b2) * gg * gg
    bc2s = torch.sqrt(1 - b2 ** t)
    den = (torch.sqrt(vv) + eps) / bc2s if mut == "eps_before_bc2" else torch.sqrt(vv) / bc2s + eps
    pn = pp - lr / (1 - b1 ** t) * (mm / den)
    return {"norm": N.view(1), "p": torch.where(act, pn, P), "m": torch.where(act, mm, M_), "v": torch.where(act, vv, V)}


@pytest.mark.parametrize("mut", ["eps_before_bc2", "decay_exchanged", "clip_after_l2", "clip_without_1e-6",
                                 "bias_correction_of_t-1"])
def test_adam_planted_defects(mut):
    hit = []
    for case in ref.adam_cases():
        if case[1] > 300:
            continue
        (pr, hp), R = _adam(case)
        assert max(_worst(_adam_spec(pr, hp), R, ref.ADAM_OUT).values()) < 1e-6
        hit += [case + o for o in _outside(_adam_spec(pr, hp, mut), R, ref.ADAM_OUT)]
    assert hit, f"{mut}: inside every bound on every case"
    print(mut, [h[:5] + (h[5], float("%.3g" % h[6])) for h in hit[:6]])


# ---------------------------------------------------------------------------------------------- refusals of the C ABI
def test_abi_refusals():
    from amk import lib

    L = lib.load()
    null, p, off = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    err = lambda: L.amk_last_error().decode()  # noqa: E731

    def fwd(x=p, res=p, gamma=p, M=3, D=8, h=p, y=p, mean=p):
        return L.amk_add_layernorm_fwd(x, res, gamma, p, M, D, 1e-5, h, y, mean, p, null)

    def bwd(dy=p, dh_in=p, M=3, D=8, dh=p, part=p):
        return L.amk_add_layernorm_bwd(dy, p, dh_in, p, p, p, M, D, dh, part, null)

    def col(x=p, M=3, D=8, part=p):
        return L.amk_colsum(x, M, D, part, null)

    for call, name, first in ((fwd, "amk_add_layernorm_fwd", "x"), (bwd, "amk_add_layernorm_bwd", "dy"), (col, "amk_colsum", "x")):
        assert call(**{first: null}) == -1 and "null" in err() and name in err()
        for kw in (dict(M=0), dict(D=0), dict(M=-1)):
            assert call(**kw) == -1 and "non-positive" in err(), kw
        for D in (6, 4100, 8192):
            assert call(D=D) == -2 and "not supported" in err(), D
        assert call(**{first: off}) == -1 and "16-byte" in err()
    assert fwd(y=null) == -1 and fwd(mean=null) == -1 and fwd(gamma=null) == -1
    assert fwd(res=null) == -1 and "go together" in err()
    assert fwd(h=null) == -1 and "go together" in err()
    assert fwd(res=off) == -1 and fwd(h=off) == -1 and fwd(y=off) == -1 and fwd(gamma=off) == -1 and "16-byte" in err()
    assert bwd(dh=null) == -1 and bwd(part=null) == -1 and "null" in err()
    assert bwd(dh_in=off) == -1 and bwd(dh=off) == -1 and bwd(part=off) == -1 and "16-byte" in err()
    assert col(part=null) == -1 and col(part=off) == -1
    for M in (0, 1, 4, 5, 8192, 8193, 10 ** 6):
        assert L.amk_rowsum_num_partials(M) == (ref.ln_parts(M) if M > 0 else 0), M
    assert L.amk_rowsum_num_partials(-3) == 0

    for name in ("amk_swiglu", "amk_geglu"):
        f, b = getattr(L, name + "_fwd"), getattr(L, name + "_bwd")
        for rc in (f(null, 3, 8, p, null), f(p, 3, 8, null, null), b(null, p, 3, 8, p, null), b(p, null, 3, 8, p, null),
                   b(p, p, 3, 8, null, null)):
            assert rc == -1 and "null" in err()
        for M, H in ((0, 8), (3, 0), (-1, 8)):
            assert f(p, M, H, p, null) == -1 and "non-positive" in err()
            assert b(p, p, M, H, p, null) == -1 and "non-positive" in err()
        for rc in (f(p, 3, 6, p, null), f(off, 3, 8, p, null), f(p, 3, 8, off, null), b(p, p, 3, 10, p, null),
                   b(off, p, 3, 8, p, null), b(p, off, 3, 8, p, null), b(p, p, 3, 8, off, null)):
            assert rc == -2 and "16-byte" in err()

    assert L.amk_opt_num_partials() == ref.NPART
    assert L.amk_sumsq_partials(null, 256, p, null) == -1 and L.amk_sumsq_partials(p, 256, null, null) == -1
    for n in (0, -256, 255, 257, 1000):
        assert L.amk_sumsq_partials(p, n, p, null) == -1 and "multiple of 256" in err(), n
    assert L.amk_sumsq_partials(off, 256, p, null) == -1 and "16-byte" in err()

    def adam(param=p, grad=p, m=p, v=p, n=512, seg=p, tab=p, partials=p, n_partials=256, max_norm=1.0, p16=None):
        hyper = (max_norm, 1e-3, 0.9, 0.999, 1e-8, 0.0, 3, null)
        if p16 is None:
            return L.amk_adam_flat_step(param, grad, m, v, n, seg, tab, partials, n_partials, *hyper, null)
        return L.amk_adam_flat_step_shadow(param, grad, m, v, n, seg, tab, partials, n_partials, *hyper, p16, null)

    for kw in (dict(param=null), dict(grad=null), dict(m=null), dict(v=null), dict(seg=null), dict(tab=null)):
        assert adam(**kw) == -1 and "null" in err(), kw
    for n in (0, -256, 100, 300):
        assert adam(n=n) == -1 and "multiple of 256" in err(), n
    assert adam(partials=null) == -1 and "clipping needs" in err()
    assert adam(n_partials=0) == -1 and "clipping needs" in err()
    for kw in (dict(param=off), dict(grad=off), dict(m=off), dict(v=off), dict(tab=off)):
        assert adam(**kw) == -1 and "16-byte" in err(), kw
    assert adam(p16=off) == -1 and "8-byte" in err()
    with pytest.raises(RuntimeError, match="amk_colsum"):
        lib.check(col(D=6), "amk_colsum")
