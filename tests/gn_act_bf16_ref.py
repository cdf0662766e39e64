"""fp64 reference, per-element conditions and a CPU emulation for the fused GroupNorm + Swish on bf16 tensors under bf16
autocast, csrc/gn_act.hip with T = __bf16 (amk_gnact_bf16_fwd / _bwd, ops.group_norm_act on a bf16 x).  Built on
tests/gn_act_ref.py: its inputs, its fp64 reference, its bound formulas and its emulation, with the geometry of the bf16 walk.

Inputs and reference.  gn_act_ref.make_inputs(family, case) with x and gz rounded to bf16 (gamma and beta stay f32); the
reference is gn_act_spec.fwd / bwd in fp64 on those values.

Geometry.  The kernels are the f32 kernels on another element type: a 16-byte access holds 8 elements, so a plane is walked as
a scalar head of up to 7 elements ((8 - base % 8) % 8), an 8-element body and a scalar tail of up to 7; thread t adds the body
runs t, t + 256, ... (eight elements each, in order) and then at most one edge element per plane.  The segment stays 4096
ELEMENTS; for HW > 4096 a plane is cut into Q = ceil(HW / 4096) pieces of L = ceil(HW / Q) rounded up to a multiple of 8.
make_geo / plane_steps / _plans below restate that; S, Q and the workspace are those of the f32 geometry, only L and the heads
and tails differ.  The depths D1, d_chan, Dp, Dn, Dg of gn_act_ref's docstring are taken from these plans (a full
segment is 2 body trips of 8 adds and one edge add, T_seg = 17, where the f32 walk has 4 trips of 4 and one edge add).

Bounds.  Everything between the load and the store is the f32 arithmetic of the f32 kernels on f32 values that happen to be
bf16, so gn_act_ref.reference's formulas with the depths above give b32, a bound on |f32 value before the store - exact|.
    mean, rstd (N, G), dgamma, dbeta (f32 outputs):   |got - ref| <= b32.
    z, gx (bf16 outputs): the kernel stores RNE(v), v the f32 value, |v - ref| <= b32, and nothing else is rounded.  RNE is
    monotone, so                 RNE(ref - b32) <= got <= RNE(ref + b32)                    (lo <= got <= hi),
    RNE's image of the interval, evaluated exactly in fp64 (bf16_rne below; bf16_down / bf16_up are the nearest bf16 values at
    or below / at or above, and lo, hi always lie between bf16_down(ref - b32) and bf16_up(ref + b32)).  The project's usual
    charge for a bf16 output is 2 U16 |ref| on top of the f32 bound; this is tighter, and is used because the rounding here is
    fully determined: one conversion, to nearest even, of a value the f32 bound already pins.  Where b32 is far below half a
    bf16 ulp (every family but `constant`) lo == hi for most elements and the condition is equality with RNE(ref).  The looser
    [bf16_down(ref - b32), bf16_up(ref + b32)] would admit an output truncated to bf16; tests/test_gn_act_bf16_bounds.py
    plants that defect and shows it outside.
ratios() reports |got - ref| / b32 for the four f32 outputs and, for z and gx, the share of b32 that the f32 value behind the
stored one must have used (interval_ratio: 0 where got == RNE(ref), else the distance from ref to the nearest value that RNE
sends to got, over b32); it is at most 1 where lo <= got <= hi and reported above 1 where not.  The tests assert the interval
condition itself.

Cases: gn_act_ref.CASES and (1, 64, 67, 67, 32): HW = 4489 is above the segment size and odd, so each plane is 2 pieces
(2248 + 2241), plane bases fall on every residue mod 8 and heads and tails of 1 to 7 elements all occur.  Families follow
gn_act_ref.family_cases() with the new case in the all-family list.

The emulation is gn_act_ref.emulate on the bf16 geometry (f32 torch ops in the kernels' order) with z and gx rounded by
tests/bf16_dense_ref.bf16_round; tests/test_gn_act_bf16_bounds.py holds its f32 values under HALF of every b32, its rounded
z and gx inside [lo, hi], and shows seven planted defects outside.

Measured, worst ratio per tensor (interval_ratio for z and gx, |got - ref| / b32 for the others) over tests/test_gn_act_bf16_gpu.py on the
MI355X, and the emulation's worst over tests/test_gn_act_bf16_bounds.py below it:
    MI355X      z 0.014    mean 0.006    rstd 0.011    gx 0.020    dgamma 0.016    dbeta 0.022
    emulation   z 0.025    mean 0.006    rstd 0.012    gx 0.026    dgamma 0.016    dbeta 0.023
(Far below the f32 kernels' 0.167: their worst is `constant`, where r = 1000 multiplies the error of the mean of 4096 equal f32
values; a bf16 constant has 8 significant bits, so its partial sums are exact and the mean comes out exact.  For z and gx the
figure says that no stored element needed its f32 value to be more than 3 % of b32 away from the reference.)
"""
import contextlib
import functools
from unittest import mock

import torch

import gn_act_ref as ref
from bf16_dense_ref import bf16_round

F32, F64 = torch.float32, torch.float64
BLOCK, SEG, VW = 256, 4096, 8
EPS = ref.EPS
FAMILIES = ref.FAMILIES
TENSORS = ref.TENSORS
ROUNDED = ("z", "gx")                      # bf16 outputs; the others are f32
NEW_CASE = (1, 64, 67, 67, 32)
CASES = ref.CASES + [NEW_CASE]
ALL_FAMILY_CASES = ref.ALL_FAMILY_CASES + [NEW_CASE]
WORST = {}
_f32_make_geo = ref.make_geo


def family_cases():
    """[(family, case)]: diffuse on every case, the other families on ALL_FAMILY_CASES."""
    return [("diffuse", c) for c in CASES] + [(f, c) for f in FAMILIES[1:] for c in ALL_FAMILY_CASES]


# ---------------------------------------------------------------------------------------------- geometry of the bf16 walk
def make_geo(C, HW, G):
    g = _f32_make_geo(C, HW, G)
    if g["Q"] > 1:
        g["L"] = (((HW + g["Q"] - 1) // g["Q"]) + VW - 1) & ~(VW - 1)
    return g


def ws_floats(N, C, HW, G):
    return N * C * make_geo(C, HW, G)["Q"] * 2


def plane_steps(base, ln, pad):
    """(steps, 256) flat offsets thread t adds, in order, for `ln` elements at `base`; `pad` where it adds nothing."""
    head = min((VW - (base & (VW - 1))) & (VW - 1), ln)
    nv = (ln - head) >> 3
    tail = ln - head - VW * nv
    it = (nv + BLOCK - 1) // BLOCK
    blk = torch.full((VW * it + 1, BLOCK), pad, dtype=torch.int64)
    i = torch.arange(nv)
    for k in range(VW):
        blk[(i // BLOCK) * VW + k, i % BLOCK] = base + head + VW * i + k
    t = torch.arange(head)
    blk[VW * it, t] = base + t
    t = torch.arange(head, head + tail)
    blk[VW * it, t] = base + VW * nv + t
    return blk


@functools.lru_cache(maxsize=4)
def _plans(N, C, HW, G):
    """gn_act_ref._plans for the bf16 walk."""
    g = make_geo(C, HW, G)
    pad = N * C * HW
    seg_rows, plane_rows = [], {}
    for run in range(N * G):
        for s in range(g["S"]):
            p0, p1, q, e0, e1 = ref.seg_of(g, s)
            steps = []
            for p in range(p0, p1):
                pl = run * g["cpg"] + p
                plane_rows[(pl, q)] = plane_steps(pl * HW + e0, e1 - e0, pad)
                steps.append(plane_rows[(pl, q)])
            seg_rows.append(torch.cat(steps))
    seg = ref._stack(seg_rows, pad)
    plane = ref._stack([plane_rows[(pl, q)] for pl in range(N * C) for q in range(g["Q"])], pad)
    return seg.view(N * G, g["S"], -1, BLOCK), plane.view(N * C, g["Q"], -1, BLOCK)


@functools.lru_cache(maxsize=None)
def _segmap(C, HW, G):
    g = make_geo(C, HW, G)
    segid = torch.empty(g["cpg"], HW, dtype=torch.int64)
    cnt = []
    for s in range(g["S"]):
        p0, p1, _, e0, e1 = ref.seg_of(g, s)
        segid[p0:p1, e0:e1] = s
        cnt.append((p1 - p0) * (e1 - e0))
    return segid.reshape(-1), torch.tensor(cnt, dtype=F64)


def depths(N, C, HW, G):
    """(D1, d_chan, Dp, Dn, Dg) of gn_act_ref's docstring for the bf16 walk."""
    g = make_geo(C, HW, G)
    seg, plane = _plans(N, C, HW, G)
    trips = lambda k: (k + BLOCK - 1) // BLOCK  # noqa: E731
    Dp = plane.shape[2] + 9
    return (seg.shape[2] + 9, min(trips(g["S"]) + 8, g["S"] - 1), Dp, Dp + trips(N * g["Q"]) + 9,
            Dp + trips(g["cpg"] * g["Q"]) + 10)


@contextlib.contextmanager
def _bf16_walk():
    """gn_act_ref's reference and emulation read the geometry through these four names."""
    with mock.patch.multiple(ref, make_geo=make_geo, _plans=_plans, _segmap=_segmap, depths=depths):
        yield


# ---------------------------------------------------------------------------------------------- bf16 in fp64
def _ulp(v):
    """The spacing of bf16 at each fp64 value (normal range; 2^-133 below 2^-126)."""
    _, ex = torch.frexp(v)
    return torch.exp2((ex - 1).clamp(min=-126).to(F64) - 7)


def _on_grid(v, fn):
    u = _ulp(v)
    return torch.where(torch.isfinite(v), fn(v / u) * u, v)


def bf16_rne(v):
    """fp64 -> the nearest bf16 value, ties to even, as fp64 (exact: v / ulp is a scaling by a power of two)."""
    return _on_grid(v, torch.round)


def bf16_down(v):
    return _on_grid(v, torch.floor)


def bf16_up(v):
    return _on_grid(v, torch.ceil)


# ---------------------------------------------------------------------------------------------- inputs, reference, ratios
def make_inputs(family, case, seed=0):
    """gn_act_ref.make_inputs with x and gz rounded to bf16 (held as f32)."""
    inp = ref.make_inputs(family, case, seed)
    return dict(inp, x=bf16_round(inp["x"]), gz=bf16_round(inp["gz"]))


def reference(inp, G, act):
    """gn_act_ref.reference on the bf16 walk: {name: fp64 reference, "bound_" + name: b32}, and for z and gx "lo_" + name and
    "hi_" + name, the bf16 values (as fp64) the stored element must lie between."""
    with _bf16_walk():
        R = ref.reference(inp, G, act)
    for name in ROUNDED:
        R["lo_" + name] = bf16_rne(R[name] - R["bound_" + name])
        R["hi_" + name] = bf16_rne(R[name] + R["bound_" + name])
    return R


def inside(v, R, name):
    """lo <= v <= hi per element (fp64 v)."""
    return (R["lo_" + name] <= v) & (v <= R["hi_" + name]) & torch.isfinite(v)


def interval_ratio(v, R, name):
    """Per element, the share of b32 the f32 value behind the stored v must have used: 0 where v == RNE(ref); where v lies
    above it, (m - ref) / b32 with m the midpoint between v and the bf16 value below v (what RNE sends to v starts there), and
    alike below.  At most 1 where inside() holds, and set above 1 where it does not."""
    r, b = R[name], R["bound_" + name]
    c = bf16_rne(r)
    step = v.abs() * 2.0 ** -10 + 2.0 ** -140
    prev, nxt = bf16_down(v - step), bf16_up(v + step)
    s = torch.where(v > c, ((v + prev) / 2 - r) / b, torch.where(v < c, (r - (v + nxt) / 2) / b, torch.zeros_like(r)))
    ok = inside(v, R, name)
    s = torch.where(ok, s.clamp(0.0, 1.0), s.clamp(min=1.0) + 2.0 ** -20)
    return torch.where(torch.isfinite(v), s, torch.full_like(s, float("inf")))


def ratios(got, R, names=TENSORS, record=True):
    """{name: worst ratio}: q of interval_ratio for z and gx, |got - ref| / b32 for the f32 outputs."""
    out = {}
    for name in names:
        v = got[name].detach().to(F64).cpu().reshape(R[name].shape)
        if name in ROUNDED:
            q = interval_ratio(v, R, name)
        else:
            q = (v - R[name]).abs() / R["bound_" + name]
            q = torch.where(torch.isfinite(v), q, torch.full_like(q, float("inf")))
        out[name] = float(q.max()) if q.numel() else 0.0
        if record:
            WORST[name] = max(WORST.get(name, 0.0), out[name])
    return out


# ---------------------------------------------------------------------------------------------- CPU emulation
def emulate_f32(inp, G, act):
    """gn_act_ref.emulate in the bf16 walk's order: every tensor in f32, z and gx before the store."""
    with _bf16_walk():
        return ref.emulate(inp, G, act)


def emulate(inp, G, act):
    """What the kernels write: emulate_f32 with z and gx rounded to bf16."""
    got = emulate_f32(inp, G, act)
    return dict(got, **{name: bf16_round(got[name]) for name in ROUNDED})
