"""fp64 reference, per-element conditions and a CPU emulation for the fused training-mode BatchNorm2d + LeakyReLU on bf16
tensors under bf16 autocast, csrc/discr_norm.hip with T = __bf16 (amk_bnact_bf16_fwd / _bwd / _bwd_bwd,
ops.bn_leaky_relu_bf16).  Built on tests/discr_norm_ref.py: its inputs, its fp64 reference, its bound formulas and its
emulation, with the geometry of the bf16 walk.

Inputs and reference.  discr_norm_ref.make_inputs(family, shape, seed) with x, gz and ggx rounded to bf16 (gamma, beta,
gg_gamma, gg_beta and the running statistics stay f32); the reference is discr_norm_spec.fwd / bwd / bwd_bwd in fp64 on those
values.  Two families change their meaning on the bf16 grid:
    `offset`      the f32 family has x = 100 + 0.1 N(0, 1), |mu| r = 10^3.  bf16 is spaced 0.5 at 100, so rounding would leave a
                  channel one or two distinct values (99.5, 100, 100.5) and the family would test a near-constant channel, not a
                  mean far from its deviation.  Here x = RNE(100 + 2 N(0, 1)): a deviation of 4 bf16 spacings, about 25 distinct
                  values per channel, |mu| r = 50, the largest offset at which the channel still has a distribution.  It holds
                  what the f32 family holds (statistics by two passes, shift's cancellation of mu scale), at the scale bf16 can
                  express.  Its kink cap stays discr_norm_ref's 4e-3; with |mu| r = 50, E_y is 20 times smaller and the kink
                  set is met at a few 1e-4 at most.
    `mean_heavy`  gz and ggx = c + 0.01 N(0, 1) with |c| in [0.5, 1.5] keep two or three bf16 spacings of deviation: E, AC and
                  BD still cancel to about 1e-4 of their size, which is the family's point.
The flat constants (0, 1.5) and the dead channels' gamma = 0 are exact in bf16.  SEEDS names, per (family, shape), the seed
used where seed 0 does not meet the kink cap on the bf16 values (on the bf16 grid a whole cluster of equal x values can sit
inside E_y of the kink at once); tests/test_discr_norm_bf16_bounds.py asserts the caps on the CPU for every case of the GPU
file, from the fp64 reference alone.

Geometry.  The kernels are the f32 kernels on another element type: a 16-byte access holds 8 elements, so a plane is walked as
a scalar head of (8 - base % 8) % 8 elements, a body of 8-element runs and a scalar tail of up to 7; thread t adds the body
runs t, t + 256, ... (eight elements each, in order) and then at most one edge element per plane.  The segment stays 4096
ELEMENTS; for HW > 4096 a plane is cut into Q = ceil(HW / 4096) pieces of L = ceil(HW / Q) rounded up to a multiple of 8.  S,
Q and the workspace are those of the f32 geometry; only L and the heads and tails differ.  make_geo / plane_walk / _plan
restate that, and the depths T_chain, D1 = T_chain + 9, d_fold and d_chan of discr_norm_ref's docstring are taken from these
plans (a full segment of one plane is 2 body trips of 8 adds and one edge add, T_chain = 17, where the f32 walk has 4 trips
of 4 and one edge add).

Bounds.  Everything between a load and a store is the f32 arithmetic of the f32 kernels on f32 values that happen to be
bf16, so discr_norm_ref.reference's formulas with the depths above give b32, a bound on |f32 value before the store - exact|.
    mean, rstd, run_mean, run_var, dgamma, dbeta, g_gamma (f32 outputs):   |got - ref| <= b32.
    z, gx, g_gz, g_x (bf16 outputs): the kernel stores RNE(v), v the f32 value, |v - ref| <= b32, and nothing else is rounded.
    RNE is monotone, so          RNE(ref - b32) <= got <= RNE(ref + b32)                    (lo <= got <= hi),
    RNE's image of the interval, evaluated exactly in fp64 (gn_act_bf16_ref.bf16_rne).  For an element of the kink set K
    (discr_norm_ref: the f32 sign of y is not determined there) gx, g_gz and g_x are held to the interval of the nearer branch
    of s, each branch with its own b32, as discr_norm_ref does for TWO_BRANCH; z's b32 on K already covers both branches.
ratios() reports |got - ref| / b32 for the f32 outputs and, for the bf16 outputs, the share of b32 that the f32 value behind
the stored one must have used (gn_act_bf16_ref.interval_ratio; the smaller of the two branches on K); at most 1 where the
condition holds and above 1 where not.  The tests assert the interval condition itself.

The emulation is discr_norm_ref.emulate on the bf16 geometry (f32 torch ops in the kernels' order) with the four bf16
outputs rounded by tests/bf16_dense_ref.bf16_round; tests/test_discr_norm_bf16_bounds.py holds its f32 values under HALF of
every b32, its rounded outputs inside [lo, hi], and shows planted defects outside.

Measured, worst ratio per tensor over tests/test_discr_norm_bf16_gpu.py on the MI355X (interval_ratio for z, gx, g_gz and g_x,
|got - ref| / b32 for the others), and the emulation's worst over tests/test_discr_norm_bf16_bounds.py below it:
    MI355X      z 0.014    mean 0.008    rstd 0.008    run_mean 0.010    run_var 0.008    gx 0.012    dgamma 0.013
                dbeta 0.005    g_gz 0.008    g_x 0.011    g_gamma 0.030
    emulation   z 0.002    mean 0.008    rstd 0.008    run_mean 0.010    run_var 0.009    gx 0.008    dgamma 0.008
                dbeta 0.005    g_gz 0.004    g_x 0.011    g_gamma 0.031
(g_gamma's 0.030 is `mean_heavy`, where E - AC - BD cancels to 1e-4 of its terms, in the kernel and in the emulation alike; z's
0.014 is `offset`; as discr_norm_ref says, the emulation is an upper model of the kernels' roundings, not their arithmetic to
the bit, and the two rows of one tensor differ.  For a bf16 output the figure says that no stored element needed its f32 value
to be more than 1.4 % of b32 away from the reference.)
"""
import contextlib
import functools
from unittest import mock

import torch

import discr_norm_ref as ref
from bf16_dense_ref import bf16_round
from gn_act_bf16_ref import bf16_down, bf16_rne, bf16_up  # noqa: F401  (re-exported for the tests)

F32, F64 = torch.float32, torch.float64
BLOCK, SEG, VW = ref.BLOCK, ref.SEG, 8
EPS, MOMENTUM, SLOPE = ref.EPS, ref.MOMENTUM, ref.SLOPE
FAMILIES = ref.FAMILIES
TENSORS = ref.TENSORS
TWO_BRANCH = ref.TWO_BRANCH
ROUNDED = ("z", "gx", "g_gz", "g_x")          # bf16 outputs; the others are f32
BF16_INPUTS = ("x", "gz", "ggx")
NEW_SHAPES = [(3, 5, 3, 5),                   # HW = 15: plane bases on every residue mod 8
              (2, 3, 7, 1),                   # HW = 7: no body at all
              (1, 2, 67, 67)]                 # HW = 4489, above the segment and odd: two pieces of 2248 + 2241
CPU_SHAPES = ref.CPU_SHAPES + NEW_SHAPES
SHAPES = ref.CPU_SHAPES + ref.GPU_SHAPES + NEW_SHAPES
KINK_CAP, KINK_CAP_DEFAULT = ref.KINK_CAP, ref.KINK_CAP_DEFAULT
OFFSET_SCALE = 20.0                           # x - 100: 0.1 N(0, 1) -> 2 N(0, 1)
# (family, shape) -> seed, where seed 0 leaves more of the bf16 case inside E_y of the kink than the cap allows
SEEDS = {}
WORST = {}
WORST_BY_FAMILY = {}


# ---------------------------------------------------------------------------------------------- geometry of the bf16 walk
_f32_make_geo = ref.make_geo


def make_geo(N, C, HW):
    g = _f32_make_geo(N, C, HW)
    if g["Q"] > 1:
        g["L"] = (((HW + g["Q"] - 1) // g["Q"]) + VW - 1) & ~(VW - 1)
    return g


def plane_walk(g, c, s):
    """[(base, head, nv, tail)] per plane of segment s of channel c, as seg_walk<__bf16> splits it."""
    p0, p1, e0, e1 = ref.seg_of(g, s)
    ln = e1 - e0
    out = []
    for p in range(p0, p1):
        base = (p * g["C"] + c) * g["HW"] + e0
        head = min((VW - (base & (VW - 1))) & (VW - 1), ln)
        nv = (ln - head) >> 3
        out.append((base, head, nv, ln - head - VW * nv))
    return out


def ws_floats(N, C, HW):
    return C * make_geo(N, C, HW)["S"] * 3


@functools.lru_cache(maxsize=None)
def _plan(N, C, HW, defect=None):
    """discr_norm_ref._plan for the bf16 walk: idx (C, S, T, 256), the flat NCHW offset thread t adds at its step i of segment
    (c, s), or N C HW (a zero) for none.  defect plants a walk that is wrong: "tail_dropped", "head_short" (the head taken one
    element short: the element in front of the body is never read), "tail_twice" (the first tail element read twice)."""
    g = make_geo(N, C, HW)
    S, pad = g["S"], N * C * HW
    rows = []
    T = 0
    for c in range(C):
        for s in range(S):
            steps = []
            for base, head, nv, tail in plane_walk(g, c, s):
                it = (nv + BLOCK - 1) // BLOCK
                blk = torch.full((VW * it + 2, BLOCK), pad, dtype=torch.int64)
                i = torch.arange(nv)
                for k in range(VW):
                    blk[(i // BLOCK) * VW + k, i % BLOCK] = base + head + VW * i + k
                t = torch.arange(head - 1 if defect == "head_short" and head else head)
                blk[VW * it, t] = base + t
                if defect != "tail_dropped":
                    t = torch.arange(head, head + tail)
                    blk[VW * it, t] = base + VW * nv + t
                if defect == "tail_twice" and tail:
                    blk[VW * it + 1, head] = base + VW * nv + head
                steps.append(blk if defect == "tail_twice" else blk[:VW * it + 1])
            steps = torch.cat(steps)
            T = max(T, steps.shape[0])
            rows.append(steps)
    idx = torch.full((C * S, T, BLOCK), pad, dtype=torch.int64)
    for k, st in enumerate(rows):
        idx[k, :st.shape[0]] = st
    return idx.view(C, S, T, BLOCK)


@functools.lru_cache(maxsize=None)
def _segmap(N, C, HW):
    """(segid (N HW) of every element of a channel in (n, hw) order, cnt (S)) on the bf16 geometry."""
    g = make_geo(N, C, HW)
    segid = torch.empty(N, HW, dtype=torch.int64)
    for s in range(g["S"]):
        p0, p1, e0, e1 = ref.seg_of(g, s)
        segid[p0:p1, e0:e1] = s
    cnt = torch.tensor([ref.seg_count(g, s) for s in range(g["S"])], dtype=F64)
    return segid.reshape(-1), cnt


def depths(N, C, HW):
    """(D1, d_fold, d_chan) of discr_norm_ref's docstring for the bf16 walk."""
    S = make_geo(N, C, HW)["S"]
    trips = (S + BLOCK - 1) // BLOCK
    return _plan(N, C, HW).shape[2] + 9, trips + 9, min(trips + 8, S - 1)


@contextlib.contextmanager
def _bf16_walk(defect=None):
    """discr_norm_ref's reference and emulation read the geometry through these names."""
    def plan(N, C, HW, drop_tail=False):
        return _plan(N, C, HW, "tail_dropped" if drop_tail else defect)

    with mock.patch.multiple(ref, make_geo=make_geo, plane_walk=plane_walk, _plan=plan, _segmap=_segmap, depths=depths):
        yield


# ---------------------------------------------------------------------------------------------- inputs, reference, ratios
def make_inputs(family, shape, seed=None):
    """discr_norm_ref.make_inputs with x, gz and ggx rounded to bf16 (held as f32); `offset` re-scaled as the module docstring
    says.  seed None: SEEDS' choice for the case."""
    if seed is None:
        seed = SEEDS.get((family, tuple(shape)), 0)
    inp = ref.make_inputs(family, shape, seed)
    if family == "offset":
        inp["x"] = 100 + OFFSET_SCALE * (inp["x"] - 100)
    return dict(inp, **{k: bf16_round(inp[k]) for k in BF16_INPUTS})


def reference(inp, family=None):
    """discr_norm_ref.reference on the bf16 walk: {name: fp64 reference, "bound_" + name: b32, ...}, and for the bf16 outputs
    "lo_" + name and "hi_" + name (and "lo_alt_" / "hi_alt_" for gx, g_gz and g_x: the other branch of s on K), the bf16
    values (as fp64) the stored element must lie between."""
    with _bf16_walk():
        R = ref.reference(inp, family)
    for name in ROUNDED:
        for pre in ("", "alt_") if name in TWO_BRANCH else ("",):
            R["lo_" + pre + name] = bf16_rne(R[pre + name] - R["bound_" + pre + name])
            R["hi_" + pre + name] = bf16_rne(R[pre + name] + R["bound_" + pre + name])
    return R


def _inside1(v, R, key):
    return (R["lo_" + key] <= v) & (v <= R["hi_" + key]) & torch.isfinite(v)


def inside(v, R, name):
    """lo <= v <= hi per element (fp64 v); for gx, g_gz and g_x on either branch of s."""
    ok = _inside1(v, R, name)
    return ok | _inside1(v, R, "alt_" + name) if name in TWO_BRANCH else ok


def _interval_ratio1(v, R, key):
    """gn_act_bf16_ref.interval_ratio for one branch: the share of b32 that the f32 value behind the stored v must have used."""
    r, b = R[key], R["bound_" + key]
    c = bf16_rne(r)
    step = v.abs() * 2.0 ** -10 + 2.0 ** -140
    prev, nxt = bf16_down(v - step), bf16_up(v + step)
    s = torch.where(v > c, ((v + prev) / 2 - r) / b, torch.where(v < c, (r - (v + nxt) / 2) / b, torch.zeros_like(r)))
    ok = _inside1(v, R, key)
    s = torch.where(ok, s.clamp(0.0, 1.0), s.clamp(min=1.0) + 2.0 ** -20)
    return torch.where(torch.isfinite(v), s, torch.full_like(s, float("inf")))


def interval_ratio(v, R, name):
    q = _interval_ratio1(v, R, name)
    return torch.minimum(q, _interval_ratio1(v, R, "alt_" + name)) if name in TWO_BRANCH else q


def ratios(got, R, names=TENSORS, record=True, family=None):
    """{name: worst ratio}: interval_ratio for the bf16 outputs, |got - ref| / b32 (the nearer branch) for the f32 ones."""
    out = {}
    f32_names = [n for n in names if n not in ROUNDED]
    out.update(ref.ratios(got, R, names=f32_names, record=False))
    for name in names:
        if name in ROUNDED:
            v = got[name].detach().to(F64).cpu().reshape(R[name].shape)
            q = interval_ratio(v, R, name)
            out[name] = float(q.max()) if q.numel() else 0.0
        if record:
            WORST[name] = max(WORST.get(name, 0.0), out[name])
            if family is not None:
                WORST_BY_FAMILY[(family, name)] = max(WORST_BY_FAMILY.get((family, name), 0.0), out[name])
    return out


def outside(got, R, names=TENSORS):
    """[(tensor, ratio)] of the tensors with at least one element outside its condition."""
    q = ratios(got, R, names=names, record=False)
    bad = {n for n in names if n in ROUNDED and not bool(inside(got[n].detach().to(F64).cpu().reshape(R[n].shape), R, n).all())}
    return [(n, round(v, 2)) for n, v in q.items() if v > 1.0 or n in bad]


# ---------------------------------------------------------------------------------------------- CPU emulation
def emulate_f32(inp, mut=None, walk=None):
    """discr_norm_ref.emulate in the bf16 walk's order: every tensor in f32, the bf16 outputs before the store.  mut: a defect
    of discr_norm_ref.emulate; walk: a defect of _plan."""
    with _bf16_walk(walk):
        return ref.emulate(inp, mut=mut)


def emulate(inp, mut=None, walk=None):
    """What the kernels write: emulate_f32 with z, gx, g_gz and g_x rounded to bf16."""
    got = emulate_f32(inp, mut, walk)
    return dict(got, **{name: bf16_round(got[name]) for name in ROUNDED})
