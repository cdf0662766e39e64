"""fp64 reference, per-element condition and a CPU emulation for the single-token decode attention on a bf16 cache
(csrc/attn_decode.hip, amk_attn_decode_bf16), built on tests/attn_decode_ref.py.

Inputs.  attn_decode_ref.make_inputs rounded to bf16 (held as f32): the kernel's operands are bf16 values taken exactly.

Bound.  Between the loads and the final store the kernel is the f32 kernel's arithmetic on f32 values that happen to be
bf16: q' = f32(q) * qscale in f32, scores, maxima, exp2, l and o in f32, p never rounded, the same chunks, the same 32 key
groups added in order, the same combine.  Only the lane layout differs -- lane g of a key's group owns dims
[8 (g + 8 i), +8) for i < ceil(D / 64), lanes 4-7 nothing of a last step that holds 32 dims -- so a lane's dot product has
at most 8 ceil(D / 64) FMAs and 3 shuffle additions where the f32 kernel has D / 8 + 3: no more than D / 8 + 8 for every
D from 32 on, which is what attn_decode_ref's score term (D + 2) u already covers.  So the f32 value v before the store
obeys attn_decode_ref.reference's bound unchanged:  |v - ref| <= b32.

Condition on the stored output.  The kernel stores RNE(v) and rounds nothing else; RNE is monotone, so
    RNE(ref - b32) <= got <= RNE(ref + b32)                                  (lo <= got <= hi),
evaluated exactly in fp64 with gn_act_bf16_ref.bf16_rne.  This is not a 2 u |ref| allowance: b32 is far below half a
bf16 ulp for almost every element, where lo == hi and the condition is equality with RNE(ref).  An output truncated to
bf16, or a p rounded to bf16 on the way, lands outside (tests/test_attn_decode_bf16_bounds.py plants both).

emulate() is the kernel's chain in f32 on the CPU with the bf16 lane layout, chunks and key groups in the kernel's order,
and the output rounded to bf16 once; its switches plant the arithmetic faults of the CPU test.
"""
import torch

import attn_decode_ref as R
from bf16_dense_ref import bf16_round
from gn_act_bf16_ref import bf16_rne

F32, F64 = torch.float32, torch.float64
KEYS, KGROUPS = R.KEYS, R.KGROUPS


def make_inputs(B, H, D, J, seed):
    """attn_decode_ref.make_inputs with every operand a bf16 value (f32 tensors on the CPU)."""
    return tuple(bf16_round(t) for t in R.make_inputs(B, H, D, J, seed))


def reference(q, k, v, scale, mask=None):
    """(o fp64, b32, lo, hi, p): attn_decode_ref.reference on the bf16 values, and the bf16 values (as fp64) the stored
    element must lie between."""
    o, b32, p = R.reference(q, k, v, scale, mask)
    return o, b32, bf16_rne(o - b32), bf16_rne(o + b32), p


def inside(got, lo, hi):
    g = got.to(F64)
    return (lo <= g) & (g <= hi) & torch.isfinite(g)


def count_outside(got, lo, hi):
    return int((~inside(got, lo, hi)).sum())


def bf16_truncate(x):
    """f32 -> bf16 by dropping the low 16 bits (round toward zero), as f32: the planted store fault."""
    return (x.to(F32).contiguous().view(torch.int32) & -65536).view(F32)


def lane_dims(D):
    """(8, T) dims lane g of a key's group owns, in the order it adds them; D (a zero column) where it owns nothing."""
    steps = (D + 63) // 64
    rows = []
    for g in range(8):
        row = []
        for i in range(steps):
            base = 8 * (g + 8 * i)
            row += [base + e if base < D else D for e in range(8)]
        rows.append(row)
    return torch.tensor(rows)


def emulate_f32(q, k, v, scale, mask=None, keys=KEYS, round_p=False, drop_tail=False):
    """The f32 value before the store.  round_p: p rounded to bf16 before it is used (a fault).  drop_tail: the last
    32 dims of a D % 64 == 32 row left out of the dot product and of the output's sums (a fault)."""
    B, H, J, D = k.shape
    qscale = torch.tensor(scale, dtype=F32) * torch.tensor(R.LOG2E32, dtype=F32)
    zero = torch.zeros(B, H, 1, dtype=F32)
    qp = torch.cat((q.to(F32) * qscale, zero), dim=-1)
    kz = torch.cat((k.to(F32), torch.zeros(B, H, J, 1, dtype=F32)), dim=-1)
    vv = v.to(F32).clone()
    dims = lane_dims(D)
    if drop_tail:
        assert D % 64 == 32
        dims = torch.where(dims >= D - 32, torch.full_like(dims, D), dims)
        vv[..., D - 32:] = 0.0
    lane = torch.zeros(B, H, J, 8, dtype=F32)
    for t in range(dims.shape[1]):
        lane = lane + qp[:, :, None, dims[:, t]] * kz[:, :, :, dims[:, t]]
    for x in (1, 2, 4):
        lane = lane + lane[..., [g ^ x for g in range(8)]]
    s = lane[..., 0]
    if mask is not None:
        s = torch.where(mask[:, None, :].expand_as(s), s, torch.full_like(s, R.FILL * R.LOG2E32))
    parts = []
    for j0 in range(0, J, keys):
        j1 = min(j0 + keys, J)
        M = s[:, :, j0:j1].max(dim=-1).values
        oc = torch.zeros(B, H, D, dtype=F32)
        lc = torch.zeros(B, H, dtype=F32)
        for kg in range(KGROUPS):
            og = torch.zeros(B, H, D, dtype=F32)
            lg = torch.zeros(B, H, dtype=F32)
            for j in range(j0 + kg, j1, KGROUPS):
                pj = torch.exp2(s[:, :, j] - M)
                if round_p:
                    pj = bf16_round(pj)
                lg = lg + pj
                og = og + pj[..., None] * vv[:, :, j]
            oc, lc = oc + og, lc + lg
        parts.append((M, lc, oc))
    if len(parts) == 1:
        return parts[0][2] / parts[0][1][..., None]
    Mt = torch.stack([m for m, _, _ in parts]).max(dim=0).values
    acc = torch.zeros(B, H, D, dtype=F32)
    den = torch.zeros(B, H, dtype=F32)
    for M, lc, oc in parts:
        f = torch.exp2(M - Mt)
        acc = acc + f[..., None] * oc
        den = den + f * lc
    return acc / den[..., None]


def emulate(q, k, v, scale, mask=None, truncate=False, **faults):
    """What the kernel stores: emulate_f32 rounded to bf16 once (truncate: cut instead, a fault)."""
    o = emulate_f32(q, k, v, scale, mask, **faults)
    return bf16_truncate(o) if truncate else bf16_round(o)
