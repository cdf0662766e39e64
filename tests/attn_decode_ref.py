"""fp64 reference, per-element error bound and an f32 emulation for the single-token decode attention
(csrc/attn_decode.hip, amk_attn_decode), in the manner of tests/attn_x6_ref.py and tests/bf16_attention_ref.py.

What the kernel computes, for one query row q (D) of a (batch, head) against J keys / values (rows 0 .. J - 1: the valid
cache rows and, in append mode, the new row last):
    q' = f32(q * qscale), qscale = f32(scale * log2 e)
    s_j = q' . k_j: a lane sums D / 8 products by FMA, three shuffle additions join the eight lanes of a key
    s_j = -1e9 log2 e where the key is masked
    per chunk c of KEYS keys: M_c = max s_j, p_j = exp2(s_j - M_c), l_c = sum p_j, o_c = sum p_j v_j  (a key group adds
        its <= KEYS / 32 keys by FMA, the 32 key groups are added in order)
    one chunk: o = o_c / l_c.  More: f_c = exp2(M_c - max M), o = (sum_c f_c o_c) / (sum_c f_c l_c), chunks in order.

The bound, with u = 2^-24, first order in u.
* score: a path through the dot product's additions has D / 8 FMAs and 3 additions; q' carries 1 rounding of its own
  and qscale 2 (the product scale * log2 e, and log2 e as an f32): D / 8 + 6 roundings relative to A_j = scale sum_d
  |q_d k_jd|.  The two exponent arguments, s_j - M_c and M_c - max M, have one sign and add up to s_j - max M, so their
  two roundings together are at most u |s_j - max M| <= 2 u max_j A_j.  In natural-log units all of it is below
      eps_j = (D + 2) u scale sum_d |q_d k_jd|,   E = max_j eps_j          (D / 8 + 8 <= D + 2 from D = 32 on)
  and a masked key's score is a constant: eps_j = 0.  p_j = e^(s_j) / Z moves by at most E in the numerator and E in
  the denominator: 2 E, relative.
* sums: the path of one term of o through its additions has at most KEYS / 32 FMAs in its key group, 31 additions of
  key groups and one FMA per chunk, and no more than J of them round (adding an empty key group's zero is exact): depth
  n <= min(J, KEYS / 32 + 31) + ceil(J / KEYS).  l has the same chain and enters as a relative error of o, so the two
  together are 2 n u sum_j p_j |v_jd|, and 2 n <= J + D + 4 for every J up to 1024 and D from 32 on.
* c = 16: those 4, and the remaining roundings on the path of one output element, read off the source: numerator --
  exp2 (v_exp_f32, 1 ulp = 2 u), the chunk factor's exp2 (2 u), its product (the FMA's, u), the division (2 u): 7;
  denominator -- exp2 (2 u), the chunk factor's exp2 (2 u), its product (u): 5.
      bound_d = (2 E + (J + D + c) u) sum_j p_j |v_jd| + J 2^-126 max |v|
  (the last term: v_exp_f32 flushes results under 2^-126 to zero).  No term is relative to a tensor's maximum.
The inputs the tests use keep E below 1e-4, where the second-order part of e^(2E) - 1 is under 1e-4 of the bound.
"""
import torch

U32 = 2.0 ** -24
FTZ = 2.0 ** -126
LOG2E32 = 1.4426950408889634
C_OPS = 16
KEYS = 64          # keys per chunk (csrc/attn_decode.hip keys_per_chunk)
KGROUPS = 32       # key groups of a workgroup
F64 = torch.float64
FILL = -1.0e9


def make_inputs(B, H, D, J, seed):
    """q (B, H, D), k and v (B, H, J, D), f32 on the CPU, unit normal: scores of order 1 at scale D^-1/2, so every key
    carries a weight of order 1 / J and a dropped, extra or misplaced row moves the output far beyond the bound."""
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(B, H, D, generator=g), torch.randn(B, H, J, D, generator=g), torch.randn(B, H, J, D, generator=g))


def reference(q, k, v, scale, mask=None):
    """(o in fp64 (B, H, D), per-element bound, p (B, H, J)) from f32 operands; mask: bool (B, J), True = keep."""
    qd, kd, vd = q.to(F64), k.to(F64), v.to(F64)
    J, D = k.shape[2], k.shape[3]
    s = torch.einsum("bhd,bhjd->bhj", qd, kd) * scale
    A = torch.einsum("bhd,bhjd->bhj", qd.abs(), kd.abs()) * scale
    eps = (D + 2) * U32 * A
    if mask is not None:
        keep = mask[:, None, :].expand_as(s)
        s = torch.where(keep, s, torch.full_like(s, FILL))
        eps = torch.where(keep, eps, torch.zeros_like(eps))
    p = torch.softmax(s, dim=-1)
    o = torch.einsum("bhj,bhjd->bhd", p, vd)
    E = eps.max(dim=-1).values[..., None]
    bound = (2 * E + (J + D + C_OPS) * U32) * torch.einsum("bhj,bhjd->bhd", p, vd.abs()) + J * FTZ * float(vd.abs().max())
    return o, bound, p


def worst_ratio(got, ref, bound):
    """(elements outside the bound, worst |got - ref| / bound)."""
    err = (got.to(F64) - ref).abs()
    return int((err > bound).sum()), float((err / bound).max())


def emulate(q, k, v, scale, mask=None, keys=KEYS):
    """The kernel's chain in f32 on the CPU, chunks and key groups added in the kernel's order.  Products and additions
    round separately here (the kernel's FMAs round once): no fewer roundings than the bound counts."""
    f32 = torch.float32
    B, H, J, D = k.shape
    qscale = (torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E32, dtype=f32))
    qp = q.to(f32) * qscale
    # lane g of a key's group owns dims 4 (g + 8 i) + e
    dims = torch.tensor([[4 * (g + 8 * i) + e for i in range(D // 32) for e in range(4)] for g in range(8)])
    lane = torch.zeros(B, H, J, 8, dtype=f32)
    for t in range(dims.shape[1]):
        lane = lane + qp[:, :, None, dims[:, t]] * k.to(f32)[:, :, :, dims[:, t]]
    for x in (1, 2, 4):   # the xor butterfly: lane 0's tree
        lane = lane + lane[..., [g ^ x for g in range(8)]]
    s = lane[..., 0]
    if mask is not None:
        s = torch.where(mask[:, None, :].expand_as(s), s, torch.full_like(s, FILL * LOG2E32))
    parts = []
    for j0 in range(0, J, keys):
        j1 = min(j0 + keys, J)
        M = s[:, :, j0:j1].max(dim=-1).values
        oc = torch.zeros(B, H, D, dtype=f32)
        lc = torch.zeros(B, H, dtype=f32)
        for kg in range(KGROUPS):
            og = torch.zeros(B, H, D, dtype=f32)
            lg = torch.zeros(B, H, dtype=f32)
            for j in range(j0 + kg, j1, KGROUPS):
                pj = torch.exp2(s[:, :, j] - M)
                lg = lg + pj
                og = og + pj[..., None] * v.to(f32)[:, :, j]
            oc, lc = oc + og, lc + lg
        parts.append((M, lc, oc))
    if len(parts) == 1:
        return parts[0][2] / parts[0][1][..., None]
    Mt = torch.stack([m for m, _, _ in parts]).max(dim=0).values
    acc = torch.zeros(B, H, D, dtype=f32)
    den = torch.zeros(B, H, dtype=f32)
    for M, lc, oc in parts:
        f = torch.exp2(M - Mt)
        acc = acc + f[..., None] * oc
        den = den + f * lc
    return acc / den[..., None]
