"""fp64 reference, per-element error bounds, input families and a CPU f32 emulation for the f32 attention core
(csrc/attn_fwd.hip, attn_fwd_x6.hip, attn_generic.h, attn_bwd_fused.hip, attn_bwd_fused_x6.hip), in the manner of
tests/bf16_attention_ref.py (whose masks it uses) and tests/attn_x6_ref.py (whose split and constants it uses).

The reference is oracle.ref_cpu.attention_core in fp64 and torch.autograd: masked_fill(-1e9) on the scaled scores,
key_mask True = keep, causal_mask True = masked, a fully masked ("dead") row is uniform over all J keys and passes no
gradient to q or k.  lse is the natural-log normaliser of the same filled scores; the kernels leave (m, l) with
lse = ln 2 (m + log2 l), where m is a lazy reference in the unmasked forwards, so m and l are not held separately.

The bound (hard tier of tests/dense_f32_ref.py: |got - ref| <= gamma_n sum|t_i| + n 2^-126, u = 2^-24,
gamma_n = n u / (1 - n u)).  An MFMA's internal sum counts as one rounded addition per product, in any order, plus one
for the product.  exp2 is v_exp_f32, 1 / l is v_rcp_f32 (or an f32 division), log2 is v_log_f32: neither
MI355X_MICROARCH.md nor cdna_hip_programming.md states their accuracy, so each is taken as 1 ulp = 2 u relative.
c = scale log2 e;  x = c q.k (log2 domain);  A = c |q|.|k|;  p the fp64 weights;  nt = ceil(J / 32) key tiles (32 keys
per LDS tile for head dims above 64, attn_generic.h:27; 64 otherwise, attn_common.h:11: the larger count is used).

* q' = q f32(f32(scale) f32(log2 e)): three roundings in the constant and one per element (attn_fwd.hip:53,60;
  attn_generic.h:137,151; attn_bwd_fused.hip:244,248; attn_fwd_x6.hip:41,47): gamma_4.
* S: a chain of D products (attn_fwd.hip:146-156; attn_generic.h:209-213, 369-375; backward attn_bwd_fused.hip:315-323,
  attn_generic.h:605-613, 774-782):  gamma_(D+5) A.  The unmasked non-keeping forwards open the chain with -m_ref
  (attn_fwd.hip:384-385, attn_generic.h:365), so m_ref passes through the same D additions:  gamma_(D+1) |m_ref|.
* the exp2 argument: x - m is one subtraction (attn_fwd.hip:213, 458; attn_generic.h:239, 425, 618, 637, 793, 806;
  attn_bwd_fused.hip:349, 371): u (|x| + |m|).  The lazy reference (attn_fwd.hip:435-454, attn_generic.h:401-419) moves
  at most once per tile; a move subtracts d from the tile's scores (one rounding) and stores m_ref + d rounded, so the
  tiles before and after a move sit u |m_ref| apart; the rescale's own argument m_old - m_new (attn_fwd.hip:222, 438) is
  rounded at u |d|, and the moves of a row add up to at most 2 M.  The fused backward's unfilled waves use
  m + log2 l as one constant (attn_bwd_fused.hip:256, 349): 2 u log2 l for v_log_f32, u |m + log2 l| for the sum, and
  l <= 2^8 J (a weight relative to the lazy reference is at most 2^8).  The reference is always a computed score of the
  row (the first tile's maximum, then a later tile's), so |m_ref| <= M = max over the live keys of |x|, and M collects
  D + 1 (chain) + 1 (subtraction) + nt (moves) + 2 (rescale arguments) roundings, taken as D + 6 + nt:
      e_ij = gamma_(D+6) A_ij + gamma_(D+6+nt) M_i + 3 u (8 + log2 J)              (log2 domain, absolute)
      eps_ij = (2^e_ij - 1)(1 + 2u) + 2u                                           (one unnormalised weight, relative)
  A dead row has exponent exactly 0 on both sides (fill - fill): e = 0.  A filled key of a live row has weight exactly
  0 on both sides (2^(-1.4e9) flushes; exp(-1e9) is 0 in fp64).
* the row sum: J additions in any order (attn_fwd.hip:218-220, 231, 462-469; attn_generic.h:241, 252, 427-429), three
  roundings per rescale (exp2 and the product, attn_fwd.hip:222-223, 438-439), the cross-half sum (attn_fwd.hip:264, 502):
      ebar_i = (1 + sum_j p_ij eps_ij)(1 + g_l) - 1,    g_l = gamma_(J + 3 (nt - 1) + 1)
  (the first tile has no rescale: attn_fwd.hip:437; in the masked kernels its factor is exp2(-inf) = 0 on zeros).
  lse:  |got - ref| <= -ln(1 - ebar_i), plus, in a dead row, gamma_3 1e9 (m is then the f32 constant
  f32(-1e9 f32(log2 e)), attn_common.h:19, two roundings, and the fp64 reading of it is off by that much).
* the reciprocal and the final product (attn_fwd.hip:265, 270; attn_generic.h:265, 272; backward
  attn_bwd_fused.hip:254, 371; attn_generic.h:538, 618): 3 u.  A normalised weight is off by at most
      E_ij = (1 + eps_ij)(1 + 3u) / (1 - ebar_i) - 1.
  That is the backward's P, whose scores are formed again (other operand roles, chains opened with zero) and divided
  by the forward's l.  In the forward the weights that are summed into l are the very ones that multiply v, so their
  errors d_j enter a normalised weight as d_j - sum_k p_k d_k, at most (1 - p_j) eps_j + sum_(k != j) p_k eps_k:
      F_ij = (1 + (eps_ij + S_i - 2 p_ij eps_ij) / (1 - S_i)) (1 + g_l)(1 + 3u) / (1 - g_l) - 1,   S_i = sum_k p_ik eps_ik
  (one key: F is the sum's and the reciprocal's rounding alone, whatever the score).
* P.V over J: J products (attn_fwd.hip:241-259, 477-493; attn_generic.h:255-261, 432-451) and the rescales:
      o:  sum_j p_ij ((1 + F_ij)(1 + c_pv) - 1) |v_jd|,    c_pv = gamma_(J + 1 + 3 (nt - 1)).
* delta = rowsum(dO o) from the kernel's own f32 o (attn_generic.h:487-493: D products, a shuffle tree):
      ddelta_i = sum_d |dO_id| bound_o_id + gamma_(D+1) sum_d |dO_id| (|o_id| + bound_o_id).
* dP - delta: a chain of D products opened with -delta (attn_bwd_fused.hip:307-309, 323, 327) or closed by one
  subtraction (attn_generic.h:612, 619, 638, 795, 808):
      dperr_ij = (1 + gamma_(D+3)) ddelta_i + gamma_(D+3) (|dO_i|.|v_j| + |delta_i|).
* dS / c = P (dP - delta), one product (attn_bwd_fused.hip:351, 373; attn_generic.h:619, 638, 795, 808); 0 on both
  sides at a filled position.  With g = |dP - delta| in fp64:
      t_ij = p_ij (((1 + E_ij)(1 + u) - 1) g_ij + (1 + E_ij)(1 + u) dperr_ij).
  With one key g = 0 in real arithmetic and the dq, dk bound is the residue dperr alone: no special case.
* dV over I (attn_bwd_fused.hip:400; attn_generic.h:818, 825):  dv: sum_i p_ij ((1 + E_ij)(1 + c_dv) - 1) |dO_id|,
  c_dv = gamma_(I+1).
* dK over I: q' (gamma_4), I products, f32(ln 2) and its product (attn_bwd_fused.hip:404, 458; attn_generic.h:821, 840):
      dk: scale ((1 + c_dk) t^T|q| + c_dk (p g)^T|q|),    c_dk = gamma_(I+7).
* dQ over J, in ANY order: 16x16x4 MFMAs over the workgroup's keys, two chains added, the scale (its f32 rounding and
  the product), then atomics, direct stores or per-key-block partials summed by attn_bwd_dq_reduce_kernel
  (attn_bwd_fused.hip:421-445, 467-473; attn_generic.h:646, 657).  Whatever the grouping, a term passes through at most
  J - 1 additions plus one per key block of 128:
      dq: scale ((1 + c_dq) t|k| + c_dq (p g)|k|),    c_dq = gamma_(J + ceil(J / 128) + 4).
* flush to zero, the only absolute floor: a weight below 2^-126 is 0 in the kernel and about 1e-38 in fp64; l >= 1 (the
  key that set the reference has weight 1), so that is at most 2^-126 per weight: 2 2^-126 (sum_j |v_jd| + J) on o, the
  same with dO and I on dv, with (g + 1) |q| on dk and (g + 1) |k| on dq.
No term is relative to a tensor's maximum.

model: which products run on split-bf16 MFMA, read from the kernels.  attn_fwd_x6.hip splits both of its products, S
(st_x6, :53-64) and P.V (pv_x6, :67-83); attn_bwd_fused_x6.hip splits dV and dK (x6_pair, :40-49) and leaves dP and dQ
on f32 MFMA (:4-7).  A split product of contraction length n replaces its gamma_(n+1) by the tests/attn_x6_ref.py form
    gamma_(6n) (1 + 2^-7)^2 + 2^-23 (1 + 2^-9)
(n counts the rows that exist: rows past the sequence are zero planes, and adding an exact zero rounds nothing).
"f32": none; "x6fwd": S and P.V (the backward reads or recomputes scores inside the same bound); "x6bwd": dV and dK;
"x6": all four.

Input families (make_inputs), all f32 and not bf16-exact; masks are bf16_attention_ref.make_masks' kinds.
emulate(): the f32 chain on the CPU with the most roundings the bound allows, and the mutations of
tests/test_attention_f32_bounds.py.
"""
import math

import torch

import attn_x6_ref as x6
from bf16_attention_ref import MASKS, _masked, make_masks   # noqa: F401  (make_masks, MASKS: used by the tests)
from oracle import ref_cpu

U = x6.U32
FTZ = x6.FTZ
F64 = torch.float64
F32 = torch.float32
LOG2E = math.log2(math.e)
LN2 = math.log(2.0)
NAMES = ("o", "lse", "dq", "dk", "dv")
FAMILIES = ("diffuse", "peaked", "needles", "large", "climb", "binade")
MODELS = {"f32": (), "x6fwd": ("s", "pv"), "x6bwd": ("dv", "dk"), "x6": ("s", "pv", "dv", "dk")}
NEEDLE_POS = (0, 31, 32, 63, 64, 127, 128, 255, 256, -1)
LAZY_TAU = 8.0
FILL_LOG2 = -1.0e9 * LOG2E


def gamma(n):
    return n * U / (1 - n * U)


def chain(n, split, extra=0):
    """Relative-to-sum|t| error of a chain of n products with `extra` further roundings per term."""
    if not split:
        return gamma(n + 1 + extra)
    c = gamma(6 * n) * (1 + 2.0 ** -7) ** 2 + 2.0 ** -23 * (1 + 2.0 ** -9)
    return (1 + c) * (1 + gamma(extra)) - 1 if extra else c


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def needle_positions(J):
    out = []
    for n in NEEDLE_POS:
        n = J - 1 if n < 0 else n
        if n < J and n not in out:
            out.append(n)
    return out


def make_inputs(family, B, H, I, J, D, scale, seed):
    """q, d_o (B, H, I, D) and k, v (B, H, J, D), f32 on the CPU.

    diffuse: N(0, 1).  peaked: scaled scores of standard deviation 5.  needles: per (batch, head, query) one planted key
    (positions NEEDLE_POS) whose scaled score leads every other by about 24.  large: raw scores around +-3600 (the sign
    alternates by head) that differ between keys by O(15).  climb: the scores of row i grow by about 4 g_i per 64-key
    tile in the log2 domain, g_i from 0 to 6 along the rows: the lazy reference (threshold 8) moves in every tile for the
    upper rows and never for the lower ones.  binade: q and k magnitudes spread over 2^-20 .. 2^20 along the head dim
    (tests/attn_x6_ref.py)."""
    g = _gen(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    v = n(B, H, J, D)
    d_o = n(B, H, I, D)
    if family == "diffuse":
        q, k = n(B, H, I, D), n(B, H, J, D)
    elif family == "peaked":
        q, k = n(B, H, I, D) * (5.0 / (scale * math.sqrt(D))), n(B, H, J, D)
    elif family == "needles":
        pos = needle_positions(J)
        w, _ = torch.linalg.qr(n(B, H, D, len(pos)))
        w = w.transpose(-1, -2)
        k = n(B, H, J, D) * 0.25
        for c, j in enumerate(pos):
            k[:, :, j] = 8.0 * w[:, :, c]
        slot = (torch.arange(I).view(1, 1, I) + 3 * torch.arange(H).view(1, H, 1) + 5 * torch.arange(B).view(B, 1, 1)) % len(pos)
        q = 24.0 / (7.0 * scale) * torch.gather(w, 2, slot.unsqueeze(-1).expand(B, H, I, D)) + 0.1 * n(B, H, I, D)
    elif family == "large":
        u = torch.nn.functional.normalize(n(B, H, 1, D), dim=-1)
        sign = torch.where(torch.arange(H) % 2 == 0, 1.0, -1.0).view(1, H, 1, 1)
        q = 60.0 * sign * u + n(B, H, I, D)
        k = 60.0 * u + 0.25 * n(B, H, J, D)
    elif family == "climb":
        u = torch.nn.functional.normalize(n(D), dim=0)
        step = 4.0 / (LOG2E * scale)
        q = n(B, H, I, D) * (D ** -0.5 / scale) + u * torch.linspace(0.0, 6.0, I).view(1, 1, I, 1)
        k = n(B, H, J, D) * 0.3 + (torch.arange(J) // 64).float().view(1, 1, J, 1) * u * step
    elif family == "binade":
        e = torch.randint(-20, 21, (D,), generator=g).float()
        q = n(B, H, I, D) * torch.exp2(e)
        k = n(B, H, J, D) * torch.exp2(-e + torch.randint(-3, 4, (D,), generator=g).float())
    else:
        raise ValueError(family)
    return tuple(t.float().contiguous() for t in (q, k, v, d_o))


def fp64_core(q, k, v, d_o, scale, key_mask=None, causal_mask=None):
    """{"o", "lse", "dq", "dk", "dv"} in fp64 from oracle.ref_cpu.attention_core and autograd, one batch element at a
    time; lse from the same filled scores."""
    q, k, v, d_o = (t.detach().to("cpu", F64) for t in (q, k, v, d_o))
    B, H, I, _ = q.shape
    J = k.shape[2]
    km = key_mask.cpu().bool() if key_mask is not None else None
    cm = causal_mask.cpu().bool() if causal_mask is not None else None
    mask = _masked(B, I, J, km, cm)
    out = {n: [] for n in NAMES}
    for b in range(B):
        qb, kb, vb = (t[b:b + 1].clone().requires_grad_(True) for t in (q, k, v))
        o = ref_cpu.attention_core(qb, kb, vb, scale, None if km is None else km[b:b + 1], cm)
        dq, dk, dv = torch.autograd.grad((o * d_o[b:b + 1]).sum(), [qb, kb, vb])
        s = torch.matmul(q[b:b + 1] * scale, k[b:b + 1].transpose(-1, -2)).masked_fill(mask[b:b + 1], ref_cpu.FILL)
        for n, t in zip(NAMES, (o, torch.logsumexp(s, dim=-1), dq, dk, dv)):
            out[n].append(t.detach())
    return {n: torch.cat(out[n]) for n in NAMES}


def reference(q, k, v, d_o, scale, key_mask=None, causal_mask=None, model="f32", core=None):
    """{"o", "lse", "dq", "dk", "dv"}: fp64 references ((B, H, I) for lse), and {"bound_o", ...}: one bound per element,
    as the module docstring derives them.  core: a fp64_core result for the same inputs (shared between models)."""
    split = MODELS[model]
    R = dict(core if core is not None else fp64_core(q, k, v, d_o, scale, key_mask, causal_mask))
    q, k, v, d_o = (t.detach().to("cpu", F64) for t in (q, k, v, d_o))
    B, H, I, D = q.shape
    J = k.shape[2]
    km = key_mask.cpu().bool() if key_mask is not None else None
    cm = causal_mask.cpu().bool() if causal_mask is not None else None
    mask = _masked(B, I, J, km, cm)
    c = scale * LOG2E
    nt = (J + 31) // 32
    c_s = chain(D, "s" in split, extra=5)
    c_pv = chain(J, "pv" in split, extra=3 * (nt - 1))
    c_dv = chain(I, "dv" in split)
    c_dk = chain(I, "dk" in split, extra=6)
    c_dq = gamma(J + (J + 127) // 128 + 4)
    g_m = gamma(D + 6 + nt)
    g_l = gamma(J + 3 * (nt - 1) + 1)
    g_dp = gamma(D + 3)
    bnd = {n: [] for n in NAMES}
    for b in range(B):
        qb, kb, vb, dob = q[b], k[b], v[b], d_o[b]
        ob = R["o"][b]
        aq, ak, av, ado = qb.abs(), kb.abs(), vb.abs(), dob.abs()
        filled = mask[b].expand(H, I, J)
        dead = filled.all(-1, keepdim=True)
        kT = kb.transpose(-1, -2)
        x = (qb @ kT) * c
        A = (aq @ ak.transpose(-1, -2)) * c
        p = torch.softmax(((qb @ kT) * scale).masked_fill(filled, ref_cpu.FILL), dim=-1)
        M = x.abs().masked_fill(filled, 0.0).amax(-1, keepdim=True)
        e = c_s * A + g_m * M + 3 * U * (8.0 + math.log2(J))
        e = e.masked_fill(dead.expand_as(e), 0.0)
        eps = torch.expm1(LN2 * e) * (1 + 2 * U) + 2 * U
        S1 = (p * eps).sum(-1, keepdim=True)
        ebar = (1 + S1) * (1 + g_l) - 1
        assert float(ebar.max()) < 0.5, "the bound's first-order forms need a small normaliser error"
        E = (1 + eps) * (1 + 3 * U) / (1 - ebar) - 1
        Ef = (1 + (eps + S1 - 2 * p * eps) / (1 - S1)) * (1 + g_l) * (1 + 3 * U) / (1 - g_l) - 1
        b_o = (p * ((1 + Ef) * (1 + c_pv) - 1)) @ av + 2 * FTZ * (av.sum(-2, keepdim=True) + J)
        b_lse = -torch.log1p(-ebar) + dead * (gamma(3) * 1.0e9) + 2 * FTZ * J
        delta = (dob * ob).sum(-1, keepdim=True)
        ddelta = (ado * b_o).sum(-1, keepdim=True) + gamma(D + 1) * (ado * (ob.abs() + b_o)).sum(-1, keepdim=True)
        gg = (dob @ vb.transpose(-1, -2) - delta).abs()
        dperr = (1 + g_dp) * ddelta + g_dp * (ado @ av.transpose(-1, -2) + delta.abs())
        w = (1 + E) * (1 + U)
        t = (p * ((w - 1) * gg + w * dperr)).masked_fill(filled, 0.0)
        pg = (p * gg).masked_fill(filled, 0.0)
        fl = (2 * FTZ * (gg + 1)).masked_fill(filled, 0.0)
        bnd["o"].append(b_o)
        bnd["lse"].append(b_lse.squeeze(-1))
        bnd["dv"].append((p * ((1 + E) * (1 + c_dv) - 1)).transpose(-1, -2) @ ado + 2 * FTZ * (ado.sum(-2, keepdim=True) + I))
        bnd["dk"].append(scale * (((1 + c_dk) * t + c_dk * pg + fl).transpose(-1, -2) @ aq) + 2 * FTZ * (I + 8))
        bnd["dq"].append(scale * (((1 + c_dq) * t + c_dq * pg + fl) @ ak) + 2 * FTZ * (J + 8))
    for n in NAMES:
        R["bound_" + n] = torch.stack(bnd[n])
    return R


def lse_of(stats):
    """(B, H, I, 2) f32 row statistics (reference in the log2 domain, sum relative to it) -> natural-log normaliser, fp64."""
    st = stats.detach().to("cpu", F64)
    return (st[..., 0] + torch.log2(st[..., 1])) * LN2


def ratios(got, R, names=NAMES):
    """{name: (elements outside the bound, worst |got - ref| / bound)}; a NaN is outside; no element is excluded."""
    res = {}
    for n in names:
        a = got[n].detach().to("cpu", F64)
        assert a.shape == R[n].shape, (n, tuple(a.shape), tuple(R[n].shape))
        err = (a - R[n]).abs()
        bad = ~(err <= R["bound_" + n])
        r = torch.where(err == 0, torch.zeros_like(err), err / R["bound_" + n])
        res[n] = (int(bad.sum()), float(r.max()) if a.numel() else 0.0)
    return res


WORST = {}   # (path, tensor) -> worst ratio over every assert_within of the process


def assert_within(got, R, path="", what="", names=NAMES):
    res = ratios(got, R, names)
    for n, (nbad, worst) in res.items():
        WORST[(path, n)] = max(WORST.get((path, n), 0.0), worst)
    for n, (nbad, worst) in res.items():
        assert nbad == 0, f"{path} {what} {n}: {nbad} elements outside the bound (worst {worst:.3g}x the bound)"
    return res


# ---------------------------------------------------------------------------------------------------------------- emulation
def _dot_seq(a, b, split=False, drop_tail=0, drop_lh=False):
    """sum_d a[..., m, d] b[..., n, d] -> (..., m, n) in f32, one rounded product and one rounded addition per d, in
    order.  split: both operands as three bf16 planes, per 16-deep block the six products in mfma6's order, each
    product exact and each addition rounded (tests/attn_x6_ref.py emulate).  drop_tail: the last d's left out;
    drop_lh: the (l, h) partial product left out."""
    n = a.shape[-1] - drop_tail
    acc = torch.zeros(*a.shape[:-1], b.shape[-2], dtype=F32)
    if not split:
        for d in range(n):
            acc = acc + a[..., :, None, d] * b[..., None, :, d]
        return acc
    ap, bp = x6.split3(a), x6.split3(b)
    order = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))   # (b plane, a plane): the K / A-operand part first
    for c0 in range(0, n, 16):
        for pb, pa in order:
            if drop_lh and (pb, pa) == (2, 0):
                continue
            for d in range(c0, min(c0 + 16, n)):
                acc = acc + ap[pa][..., :, None, d] * bp[pb][..., None, :, d]
    return acc


def _group_any(flag, group=32):
    """any() over groups of `group` consecutive rows (a wave's rows), broadcast back: (B, H, I, 1) bool."""
    B, H, I, _ = flag.shape
    pad = (-I) % group
    f = torch.nn.functional.pad(flag, (0, 0, 0, pad)).view(B, H, -1, group).any(-1, keepdim=True)
    return f.expand(B, H, f.shape[2], group).reshape(B, H, -1, 1)[:, :, :I]


def emulate(q, k, v, d_o, scale, key_mask=None, causal_mask=None, model="f32", mutation=None, keys_per_wg=128):
    """The kernels' chain in f32 on the CPU: 64-key tiles, every sum as sequential f32 additions of rounded products,
    the exp2 / log2 domain, the lazy reference (held in the chain's opening value) where there is no mask and the true
    running maximum where there is one, delta from the emulation's own o, dq as per-key-block partials summed in order.
    Returns {"o", "lse", "dq", "dk", "dv"}.  mutation plants one defect:
    drop_key64 (row 1 loses key 64), dead_live_only (a dead row is normalised over the keys the key mask keeps),
    causal_shift (the causal mask moved by one key), drop_d2 (S without the last two of D), skip_rescale (the last tile's
    rescale of o skipped), dq_drop_block (key block 1's dq partial omitted), delta_bf16_o (delta from o rounded to
    bf16), drop_lh (every split product without its (l, h) part)."""
    split = MODELS[model]
    q, k, v, d_o = (t.detach().to("cpu", F32) for t in (q, k, v, d_o))
    B, H, I, D = q.shape
    J = k.shape[2]
    km = key_mask.cpu().bool() if key_mask is not None else None
    cm = causal_mask.cpu().bool() if causal_mask is not None else None
    lazy = km is None and cm is None
    cm_f = cm
    if mutation == "causal_shift":
        cm_f = torch.cat([cm[:, :1], cm[:, :-1]], dim=1)
    filled = _masked(B, I, J, km, cm_f).expand(B, H, I, J)
    if mutation == "dead_live_only":
        gone = filled.all(-1, keepdim=True) & ~km[:, None, None, :]    # -inf there instead of the fill
    drop_lh = mutation == "drop_lh"
    qscale = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    qp = q * qscale
    fill = torch.tensor(-1.0e9, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    tail = 2 if mutation == "drop_d2" else 0
    s_all = _dot_seq(qp, k, "s" in split, tail, drop_lh)          # chains opened with zero: the backward's scores
    o = torch.zeros(B, H, I, D, dtype=F32)
    l = torch.zeros(B, H, I, 1, dtype=F32)
    m = torch.full((B, H, I, 1), -math.inf, dtype=F32) if not lazy else torch.zeros(B, H, I, 1, dtype=F32)
    ntile = (J + 63) // 64
    for t in range(ntile):
        j0, j1 = 64 * t, min(64 * t + 64, J)
        if lazy and "s" not in split:   # -m_ref opens the chain (the split-bf16 kernel subtracts afterwards)
            s = (-m).expand(B, H, I, j1 - j0)
            for d in range(D - tail):
                s = s + qp[..., :, None, d] * k[:, :, None, j0:j1, d]
        elif lazy:
            s = s_all[..., j0:j1] - m
        else:
            s = torch.where(filled[..., j0:j1], fill, s_all[..., j0:j1])
            if mutation == "dead_live_only":
                s = torch.where(gone[..., j0:j1], torch.tensor(-math.inf), s)
        mx = s.amax(-1, keepdim=True)
        if lazy:
            move = _group_any(mx > LAZY_TAU) if t else torch.ones_like(mx, dtype=torch.bool)
            d_ = torch.where(move, mx if t == 0 else mx.clamp_min(0.0), torch.zeros_like(mx))
            alpha = torch.exp2(-d_) if t else torch.ones_like(mx)   # (no rescale in the first tile: nothing to scale)
            m = m + d_
            s = s - d_
        else:
            m_new = torch.maximum(m, mx)
            alpha = torch.where(torch.isinf(m_new), torch.zeros_like(m), torch.exp2(m - m_new))
            s = s - m_new
            m = m_new
        pw = torch.exp2(s)
        if mutation == "drop_key64" and j0 <= 64 < j1:
            pw[:, :, 1, 64 - j0] = 0.0
        l = l * alpha
        if not (mutation == "skip_rescale" and t == ntile - 1):
            o = o * alpha
        if "pv" in split:
            o = o + _dot_seq(pw, v[:, :, j0:j1].transpose(-1, -2), True, 0, drop_lh)
        else:
            for j in range(j1 - j0):
                o = o + pw[..., j:j + 1] * v[:, :, None, j0 + j]
        for j in range(j1 - j0):
            l = l + pw[..., j:j + 1]
    linv = 1.0 / l
    o = o * linv
    out = {"o": o, "lse": ((m.double() + torch.log2(l.double())) * LN2).squeeze(-1)}

    # ---- backward: P from the scores and (m, l), dP opened with -delta
    od = o.to(torch.bfloat16).float() if mutation == "delta_bf16_o" else o
    delta = torch.zeros(B, H, I, 1, dtype=F32)
    for d in range(D):
        delta = delta + d_o[..., d:d + 1] * od[..., d:d + 1]
    if lazy:
        p = torch.exp2(s_all - (m + torch.log2(l)))
    else:
        s_f = torch.where(filled, fill, s_all)
        if mutation == "dead_live_only":
            s_f = torch.where(gone, torch.tensor(-math.inf), s_f)
        p = torch.exp2(s_f - m) * linv
    dp = (-delta).expand(B, H, I, J)
    for d in range(D):
        dp = dp + d_o[..., :, None, d] * v[:, :, None, :, d]
    ds = torch.where(filled, torch.zeros((), dtype=F32), p * dp)
    pT, dsT = p.transpose(-1, -2), ds.transpose(-1, -2)
    out["dv"] = _dot_seq(pT, d_o.transpose(-1, -2), "dv" in split, 0, drop_lh)
    out["dk"] = _dot_seq(dsT, qp.transpose(-1, -2), "dk" in split, 0, drop_lh) * torch.tensor(LN2, dtype=F32)
    dq = None
    sc = torch.tensor(scale, dtype=F32)
    for kb, j0 in enumerate(range(0, J, keys_per_wg)):
        if mutation == "dq_drop_block" and kb == 1:
            continue
        part = _dot_seq(ds[..., j0:j0 + keys_per_wg], k[:, :, j0:j0 + keys_per_wg].transpose(-1, -2)) * sc
        dq = part if dq is None else dq + part
    out["dq"] = dq
    return out
