"""fp64 reference and per-element error bounds for the bf16 attention kernels (csrc/attn_bf16.hip).

The reference is models/softmax_attention.py:62-76 (oracle.ref_cpu.attention_core) run in fp64 on the bf16 values the
kernels see, forward and torch.autograd backward: masked_fill(-1e9) on the scaled scores, key_mask True = keep,
causal_mask True = masked, a fully masked row gets uniform weights over all J keys.

Bounds.  u = 2^-8: bf16 keeps 8 significant bits, so one round-to-nearest is off by up to 2^-8 relative (2^-9 of the
next power of two, which is up to 2^-8 of the value).  u32 = 2^-24 for f32.  Per (b, h), with p the fp64 softmax
weights, s = q.k the raw scores, m_i = max over the unmasked keys of |s_ij|, and all products below taken over
absolute values:

* Softmax weights.  The kernels form s in f32 (bf16 x bf16 products are exact, D = 64 f32 additions), fold in the
  scale as c2 = scale log2 e and take exp2 of (s c2 - m c2) with rounded operands (the backward starts its MFMA chain
  from -(m + log2 l) / c2; the lazy reference of the unmasked forward sits up to 8 below the maximum in the exponent).
  The relative error of one unnormalised weight is then at most
      eps_ij = u32 ((D + 4) scale |q||k|_ij + 4 scale (|s_ij| + m_i) + 8),
  and the normaliser l = sum of J f32 weights (plus the rescales, one per 64-key tile) adds
      ebar_i = sum_j p_ij eps_ij + (J + 2 J / 64 + 8) u32.
  E = eps + ebar bounds the relative error of a normalised f32 weight.  A masked key has weight exactly 0 on both
  sides, and a fully masked row exactly 1 / J in f32 (the kernels' fill makes its exponent exactly 0): eps = 0 there.
* Forward: P unnormalised is rounded to bf16 for P.V (u p|v| at most), accumulated in f32 (J u32, inside ebar), and O
  is rounded to bf16 once (u |o|):
      o:  2u (|o| + p|v|) + (p E)|v| + floor.
  The factor 2 on the rounding terms is the margin: rounding errors do add up coherently (the CPU emulation of these
  rounding points reaches 0.44 of the dv bound, i.e. 0.88 of its u terms), and at 2u the emulation stays under half of
  every bound (tests/test_bf16_attention_bounds.py).
* Backward: P is recomputed in f32 (error E) and rounded to bf16 for dV; dS / scale = P (dP - delta) is formed in f32
  and rounded to bf16 once for both dK and dQ; delta = rowsum(dO o) is taken from the bf16 O of the forward, so it is
  off by
      ddelta_i = sum_d |dO_id| bound_o_id + (D + 2) u32 sum_d |dO_id o_id|,
  and dP = dO.v - delta (an f32 MFMA chain started from -delta) by dperr = (D + 2) u32 (|dO||v| + |delta|).  The
  error of one dS / scale entry is at most
      t_ij = p_ij (2u g_ij + ddelta_i + dperr_ij + E_ij g_ij + (I + J + D) u32 g_ij),   g = |dP - delta|,
  (the last term: the f32 sums of the dK / dQ products, dQ as per-256-key-block partials summed in order), and 0 at
  a masked position (its dS is exactly 0 on both sides).  dV, dK and dQ are rounded to bf16 once:
      dv: 2u (|dv| + p^T|dO|) + (p E)^T|dO| + floor
      dk: scale t^T|q| + 2u |dk| + floor
      dq: scale t |k| + 2u |dq| + floor
* floor = 1e-5 max |reference| of that tensor: it only covers weights that underflow f32 (a term the bound scales by
  p vanishes with p, while the kernel's exp2 flushes to exactly 0 below 2^-126).

Input families (make_inputs) and masks (make_masks) shared by the CPU check of the bound itself and the GPU tests.
Tensors are (B, H, T, 64); the values are bf16-exact.
"""
import math

import torch

from oracle import ref_cpu

U = 2.0 ** -8
U32 = 2.0 ** -24
D = 64
FLOOR = 1e-5
NAMES = ("o", "dq", "dk", "dv")
NEEDLE_POS = (0, 31, 32, 63, 64, 255, 256, -1)
FAMILIES = ("diffuse", "peaked", "needles", "large", "climb")
MASKS = ("none", "key", "triu", "causal", "both", "dead_rows", "dead_batch", "j1_masked")


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def needle_positions(J):
    """The needle key positions that exist at this J (0, 31, 32, 63, 64, 255, 256, J - 1), in order, without repeats."""
    out = []
    for n in NEEDLE_POS:
        n = J - 1 if n < 0 else n
        if n < J and n not in out:
            out.append(n)
    return out


def needle_of(B, H, I, J):
    """(B, H, I) long: the planted key of each query -- a different one for every batch element, head and query."""
    pos = torch.tensor(needle_positions(J))
    b = torch.arange(B).view(B, 1, 1)
    h = torch.arange(H).view(1, H, 1)
    i = torch.arange(I).view(1, 1, I)
    return pos[(i + 3 * h + 5 * b) % len(pos)]


def make_inputs(family, B, H, I, J, scale, seed):
    """q (B,H,I,64), k, v (B,H,J,64), d_o (B,H,I,64): float32 tensors of bf16 values.

    diffuse: N(0, 1).  peaked: q scaled so that the scaled scores have standard deviation 5 (a softmax support of a
    few keys).  needles: per (batch, head, query) one planted key (needle_of) whose scaled score leads every other by
    about 24.  large: raw scores around +-3600 (the sign alternates by head) that differ between keys by O(15).
    climb: scores that grow by a step per 64-key tile (the running maximum moves in every tile)."""
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
        w, _ = torch.linalg.qr(n(B, H, D, len(pos)))          # orthonormal key directions per (b, h)
        w = w.transpose(-1, -2)                                  # (B, H, npos, D)
        k = n(B, H, J, D) * 0.25
        for c, j in enumerate(pos):
            k[:, :, j] = 8.0 * w[:, :, c]
        slot = (torch.arange(I).view(1, 1, I) + 3 * torch.arange(H).view(1, H, 1) + 5 * torch.arange(B).view(B, 1, 1)) % len(pos)
        gamma = 24.0 / (7.0 * scale)
        q = gamma * torch.gather(w, 2, slot.unsqueeze(-1).expand(B, H, I, D)) + 0.1 * n(B, H, I, D)
    elif family == "large":
        u = torch.nn.functional.normalize(n(B, H, 1, D), dim=-1)
        sign = torch.where(torch.arange(H) % 2 == 0, 1.0, -1.0).view(1, H, 1, 1)
        q = 60.0 * sign * u + n(B, H, I, D)
        k = 60.0 * u + 0.25 * n(B, H, J, D)
    elif family == "climb":
        u = torch.nn.functional.normalize(n(D), dim=0)
        nt = max(1, J // 64)
        q = (n(B, H, I, D) + u * torch.linspace(0.0, 4.0, I).view(1, 1, I, 1)) * (D ** -0.5 / scale)
        k = n(B, H, J, D) * 0.3 + ((torch.arange(J) // 64).float() / nt).view(1, 1, J, 1) * u * 60.0
    else:
        raise ValueError(family)
    return tuple(bf16_round(t.float()) for t in (q, k, v, d_o))


def make_masks(kind, B, I, J, seed):
    """(key_mask (B, J) bool True = keep, causal_mask (I, J) bool True = masked), either None.

    key: random keys masked (key 0 kept); triu: causal triu(1); causal: an arbitrary random (I, J) mask, some rows fully
    masked; both: key + causal; dead_rows: triu(1) with rows 0, I / 2 and I - 1 fully masked; dead_batch: batch element
    0 has every key masked; j1_masked: every key masked (meant for J = 1)."""
    g = _gen(seed + 7)
    km = cm = None
    if kind in ("key", "both", "dead_batch"):
        km = torch.rand(B, J, generator=g) > 0.3
        km[:, 0] = True
        if kind == "dead_batch":
            km[0] = False
    if kind == "triu" or kind == "dead_rows":
        cm = torch.ones(I, J, dtype=torch.bool).triu(1)
        if kind == "dead_rows":
            cm[[0, I // 2, I - 1]] = True
    if kind in ("causal", "both"):
        cm = torch.rand(I, J, generator=g) < 0.4
        cm[::7] = True                                          # fully masked rows
        cm[1::5] = False                                        # rows that see every key
    if kind == "j1_masked":
        km = torch.zeros(B, J, dtype=torch.bool)
    if kind not in MASKS:
        raise ValueError(kind)
    return km, cm


def _masked(B, I, J, key_mask, causal_mask):
    """(B, 1, I, J) bool: True where the score is filled."""
    m = torch.zeros(B, 1, I, J, dtype=torch.bool)
    if key_mask is not None:
        m |= ~key_mask.bool()[:, None, None, :]
    if causal_mask is not None:
        m |= causal_mask.bool()[None, None]
    return m


def reference(q, k, v, d_o, scale, key_mask=None, causal_mask=None):
    """{"o", "dq", "dk", "dv"}: fp64 reference values, and {"bound_o", ...}: the per-element bounds of the module
    docstring.  q, k, v, d_o: (B, H, T, 64) CPU tensors of bf16 values; masks as make_masks returns them."""
    q, k, v, d_o = (t.detach().to("cpu", torch.float64) for t in (q, k, v, d_o))
    B, H, I, _ = q.shape
    J = k.shape[2]
    km = key_mask.cpu().bool() if key_mask is not None else None
    cm = causal_mask.cpu().bool() if causal_mask is not None else None
    out = {n: [] for n in NAMES}
    for b in range(B):   # (one batch element at a time: the (H, I, J) fp64 intermediates stay small)
        qb, kb, vb = (t[b:b + 1].clone().requires_grad_(True) for t in (q, k, v))
        o = ref_cpu.attention_core(qb, kb, vb, scale, None if km is None else km[b:b + 1], cm)
        dq, dk, dv = torch.autograd.grad((o * d_o[b:b + 1]).sum(), [qb, kb, vb])
        for n, t in zip(NAMES, (o, dq, dk, dv)):
            out[n].append(t.detach())
    R = {n: torch.cat(out[n]) for n in NAMES}
    floor = {n: FLOOR * float(R[n].abs().max()) for n in NAMES}
    bnd = {n: [] for n in NAMES}
    mask = _masked(B, I, J, km, cm)
    for b in range(B):
        qb, kb, vb, dob = q[b], k[b], v[b], d_o[b]
        ob, dqb, dkb, dvb = (R[n][b] for n in NAMES)
        aq, ak, av, ado = qb.abs(), kb.abs(), vb.abs(), dob.abs()
        filled = mask[b].expand(H, I, J)
        live = ~filled
        s = qb @ kb.transpose(-1, -2)
        p = torch.softmax((s * scale).masked_fill(filled, ref_cpu.FILL), dim=-1)
        smax = s.abs().masked_fill(filled, 0.0).amax(-1, keepdim=True)
        eps = U32 * ((D + 4) * scale * (aq @ ak.transpose(-1, -2)) + 4 * scale * (s.abs() + smax) + 8.0)
        eps = eps.masked_fill(filled, 0.0)
        ebar = (p * eps).sum(-1, keepdim=True) + (J + 2 * J / 64 + 8) * U32
        pE = p * (eps + ebar)
        b_o = 2 * U * (ob.abs() + p @ av) + pE @ av
        delta = (dob * ob).sum(-1, keepdim=True)
        dP = dob @ vb.transpose(-1, -2)
        gg = (dP - delta).abs()
        ddelta = (ado * (b_o + floor["o"])).sum(-1, keepdim=True) + (D + 2) * U32 * (ado * ob.abs()).sum(-1, keepdim=True)
        dperr = (D + 2) * U32 * (ado @ av.transpose(-1, -2) + delta.abs())
        t = p * (2 * U * gg + ddelta + dperr + (eps + ebar) * gg + (I + J + D) * U32 * gg)
        t = t * live
        bnd["o"].append(b_o)
        bnd["dv"].append(2 * U * (dvb.abs() + p.transpose(-1, -2) @ ado) + pE.transpose(-1, -2) @ ado)
        bnd["dk"].append(scale * (t.transpose(-1, -2) @ aq) + 2 * U * dkb.abs())
        bnd["dq"].append(scale * (t @ ak) + 2 * U * dqb.abs())
    for n in NAMES:
        R["bound_" + n] = torch.stack(bnd[n]) + floor[n]
    return R


def ratios(got, R, names=NAMES):
    """{name: (elements outside the bound, worst |got - ref| / bound)} for the tensors of `got` (any device / dtype)."""
    res = {}
    for n in names:
        a = got[n].detach().to("cpu", torch.float64)
        assert a.shape == R[n].shape, (n, tuple(a.shape), tuple(R[n].shape))
        err = (a - R[n]).abs()
        bad = ~(err <= R["bound_" + n])              # (a NaN is outside the bound too)
        r = torch.where(err == 0, torch.zeros_like(err), err / R["bound_" + n])   # (an all-zero reference: bound 0)
        res[n] = (int(bad.sum()), float(r.max()) if a.numel() else 0.0)
    return res


WORST = {}   # worst ratio per tensor name over every assert_within of the process (reported by the GPU tests)


def assert_within(got, R, what="", names=NAMES):
    """Every element of got[name] within the bound of R; records the worst ratios in WORST."""
    res = ratios(got, R, names)
    for n, (nbad, worst) in res.items():
        WORST[n] = max(WORST.get(n, 0.0), worst)
        assert nbad == 0, f"{what} {n}: {nbad} elements outside the bound (worst {worst:.3g}x the bound)"
    return res
