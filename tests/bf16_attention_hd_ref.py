"""fp64 reference and per-element error bounds for the bf16 attention kernels at head dims 32 and 128
(csrc/attn_bf16_hd.hip): make_inputs and reference of tests/bf16_attention_ref.py with the head dim D as an argument.

The bound is the one derived in that module's docstring; D enters it in three places -- the f32 additions of a score
((D + 4) in eps), of delta and dP ((D + 2) in ddelta and dperr) and of the dK / dQ sums ((I + J + D) in t).  Everything
that does not depend on D (masks, ratios, assert_within, needle_of, ...) is imported from there, not copied.

KEY_BLOCK: the backward's keys per workgroup, i.e. the block over which one dQ partial is summed; a CPU test checks it
against amk_attn_bf16_hd_bwd_ws_floats."""
import math

import torch

from bf16_attention_ref import (FAMILIES, FLOOR, MASKS, NAMES, NEEDLE_POS, U, U32, _gen, _masked,  # noqa: F401
                                assert_within, bf16_round, make_masks, needle_of, needle_positions, ratios)
from oracle import ref_cpu

HEAD_DIMS = (32, 128)
KEY_BLOCK = {32: 256, 128: 128}


def make_inputs(family, B, H, I, J, D, scale, seed):
    """q (B,H,I,D), k, v (B,H,J,D), d_o (B,H,I,D): float32 tensors of bf16 values; the families of
    bf16_attention_ref.make_inputs."""
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


def reference(q, k, v, d_o, scale, key_mask=None, causal_mask=None):
    """{"o", "dq", "dk", "dv"}: fp64 reference values, and {"bound_o", ...}: the per-element bounds.  q, k, v, d_o:
    (B, H, T, D) CPU tensors of bf16 values, D taken from q; masks as make_masks returns them."""
    q, k, v, d_o = (t.detach().to("cpu", torch.float64) for t in (q, k, v, d_o))
    B, H, I, D = q.shape
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
