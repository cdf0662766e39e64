"""Inputs, per-row references and a CPU model for the many-row decode attention (csrc/attn_prefill.hip, amk_attn_prefill
and amk_attn_prefill_bf16), built on tests/attn_decode_ref.py and tests/attn_decode_bf16_ref.py.

No new bound.  The kernel runs, for the query row at absolute position t = p0 + i, the chain of the single-token kernel
at J = t + 1 keys with 64 keys per chunk -- the same lane layout, the same FMAs and shuffle additions per score, one
maximum and one exp2 per key and chunk, the key groups and then the chunks added in order.  So row i is held to
attn_decode_ref.reference (f32) or to the RNE interval of attn_decode_bf16_ref.reference (bf16) of its own (q_t, k_0 ..
k_t, v_0 .. v_t), and attn_decode_ref.emulate / attn_decode_bf16_ref.emulate are its emulations.

Inputs are indexed by ABSOLUTE position: q, k, v (B, H, CAP, D), query t belongs to the row that lands at cache row t.
The reference of row t then does not depend on how a test splits the rows into (p0, n), and is computed once.

``model`` is what the launch does as a whole, on the CPU: the append and, per row, which keys it attends and where
they come from.  Its ``defect`` argument plants the faults of tests/test_attn_prefill_bounds.py.
"""
import torch

import attn_decode_bf16_ref as R16
import attn_decode_ref as R

F64 = torch.float64
DEFECTS = ("extra_key", "missing_key", "stale_new_row", "append_off_by_one")


def make_inputs(B, H, D, cap, seed, bf16=False):
    """q, k, v (B, H, cap, D) f32 on the CPU, unit normal (bf16: every value a bf16 value), by absolute position."""
    g = torch.Generator().manual_seed(int(seed))
    q, k, v = (torch.randn(B, H, cap, D, generator=g) for _ in range(3))
    return tuple(R16.bf16_round(t) for t in (q, k, v)) if bf16 else (q, k, v)


def row_reference(q, k, v, t, J=None, mask=None, bf16=False):
    """The reference of the query at position t over keys 0 .. J - 1 (default: the causal row, J = t + 1).
    f32: (ref, bound).  bf16: (ref, b32, lo, hi)."""
    J = t + 1 if J is None else J
    D = q.shape[-1]
    args = (q[:, :, t], k[:, :, :J], v[:, :, :J], D ** -0.5, None if mask is None else mask[:, :J])
    return R16.reference(*args)[:4] if bf16 else R.reference(*args)[:2]


def row_emulation(q, k, v, t, J=None, mask=None, bf16=False):
    J = t + 1 if J is None else J
    D = q.shape[-1]
    args = (q[:, :, t], k[:, :, :J], v[:, :, :J], D ** -0.5, None if mask is None else mask[:, :J])
    return (R16.emulate if bf16 else R.emulate)(*args)


def outside(got, ref, bf16=False):
    """Elements of got (B, H, D) outside the row's condition (non-finite ones included)."""
    g = got.to(F64)
    if bf16:
        return R16.count_outside(g, ref[2], ref[3])
    return int(((g - ref[0]).abs() > ref[1]).sum()) + int((~torch.isfinite(g)).sum())


def model(q, k_new, v_new, k_cache, v_cache, p0, attend, defect=None):
    """The launch in append mode.  q, k_new, v_new (B, H, n, D); k_cache, v_cache (B, H, cap, D), rows from p0 on hold
    whatever the caller left there.  attend(q_row (B, H, D), k (B, H, J, D), v) -> (B, H, D) is the row's arithmetic.
    Returns (o (B, H, n, D) or None where the call is out of range, k_cache', v_cache')."""
    assert defect is None or defect in DEFECTS
    n, cap = q.shape[2], k_cache.shape[2]
    kc, vc = k_cache.clone(), v_cache.clone()
    if p0 < 0 or p0 + n > cap:
        return None, kc, vc
    shift = 1 if defect == "append_off_by_one" else 0
    lo, hi = p0 + shift, min(p0 + shift + n, cap)
    kc[:, :, lo:hi], vc[:, :, lo:hi] = k_new[:, :, : hi - lo], v_new[:, :, : hi - lo]
    # keys as the rows see them: below p0 the cache, from p0 on the new rows -- never the cache, whatever it holds
    if defect == "stale_new_row":
        k_seen, v_seen = k_cache, v_cache
    else:
        k_seen = torch.cat((k_cache[:, :, :p0], k_new, k_cache[:, :, p0 + n:]), dim=2)
        v_seen = torch.cat((v_cache[:, :, :p0], v_new, v_cache[:, :, p0 + n:]), dim=2)
    rows = []
    for i in range(n):
        J = p0 + i + 1
        if defect == "extra_key":
            J = min(J + 1, cap)
        elif defect == "missing_key":
            J = max(J - 1, 1)
        rows.append(attend(q[:, :, i], k_seen[:, :, :J], v_seen[:, :, :J]))
    return torch.stack(rows, dim=2), kc, vc
