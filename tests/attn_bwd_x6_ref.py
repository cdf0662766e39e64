"""fp64 reference, per-element scales, input families and f32 emulations for the dV and dK products of the kept-scores
attention backward on split-bf16 MFMA (csrc/attn_bwd_fused_x6.hip, AMK_ATTN_BWD_X6), in the manner of
tests/attn_x6_ref.py, whose split it reuses.

What the kernel computes per (batch, head), key j and head dim d, summing over the queries i in tiles of 32:
    dV[j, d] = sum_i P[i, j] dO[i, d]                 dK[j, d] = ln 2 * sum_i dS[i, j] q'[i, d],   q' = q * scale * log2 e
with P and dS the f32 values the f32 kernel forms.  Both operands of either product are split  x = h + m + l  into bf16
parts and a 16-query k-slot of a product is six v_mfma_f32_32x32x16_bf16 into the f32 accumulator, A = the dO / q' planes,
B = the P / dS planes, in the order (A, B) = m m, l h, h l, m h, h m, h h.  The 16 queries of k-slot t of a tile are the
rows of accumulator registers 8t .. 8t+7 of the two lane halves ("packed-accumulator order"):
    half 0: 16t + 0..3, 16t + 8..11      half 1: 16t + 4..7, 16t + 12..15
-- B comes out of the accumulator in that order, so the A fragments must be read in it too.

The yardstick is not a closed-form bound but the f32 kernel itself (the parent's code): per element
    figure = worst |got - fp64| / A,     A_dv = sum_i P |dO|,   A_dk = scale * sum_i |dS| |q|
and the split-bf16 variant must stay within FACTOR = 2 of the f32 variant's figure on the same call.  The six-product dot
product is measured at 1.5e-6 against 2.6e-6 for the f32 MFMA (tools/ubench_bf16x6.hip), so it should not be worse; the
factor covers the different summation depth (16 queries per MFMA against 2).  A lost partial product costs about 2^-16
relative, some hundred times that.  Elements whose A is 0 in fp64 (one key: dS = 0 in real arithmetic) have no ratio;
there the absolute errors are compared, by the same factor.
"""
import torch

from attn_x6_ref import LOG2E32, split3

F64 = torch.float64
FACTOR = 2.0
LN2_32 = 0.6931471805599453
ORDER = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))   # (A plane, B plane): mfma6 of csrc/attn_fwd_x6.hip
FAMILIES = ("normal", "staircase")
MASKS = ("plain", "key_mask", "causal")
FILL = -1.0e9


def seeded(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(int(seed)))


def make_inputs(family, B, H, I, J, seed, D=64):
    """q, dO (B, H, I, D) and k, v (B, H, J, D), f32, on the CPU.  "staircase": the input of test_plain_kernel_staircase
    (tests/test_attention_x6_keep_gpu.py): the row maximum moves from 64-key tile to 64-key tile."""
    q, k, v, d_o = (seeded((B, H, T, D), seed + n) for n, T in enumerate((I, J, J, I)))
    if family == "staircase":
        u = torch.nn.functional.normalize(seeded((D,), seed + 4), dim=0)
        ramp = (torch.arange(J) // 64).float().view(1, 1, J, 1) / max(J // 64, 1)
        k = k * 0.3 + ramp * u * 70.0
        q = q + u * torch.linspace(0.0, 6.0, I).view(1, 1, I, 1)
    elif family != "normal":
        raise ValueError(family)
    return q.contiguous(), k.contiguous(), v.contiguous(), d_o.contiguous()


def make_masks(mode, B, I, J):
    """(key mask (B, J) uint8, 1 = keep; causal mask (I, J) uint8, 1 = masked) or None each.  The key mask blanks one
    whole 32-key wave of the kernel (keys 32..63 where there are that many) plus scattered keys."""
    km = cm = None
    if mode == "key_mask":
        km = torch.ones(B, J, dtype=torch.uint8)
        km[:, 32:64] = 0
        km[0, 2::5] = 0
        km[-1, 1::7] = 0
        km[:, 0] = 1          # every row keeps a key
    elif mode == "causal":
        cm = torch.ones(I, J).triu(1).to(torch.uint8)
    elif mode != "plain":
        raise ValueError(mode)
    return km, cm


def reference(q, k, v, d_o, scale, km=None, cm=None):
    """fp64 from the f32 inputs.  Returns a dict: dq, dk, dv, their scales A_dq, A_dk, A_dv, and P, dS (B, H, I, J)."""
    q, k, v, d_o = (t.to(F64) for t in (q, k, v, d_o))
    s = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    filled = torch.zeros_like(s, dtype=torch.bool)
    if km is not None:
        filled = filled | (km.to(s.device) == 0)[:, None, None, :]
    if cm is not None:
        filled = filled | (cm.to(s.device) != 0)[None, None]
    p = torch.softmax(s.masked_fill(filled, FILL), dim=-1)
    dp = torch.einsum("bhid,bhjd->bhij", d_o, v)
    ds = (p * (dp - (p * dp).sum(-1, keepdim=True))).masked_fill(filled, 0.0)
    return dict(
        P=p, dS=ds,
        dv=torch.einsum("bhij,bhid->bhjd", p, d_o), A_dv=torch.einsum("bhij,bhid->bhjd", p, d_o.abs()),
        dk=scale * torch.einsum("bhij,bhid->bhjd", ds, q), A_dk=scale * torch.einsum("bhij,bhid->bhjd", ds.abs(), q.abs()),
        dq=scale * torch.einsum("bhij,bhjd->bhid", ds, k), A_dq=scale * torch.einsum("bhij,bhjd->bhid", ds.abs(), k.abs()),
    )


def figure(got, want, A):
    """(worst |got - want| / A over the elements with A > 0, worst |got - want| over the elements with A == 0)."""
    err = (got.detach().to("cpu", F64) - want.cpu()).abs()
    A = A.cpu()
    pos = A > 0
    rel = float((err[pos] / A[pos]).max()) if bool(pos.any()) else 0.0
    zero = float(err[~pos].max()) if bool((~pos).any()) else 0.0
    return rel, zero


def within_factor(fig_x6, fig_f32):
    """The split-bf16 figure against the f32 variant's, both parts."""
    return fig_x6[0] <= FACTOR * fig_f32[0] and fig_x6[1] <= FACTOR * fig_f32[1]


def slot_rows(t, packed=True):
    """Queries (rows of a 32-query tile) of k-slot t in the order the MFMA sums them: lane half 0's eight, then half 1's."""
    if not packed:
        return list(range(16 * t, 16 * t + 16))
    return [16 * t + 4 * hf + (j & 3) + 8 * (j >> 2) for hf in (0, 1) for j in range(8)]


def kernel_operands(q, d_o, ref, scale):
    """The f32 operands of the two products: (dO, P) and (q', dS'), dS' = dS / (scale * ln 2 * log2 e) as the kernel holds it
    (P (dP - delta), no scale), all rounded to f32 from the fp64 reference."""
    qscale = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E32, dtype=torch.float32)
    return (d_o.float(), ref["P"].float()), (q.float() * qscale, ref["dS"].float())


def emulate_x6(x, y, order=ORDER, natural_slot=None, per_product=False):
    """out[b, h, j, d] = sum_i x[b, h, i, d] y[b, h, i, j] the kernel's way, on the CPU: tiles of 32 queries, two k-slots,
    six MFMAs per slot in `order`.  The products (bf16 x bf16) are exact in f32; where an MFMA rounds inside its 16-product
    sum is not specified, so there are two models: the sum formed exactly (fp64) and rounded once into the f32 accumulator,
    or, per_product, sixteen sequential f32 additions -- the most roundings it could have, as in tests/attn_x6_ref.py.
    natural_slot: that k-slot of every tile reads its A rows in natural order (a planted defect)."""
    xp, yp = split3(x), split3(y)
    B, H, I, D = x.shape
    acc = torch.zeros(B, H, y.shape[3], D, dtype=torch.float32)
    for i0 in range(0, I, 32):
        for t in (0, 1):
            rows_b = slot_rows(t)
            rows_a = slot_rows(t, packed=natural_slot != t)
            for pa, pb in order:
                wide = acc.to(F64)
                for ra, rb in zip(rows_a, rows_b):
                    if i0 + max(ra, rb) < I:      # rows past the sequence are zeros in the kernel
                        term = xp[pa][:, :, i0 + ra, None, :] * yp[pb][:, :, i0 + rb, :, None]
                        if per_product:
                            acc = acc + term
                        else:
                            wide = wide + term.to(F64)
                if not per_product:
                    acc = wide.float()
    return acc


def emulate_f32(x, y):
    """The same sum the f32 kernel's way (v_mfma_f32_32x32x2_f32): one fused multiply-add per query (a single rounding: the
    tighter yardstick), in the order of the accumulator registers r = 0..15 of a tile, lane half 0 then 1."""
    B, H, I, D = x.shape
    acc = torch.zeros(B, H, y.shape[3], D, dtype=torch.float32)
    for i0 in range(0, I, 32):
        for r in range(16):
            for hf in (0, 1):
                i = i0 + (r & 3) + 8 * (r >> 2) + 4 * hf
                if i < I:
                    acc = (acc.to(F64) + x[:, :, i, None, :].to(F64) * y[:, :, i, :, None].to(F64)).float()
    return acc
