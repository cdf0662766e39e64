"""fp64 references, per-element error bounds, input and routing families and a restatement of the host dispatch for
the MoE routing kernels and grouped expert GEMMs (csrc/moe.hip).

Every reference is computed in fp64 on the f32 values the kernel reads and takes the addressing arguments of the C ABI
(a_div, x_div, y_div, v_div, row strides, offsets, perm).  The only Python loop is over the experts (one fp64 matmul
each); nothing loops over pairs.  u32 = 2^-24.  No bound is relative to a tensor's maximum.

Hard tier (a theorem).  These are exact-f32 kernels: a result that is a sum of terms t_i formed by at most n rounded
f32 operations on any path from an input to the result -- in any order, fused or not -- satisfies
    |got - ref| <= gamma_n S + n 2^-126,   gamma_n = n u32 / (1 - n u32),   S = sum |t_i|
(the second term: flush-to-zero of each operation).  n per output, from the source:
* grouped_nt (narrow <1>, <1, short>, wide; Y = A W_e^T + b_e): the MFMA chain over Kd (one product and one add per
  k; the K tail and absent rows are staged as exact zeros), the short tile's fold of its two k-halves through LDS (1),
  the bias add (1):  n = Kd + 2,  S = |A| |W_e|^T + |b_e|.
* grouped_nn (Y = s (A W_e)): the chain over N, the short fold, the scale:  n = N + 2,  S = |s| |A| |W_e|.
* the accumulating forms add each pair's row into output row p / y_div with an f32 atomic, in any order: the terms of
  all pairs of the row and the value the row held before, n + (pairs of the row) <= n + y_div.
* grouped_wgrad (dW_e = sum_p s G^T (x) X): G is scaled at the LDS store (1), one product and one add per pair of the
  expert, and with rsplit 2 the two halves add into zeros (2):  n = cnt_e + 3,  S = sum_p |s| |G| |X|.  dbias: the
  scaled G summed per half-wave, the two half-waves added (1), the two halves (2):  n = cnt_e + 4, S = sum_p |s| |G|.
  An expert without pairs has S = 0: its dW and dbias are exactly zero.
* expert_sums (Z[g, e] = sum of s A over the row's pairs of expert e): a product and an add per pair,
  n = 2 (pairs of that expert in the row).
* gate_grad: 4 products per lane and step summed over N / 64 steps, the 16-lane fold (4), then acc g (1 - g) (3):
  n = N + 7,  S = g (1 - g) sum |dOut| |Y|; entries no slot selected are exactly zero.
* gate = 1 / (1 + expf(-v)): expf is within 1 ulp = 2 u32 (the HIP math API's stated maximum error for expf, the file
  is built without fast-math), which the sum 1 + e passes on scaled by (1 - s); the sum and the IEEE division round
  once each:  |gate - s| <= s ((1 - s) 2 u32 + 2 u32) + 2^-126.
Exact: ids, offsets, perm, the distinct lists; combine_kernel (rounds w y and every sum separately, ascending expert
id, then over `outer`: emu_combine repeats that in f32 and must match bitwise).

Tight tier.  The hard tier is 30 to 1000 times above what f32 arithmetic reaches; it sees structure, not lost
precision.  So q = (|got - ref| - n 2^-126) / (u32 S) is also held to TIGHT_FACTOR x the worst q that the f32 CPU
emulation of tests/test_moe_bounds.py (the kernel's chain: one product and add per k, folds and atomics as above)
reaches for that kernel over every family and shape class: the constants Q_EMU below, asserted there.

Measured on the MI355X (256 CUs), worst over tests/test_moe_bounds_gpu.py -- hard ratio, q / (4 Q_EMU):
    nt 0.351, 0.310    nt_acc 0.085, 0.275    nn 0.352, 0.455    nn_acc 0.090, 0.297
    dw 0.575, 0.323    db 0.386, 0.303        dlogits 0.205, 0.352    z (expert sums) 0.499, 0.549
The first run of the bitwise check found combine_kernel fusing acc + w y into v_pk_fma_f32 (its __fmul_rn / __fadd_rn
are plain * and + in the HIP headers and the default -ffp-contract=fast contracts them): the weighted sums over k >= 2
slots differed in their last bits from the separately rounded chain the source promises.  Fixed in csrc/moe.hip (contraction off
in that kernel); no fault was found in the routing kernels, the GEMMs, the gate gradient or the expert sums.

Input families (make_data): unit; expert_scale (expert e's weights and bias by 2^-round(20 e / (E - 1))); outlier_rows
(rows 0 and the middle of the activations at 64x and 16x); binade (activation rows and weight rows / columns by
powers of two over 2^-12 .. 2^12); cancel (the second half of the contraction nearly negates the first); gate_tiny
(the scale of some pairs down to 2^-20).  Routing families (make_lists): counts given per expert, shuffled over the
pairs, optionally sparse (offsets[E] < P, perm names some rows only).
"""
import numpy as np
import torch

U32 = 2.0 ** -24
FTZ = 2.0 ** -126
TIGHT_FACTOR = 4.0
F64 = torch.float64
DATA_FAMILIES = ("unit", "expert_scale", "outlier_rows", "binade", "cancel", "gate_tiny")

# worst q = |err| / (u32 S) of the f32 emulation per kernel (tests/test_moe_bounds.py::test_emulation_defines_q)
Q_EMU = {"nt": 7.7, "nn": 6.7, "nt_acc": 6.8, "nn_acc": 7.1, "dw": 16.1, "db": 5.5, "z": 2.7, "dlogits": 1.6}


def gamma(n):
    n = torch.as_tensor(n, dtype=F64)
    return n * U32 / (1 - n * U32)


def hard_bound(n, S):
    n = torch.as_tensor(n, dtype=F64, device=S.device)
    return gamma(n).to(S.device) * S + n * FTZ


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def take_rows(buf, ld, rows, width):
    """fp64 (len(rows), width): row r of a buffer with row stride ld (in elements)."""
    idx = rows.view(-1, 1) * int(ld) + torch.arange(width, device=buf.device)
    return buf.reshape(-1)[idx].to(F64)


def named_pairs(offsets, perm, E):
    """(pairs named by the lists, their experts, per-expert counts), int64, on the lists' device."""
    off = offsets.long()
    cnt = off[1:E + 1] - off[:E]
    pp = perm[:int(off[E])].long()
    ee = torch.repeat_interleave(torch.arange(E, device=off.device), cnt)
    return pp, ee, cnt


# ---------------------------------------------------------------------------------------------- references
def ref_topk(logits, k):
    """(ids (U, k), gate ref fp64, gate bound): stable descending order, lowest index first."""
    v, i = torch.sort(logits, dim=1, descending=True, stable=True)
    v, i = v[:, :k].to(F64), i[:, :k]
    s = torch.sigmoid(v)
    return i, s, s * ((1 - s) * 2 * U32 + 2 * U32) + FTZ


def ref_route(ids, E):
    """(offsets (E + 1) int32, perm (P) int32) of amk_moe_route: pairs by expert, ascending pair id inside one."""
    flat = ids.reshape(-1)
    cnt = torch.bincount(flat, minlength=E)
    off = torch.zeros(E + 1, dtype=torch.int64, device=ids.device)
    off[1:] = torch.cumsum(cnt, 0)
    return off.int(), torch.sort(flat, stable=True)[1].int()


def ref_route_distinct(ids, G, fan, E):
    """(offsets, perm) of amk_moe_route_distinct: virtual pairs g E + e, by expert, ascending g."""
    m = torch.zeros(G, E, dtype=torch.bool, device=ids.device)
    m[torch.arange(G, device=ids.device).repeat_interleave(fan), ids.reshape(-1)] = True
    e, g = torch.nonzero(m.t(), as_tuple=True)      # row-major over (e, g): e ascending, g ascending inside
    off = torch.zeros(E + 1, dtype=torch.int64, device=ids.device)
    off[1:] = torch.cumsum(m.sum(0), 0)
    return off.int(), (g * E + e).int()


def _grouped(kind, A, lda, a_div, W, vec, offsets, perm, P, E, N, Kd, y_div, y0):
    pp, ee, cnt = named_pairs(offsets, perm, E)
    dev = W.device
    win, wout = (Kd, N) if kind == "nt" else (N, Kd)
    Y = torch.zeros(pp.numel(), wout, dtype=F64, device=dev)
    S = torch.zeros_like(Y)
    off = offsets.long().tolist()
    W64 = W.reshape(E, N, Kd)
    for e in range(E):
        lo, hi = off[e], off[e + 1]
        if hi == lo:
            continue
        rows = pp[lo:hi]
        a = take_rows(A, lda, rows // a_div, win)
        w = W64[e].to(F64)
        w = w.t() if kind == "nt" else w
        y, s = a @ w, a.abs() @ w.abs()
        if vec is not None:
            if kind == "nt":
                b = vec.reshape(E, N)[e].to(F64)
                y, s = y + b, s + b.abs()
            else:
                sc = vec.reshape(-1)[rows].to(F64).view(-1, 1)
                y, s = y * sc, s * sc.abs()
        Y[lo:hi], S[lo:hi] = y, s
    n = win + 2
    if y_div == 0:
        ref = torch.full((P, wout), float("nan"), dtype=F64, device=dev)
        Sf = torch.zeros(P, wout, dtype=F64, device=dev)
        ref[pp], Sf[pp] = Y, S
        named = torch.zeros(P, dtype=torch.bool, device=dev)
        named[pp] = True
    else:
        rows_out = (P - 1) // y_div + 1
        ref = torch.zeros(rows_out, wout, dtype=F64, device=dev) if y0 is None else y0.to(F64).clone()
        Sf = ref.abs()
        ref.index_add_(0, pp // y_div, Y)
        Sf.index_add_(0, pp // y_div, S)
        named = torch.bincount(pp // y_div, minlength=rows_out) > 0
        n = n + y_div
    return {"y": ref, "S_y": Sf, "n_y": n, "bound_y": hard_bound(n, Sf), "named_y": named}


def ref_nt(A, lda, a_div, W, bias, offsets, perm, P, E, N, Kd, y_div=0, y0=None):
    """amk_grouped_gemm_nt (y_div 0) / _nt_acc: {"y", "S_y", "n_y", "bound_y", "named_y"}; rows the lists do not
    name are NaN in "y" (y_div 0) or hold y0 (accumulating form)."""
    return _grouped("nt", A, lda, a_div, W, bias, offsets, perm, P, E, N, Kd, y_div, y0)


def ref_nn(A, lda, a_div, W, scale, offsets, perm, P, E, N, Kd, y_div=0, y0=None):
    """amk_grouped_gemm_nn / _nn_acc, as ref_nt."""
    return _grouped("nn", A, lda, a_div, W, scale, offsets, perm, P, E, N, Kd, y_div, y0)


def ref_wgrad(G, ldg, g_div, X, ldx, x_div, scale, offsets, perm, P, E, N, Kd):
    """amk_grouped_gemm_wgrad: {"dw" (E, N, Kd), "db" (E, N)} with S_, n_ (per expert) and bound_."""
    pp, ee, cnt = named_pairs(offsets, perm, E)
    dev = G.device
    dw = torch.zeros(E, N, Kd, dtype=F64, device=dev)
    Sw = torch.zeros_like(dw)
    db = torch.zeros(E, N, dtype=F64, device=dev)
    Sb = torch.zeros_like(db)
    off = offsets.long().tolist()
    for e in range(E):
        lo, hi = off[e], off[e + 1]
        if hi == lo:
            continue
        rows = pp[lo:hi]
        g = take_rows(G, ldg, rows // g_div, N)
        if scale is not None:
            g = g * scale.reshape(-1)[rows].to(F64).view(-1, 1)
        x = take_rows(X, ldx, rows // x_div, Kd)
        dw[e], Sw[e] = g.t() @ x, g.abs().t() @ x.abs()
        db[e], Sb[e] = g.sum(0), g.abs().sum(0)
    c = cnt.to(F64)
    nw, nb = (c + 3).view(E, 1, 1), (c + 4).view(E, 1)
    return {"dw": dw, "S_dw": Sw, "n_dw": nw, "bound_dw": hard_bound(nw, Sw),
            "db": db, "S_db": Sb, "n_db": nb, "bound_db": hard_bound(nb, Sb)}


def ref_expert_sums(A, lda, a_div, ids, scale, G, fan, E, d):
    """amk_moe_expert_sums: {"z" (G, E d), ...}."""
    dev = A.device
    p = torch.arange(G * fan, device=dev)
    a = take_rows(A, lda, p // a_div, d)
    if scale is not None:
        a = a * scale.reshape(-1).to(F64).view(-1, 1)
    slot = (p // fan) * E + ids.reshape(-1)
    z = torch.zeros(G * E, d, dtype=F64, device=dev)
    S = torch.zeros_like(z)
    z.index_add_(0, slot, a)
    S.index_add_(0, slot, a.abs())
    n = (2 * torch.bincount(slot, minlength=G * E)).to(F64).view(-1, 1).expand(G * E, d)
    return {"z": z.view(G, E * d), "S_z": S.view(G, E * d), "n_z": n.reshape(G, E * d),
            "bound_z": hard_bound(n, S).view(G, E * d)}


def _y_rows(ids, v_div, E):
    p = torch.arange(ids.numel(), device=ids.device)
    return (p // v_div) * E + ids.reshape(-1) if v_div else p


def ref_gate_grad(d_out, Y, ids, gate, P, k, E, N, g_div, v_div=0):
    """amk_moe_gate_grad / _rows: {"dlogits" (P / k, E), ...}; entries no slot selected have S = 0 (exactly zero)."""
    dev = Y.device
    p = torch.arange(P, device=dev)
    a = d_out.reshape(-1, N)[p // g_div].to(F64)
    y = Y.reshape(-1, N)[_y_rows(ids, v_div, E)].to(F64)
    g = gate.reshape(-1).to(F64)
    f = g * (1 - g)
    dl = torch.zeros(P // k, E, dtype=F64, device=dev)
    S = torch.zeros_like(dl)
    idx = (p // k, ids.reshape(-1))
    dl[idx] = f * (a * y).sum(1)
    S[idx] = f.abs() * (a.abs() * y.abs()).sum(1)
    return {"dlogits": dl, "S_dlogits": S, "n_dlogits": N + 7, "bound_dlogits": hard_bound(N + 7, S)}


def emu_combine(Y, ids, scale, G, outer, k, N, v_div=0, E=0, order="expert"):
    """combine_kernel in f32, operation by operation (bitwise): per unit the slots in ascending expert id (stable),
    acc = acc + w * y with both roundings, then the `outer` partial sums in order.  order="slot": the planted fault."""
    ids2 = ids.reshape(G * outer, k)
    o = torch.sort(ids2, dim=1, stable=True)[1] if order == "expert" else torch.arange(k, device=ids.device).expand(G * outer, k)
    p = torch.arange(G * outer, device=ids.device).view(-1, 1) * k + o          # (units, k) pairs in summation order
    rows = _y_rows(ids, v_div, E)[p]
    Y2 = Y.reshape(-1, N).float()
    acc = torch.zeros(G * outer, N, dtype=torch.float32, device=Y.device)
    for s in range(k):
        y = Y2[rows[:, s]]
        acc = acc + (y if scale is None else scale.reshape(-1).float()[p[:, s]].view(-1, 1) * y)
    acc = acc.view(G, outer, N)
    if outer == 1:
        return acc[:, 0]
    tot = torch.zeros(G, N, dtype=torch.float32, device=Y.device)
    for j in range(outer):
        tot = tot + acc[:, j]
    return tot


# ---------------------------------------------------------------------------------------------- checking
WORST = {}   # key -> [worst hard ratio, worst q / (TIGHT_FACTOR Q_EMU)] over every check of the process


def measures(got, R, name):
    """(elements outside the hard bound, worst |err| / hard bound, worst q) over the elements whose reference is not
    NaN (rows the lists do not name are checked by the caller against the canvas)."""
    ref = R[name]
    a = got.detach().to(ref.device, F64).reshape(ref.shape)
    live = ~torch.isnan(ref)
    err = (a - ref).abs()
    hb, S = R["bound_" + name], R["S_" + name]
    n = torch.as_tensor(R["n_" + name], dtype=F64, device=ref.device)
    bad = live & ~(err <= hb)                                     # (a NaN result is outside the bound too)
    zero = torch.zeros_like(err)
    ratio = torch.where(live & (err > 0), err / hb, zero)
    q = torch.where(live & (err > 0) & (S > 0), (err - n * FTZ).clamp_min(0) / (U32 * S), zero)
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return int(bad.sum()), float(ratio.max()) if a.numel() else 0.0, float(q.max()) if a.numel() else 0.0


def violations(got, R, name, kernel=None):
    """Number of elements that miss the hard tier, plus 1 if the tight tier (kernel given) is missed."""
    nbad, _, q = measures(got, R, name)
    return nbad + (1 if kernel is not None and q > TIGHT_FACTOR * Q_EMU[kernel] else 0)


def assert_within(got, R, name, kernel, what=""):
    """Both tiers on every element; records the worst figures in WORST[kernel]."""
    nbad, ratio, q = measures(got, R, name)
    lim = TIGHT_FACTOR * Q_EMU[kernel]
    w = WORST.setdefault(kernel, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], q / lim)
    print(f"{what} {name}: hard ratio {ratio:.4g}, q {q:.4g} (limit {lim:.4g})")
    assert nbad == 0, f"{what} {name}: {nbad} elements outside the hard bound (worst {ratio:.3g}x)"
    assert q <= lim, f"{what} {name}: q = |err| / (u32 S) reaches {q:.3g}, limit {lim:.3g} ({TIGHT_FACTOR} x the emulation)"


# ---------------------------------------------------------------------------------------------- input families
def make_lists(counts, P=None, seed=0):
    """ids (P) int64 (-1: a row no list names), offsets (E + 1) int32, perm int32 for the given per-expert counts,
    the experts dealt over the named pairs at random; P > sum(counts): a sparse list."""
    g = _gen(seed)
    cnt = torch.as_tensor(counts, dtype=torch.int64)
    L, E = int(cnt.sum()), cnt.numel()
    P = L if P is None else P
    rows = torch.sort(torch.randperm(P, generator=g)[:L])[0]
    lab = torch.repeat_interleave(torch.arange(E), cnt)[torch.randperm(L, generator=g)]
    ids = torch.full((P,), -1, dtype=torch.int64)
    ids[rows] = lab
    off = torch.zeros(E + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(cnt, 0)
    return ids, off.int(), rows[torch.sort(lab, stable=True)[1]].int()


def skewed_counts(P, E, seed=0):
    """Counts proportional to 2^(-e / 2), summing to P: a few long experts next to ones of a handful of pairs."""
    w = torch.exp2(-torch.arange(E, dtype=F64) / 2)
    c = torch.floor(w / w.sum() * P).long()
    c[0] += P - int(c.sum())
    return c.tolist()


def _pow2(lo, hi, n, g):
    return torch.exp2(torch.randint(lo, hi + 1, (n,), generator=g).float())


def make_data(family, P, E, N, Kd, a_div, x_div, seed, lda=None, ldn=None, ldx=None):
    """A (rows_a, lda) nt input, W (E, N, Kd), bias (E, N), Gm (rows_a, ldn) nn / wgrad input, X (rows_x, ldx),
    scale (P): f32.  Row strides default to the row lengths; the columns past a row's length hold NaN."""
    g = _gen(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    ra, rx = (P - 1) // a_div + 1, (P - 1) // x_div + 1
    A, W, bias, Gm, X = n(ra, Kd), n(E, N, Kd), n(E, N), n(ra, N), n(rx, Kd)
    scale = torch.sigmoid(n(P))
    if family == "expert_scale":
        s = torch.exp2(-torch.round(20.0 * torch.arange(E) / max(E - 1, 1)))
        W, bias = W * s.view(E, 1, 1), bias * s.view(E, 1)
    elif family == "outlier_rows":
        for T in (A, Gm, X):
            T[0] *= 64.0
            T[T.shape[0] // 2] *= 16.0
    elif family == "binade":
        A, Gm, X = A * _pow2(-12, 12, ra, g).view(-1, 1), Gm * _pow2(-12, 12, ra, g).view(-1, 1), X * _pow2(-12, 12, rx, g).view(-1, 1)
        W = W * _pow2(-12, 12, N, g).view(1, N, 1) * _pow2(-6, 6, Kd, g).view(1, 1, Kd)
        bias = bias * _pow2(-12, 12, N, g)
    elif family == "cancel":
        h, hn = Kd // 2, N // 2
        A[:, h:2 * h] = A[:, :h]
        W[:, :, h:2 * h] = -W[:, :, :h] + n(E, N, h) / 64
        Gm[:, hn:2 * hn] = Gm[:, :hn]
        W[:, hn:2 * hn, :] = -W[:, :hn, :] + n(E, hn, Kd) / 64
        bias = bias / 64
    elif family == "gate_tiny":
        scale = scale * torch.where(torch.rand(P, generator=g) < 0.5, _pow2(-20, 0, P, g), torch.ones(P))
    elif family != "unit":
        raise ValueError(family)

    def pad(T, ld):
        if ld is None or ld == T.shape[1]:
            return T.contiguous()
        out = torch.full((T.shape[0], ld), float("nan"))
        out[:, :T.shape[1]] = T
        return out
    return {"A": pad(A, lda), "W": W.contiguous(), "bias": bias.contiguous(), "Gm": pad(Gm, ldn), "X": pad(X, ldx),
            "scale": scale.contiguous()}


# ---------------------------------------------------------------------------------------------- dispatch restatement
def _f(x):
    return np.float32(x)


def unit_plan(counts, ncol, slots):
    """find_unit_rb's choice for a launch: (m, units, nfull, r, split, [rb of every unit in unit order]); None
    without any pair."""
    nb = [(c + 31) >> 5 for c in counts]
    nbtot = sum(nb)
    U = {m: sum((b + m - 1) // m for b in nb) for m in (2, 3, 4)}
    best, mbest = _f(3.0e38), 4
    for m in (4, 3, 2):
        u = U[m] * ncol
        if u == 0:
            return None
        blocks = _f(nbtot * ncol) / _f(u)
        full, r = divmod(u, slots)
        tail = _f(0) if r == 0 else (_f(0.6) * blocks + _f(0.35) if 2 * r <= slots else blocks + _f(0.35))
        est = _f(full) * (blocks + _f(0.35)) + tail
        if est < best:
            best, mbest = est, m
    units = U[mbest] * ncol
    nfull = units // slots * slots
    r = units - nfull
    rbs = []
    for b in nb:
        parts = (b + mbest - 1) // mbest
        if parts:
            bs, extra = divmod(b, parts)
            rbs += [bs + (1 if i < extra else 0) for i in range(parts)] * ncol
    return mbest, units, nfull, r, (r > 0 and 2 * r <= slots), rbs


def _wide_name(head, counts, ncol, slots):
    plan = unit_plan(counts, ncol, slots)
    if plan is None:
        return head + " empty"
    m, units, nfull, r, split, rbs = plan
    return f"{head} m{m} full{int(nfull > 0)} tail_{'split' if split else ('whole' if r else 'none')}"


def expected_path(entry, P, E, N, Kd, y_div, counts, slots, env=()):
    """The kernel instantiation and mode the host code of csrc/moe.hip picks.  entry: nt, nn (y_div > 0: the
    accumulating forms), wgrad, wgrad_noscale; env: names of the set environment variables (AMK_MOE_NARROW).  Buffers
    are taken to be below the 2 GB that the buffer descriptors of the wide kernels span (the host code's other condition)."""
    narrow_env = "AMK_MOE_NARROW" in env
    short_fits = (P + 63) // 64 < 16 * slots // 2
    if entry == "nt":
        if N >= 128 and Kd % 32 == 0 and (y_div > 0 or not narrow_env):
            return _wide_name("nt_wide_acc" if y_div else "nt_wide", counts, (N + 127) // 128, slots)
        assert y_div == 0, "the accumulating form needs the wide kernel"
        return "nt_narrow<1,short>" if N <= 64 and Kd >= 256 and short_fits else "nt_narrow<1>"
    if entry == "nn":
        if Kd >= 128 and N % 32 == 0 and (y_div > 0 or not narrow_env):
            return _wide_name("nn_wide_acc" if y_div else "nn_wide", counts, (Kd + 127) // 128, slots)
        assert y_div == 0, "the accumulating form needs the wide kernel"
        if Kd > 64:
            return "nn_narrow<2>"
        return "nn_narrow<1,short>" if N >= 256 and short_fits else "nn_narrow<1>"
    if entry in ("wgrad", "wgrad_noscale"):
        if N >= 64 and Kd >= 64 and N + Kd >= 192 and not narrow_env:
            tn, tk = (128 if N >= 128 else 64), (128 if Kd >= 128 else 64)
            nwg = E * ((N + tn - 1) // tn) * ((Kd + tk - 1) // tk)
            rs = 2 if 2 * nwg <= slots and P // E >= 256 else 1
            return f"wgrad_wide<{tn},{tk},{'scale' if entry == 'wgrad' else 'noscale'}> rsplit {rs}"
        return "wgrad<1>"
    raise ValueError(entry)


NT_PATHS = ["nt_narrow<1>", "nt_narrow<1,short>"]
NN_PATHS = ["nn_narrow<1>", "nn_narrow<1,short>", "nn_narrow<2>"]
WGRAD_PATHS = ["wgrad<1>"] + [f"wgrad_wide<{t},{s}> rsplit {r}" for t in ("128,128", "64,128", "128,64")
                              for s in ("scale", "noscale") for r in (1, 2)]
