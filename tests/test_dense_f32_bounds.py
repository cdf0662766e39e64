"""The checker of tests/test_dense_f32_bounds_gpu.py checks itself, without a GPU.

* An f32 emulation of every kernel of csrc/gemm_f32.hip (the MFMA chain in the kernel's order: contraction index
  BK kt + (BK / 2) hf + 4 s4 + x, both lane halves' products entering one accumulator; the LayerNorm fold's three
  roundings; expf and an IEEE division; the chunks of the weight gradient summed in order; the per-thread, 8-way and
  per-chunk sums of the bias gradient; the lane partials, butterfly and two passes of row_stats) stays within half of
  the hard bound of tests/dense_f32_ref.py on every input family and shape class, and defines the constants Q_EMU of
  the tight tier.
* Seventeen planted faults -- each a realistic slip of the kernels' indexing, staging or epilogues -- applied to the
  emulation are flagged by the new criteria on every family of the kernel they are planted in.
* test_old_criteria_report prints which of them the criteria of tests/test_dense_gpu.py (assert_close at 2e-5, the
  row_stats mean check) let pass, and on which family.
* expected_path equals a hand-written table, and the GPU case list reaches every kernel instance and every condition
  it is meant to reach on devices of 256 and of 304 compute units.
"""
import pytest
import torch

import dense_f32_ref as ref
import test_dense_f32_bounds_gpu as gpu_cases
from util import elementwise_violations, rel_err

F32 = torch.float32


# ---------------------------------------------------------------------------------------------- the emulation
def _fma(acc, a, b):
    """fl32(acc + a b) with one rounding (the product of two f32 is exact in fp64)."""
    return (acc.double() + a.double() * b.double()).to(F32)


def emu_chain(A, B, bk=32, acc=None, L=None):
    """acc + A (M, L) B (L, N) as the step loop of gemm_f32.hip contracts it: per step of bk, MFMA (s4, x) adds the
    products of index 4 s4 + x (lane half 0) and bk / 2 + 4 s4 + x (lane half 1) to the accumulator, one rounding each.
    Indices past L are staged as zeros (nothing is added)."""
    L = A.shape[1] if L is None else L
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=F32) if acc is None else acc
    for k0 in range(0, L, bk):
        for j in range(bk // 2):
            for k in (k0 + j, k0 + bk // 2 + j):
                if k < L:
                    acc = _fma(acc, A[:, k:k + 1], B[k:k + 1, :])
    return acc


def emu_fold(a, ln, gam=None, bet=None):
    """fmaf((a - mu) rs, gamma, beta) in f32."""
    mean, rstd, g0, b0 = ln
    gam, bet = g0 if gam is None else gam, b0 if bet is None else bet
    t = (a - mean.view(-1, 1)) * rstd.view(-1, 1)
    return (t.double() * gam.double() + bet.double()).to(F32)


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def emu_stats(x, mut=None):
    """row_stats_kernel: (mean, rstd).  mut one_pass_variance: E[x^2] - mean^2."""
    M, D = x.shape
    nch = ref.stats_nch(D)
    xp = torch.zeros(M, nch * 256, dtype=F32)
    xp[:, :D] = x
    v = xp.view(M, nch, 64, 4)                      # chunk c = lane + 64 j holds elements 4 c .. 4 c + 3
    live = (torch.arange(nch * 256).view(nch, 64, 4) < D)[:, :, 0]
    inv_d = torch.tensor(1.0 / D, dtype=F32)
    idx = torch.arange(64)

    def lanes_sum(terms):                           # terms (M, nch, 64): s += term_j per lane, then the butterfly
        s = torch.zeros(M, 64, dtype=F32)
        for j in range(nch):
            s = s + terms[:, j]
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, idx ^ o]
        return s[:, 0]

    mean = lanes_sum(((v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3]) * inv_d
    if mut == "one_pass_variance":
        sq = lanes_sum(((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]) + v[..., 3] * v[..., 3])
        var = sq * inv_d - mean * mean
    else:
        d = v - mean.view(M, 1, 1, 1)
        q = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]
        var = lanes_sum(torch.where(live, q, torch.zeros_like(q))) * inv_d
    return mean, torch.rsqrt(var + torch.tensor(1e-5, dtype=F32))


def emu_nt(a, w, bias=None, resid=None, ln=None, mut=None, bk=32):
    """gemm_nt_kernel / gemm_nt_dkernel with the BIAS / RESID epilogue."""
    M, K = a.shape
    N = w.shape[0]
    Kp = -(-K // bk) * bk
    A = torch.zeros(M, Kp, dtype=F32)
    W = torch.zeros(N, Kp, dtype=F32)
    W[:, :K] = w
    if ln is None:
        A[:, :K] = a
    else:
        gam, bet = torch.zeros(Kp), torch.zeros(Kp)       # (gamma and beta read as zeros past K: the tail stays zero)
        gam[:K], bet[:K] = ln[2], ln[3]
        if mut == "gamma_beta_wrong_step":                # the registers of the next step's gamma / beta
            gam, bet = torch.roll(gam, -bk), torch.roll(bet, -bk)
        araw = torch.zeros(M, Kp, dtype=F32)
        araw[:, :K] = a
        if mut == "ln_tail_leak":                         # no range check on the tail: the fold runs on the zeros with
            gam[K:], bet[K:] = ln[2][:Kp - K], ln[3][:Kp - K]     # whatever gamma / beta it finds, against the next row of W
            W[:-1, K:] = w[1:, :Kp - K]
        A = emu_fold(araw, ln, gam, bet)
    L = Kp
    if mut == "k_tail_dropped":
        L = K - K % bk
    elif mut == "last_step_dropped":
        L = Kp - bk
    acc = emu_chain(A, W.t(), bk, L=L)
    if bias is not None:
        acc = acc + bias
    if resid is not None:
        r = resid
        if mut == "resid_shifted_group":                  # the ring slot of the next 8-row group
            r = resid.clone()
            r[8:16] = resid[16:24]
        acc = acc + r
    # the faults of single rows are planted where the values are smallest (on scaled data: where a criterion relative to
    # the tensor's maximum looks least)
    if mut == "row_unwritten":
        acc[int(acc.abs().amax(1).argmin())] = 0.0
    elif mut == "group_unwritten":
        g8 = int(acc[:M // 8 * 8].abs().view(M // 8, -1).amax(1).argmin())
        acc[8 * g8:8 * g8 + 8] = 0.0
    elif mut == "block_from_neighbour":
        b32 = int(acc[:M // 32 * 32].abs().view(M // 32, -1).amax(1).argmin())
        acc[32 * b32:32 * b32 + 32, 0:32] = acc[32 * b32:32 * b32 + 32, 128:160]
    return acc


def emu_swiglu(a, w12, b12, ln=None, mut=None):
    """(g, ab) of the SwiGLU epilogue."""
    H = w12.shape[0] // 2
    ab = emu_nt(a, w12, b12, None, ln)
    av, bv = ab[:, :H], ab[:, H:]
    if mut == "silu_without_bias":
        av = av - b12[:H]
    if mut == "gate_pair_shift":
        bv = torch.roll(bv, -1, 1)
    return av * _sigmoid(av) * bv, ab


def emu_nn(a, w, a2=None, w2=None, mut=None, bk=32):
    """gemm_nn_kernel: the first segment's steps, then the second's."""
    acc = emu_chain(a, w, bk)
    if a2 is not None:
        if mut == "seg2_at_k":                            # a2 read at the contraction index k, not k - split (range-checked)
            K1, K2 = a.shape[1], a2.shape[1]
            sh = torch.zeros_like(a2)
            if K2 > K1:
                sh[:, :K2 - K1] = a2[:, K1:]
            a2 = sh
        acc = emu_chain(a2, w2, bk, acc)
    return acc


def emu_nn_bwd(dy, w3, ab, mut=None):
    H = w3.shape[1]
    g = emu_chain(dy, w3)
    a_, b_ = ab[:, :H], ab[:, H:]
    sg = _sigmoid(a_)
    sp = sg if mut == "silu_prime_without" else sg * (1.0 + a_ * (1.0 - sg))
    return torch.cat([g * b_ * sp, g * (a_ * sg)], 1)


def emu_tn(y, x, ln, spc, nchunk, mut=None, bk=32):
    """(dw, db) of gemm_tn_kernel + tn_reduce_kernel."""
    M = y.shape[0]
    X = emu_fold(x, ln) if ln is not None else x
    rows = spc * bk
    parts, bparts = [], []
    for c in range(nchunk):
        ys, xs = y[c * rows:(c + 1) * rows], X[c * rows:(c + 1) * rows]
        parts.append(emu_chain(ys.t(), xs, bk))
        pad = torch.zeros(-(-ys.shape[0] // 8) * 8, y.shape[1], dtype=F32)
        pad[:ys.shape[0]] = ys
        th = torch.zeros(8, y.shape[1], dtype=F32)        # thread cr sums the rows cr (mod 8) in order
        for r in pad.view(-1, 8, y.shape[1]):
            th = th + r
        s = torch.zeros(y.shape[1], dtype=F32)
        for j in range(8):
            s = s + th[j]
        bparts.append(s)
    if nchunk == 1:
        return parts[0], bparts[0]
    order = list(range(nchunk))
    if mut == "chunk_missing":
        order.remove(nchunk // 2)
    elif mut == "chunk8_twice":
        order.insert(8, 8)
    dw, db = torch.zeros_like(parts[0]), torch.zeros_like(bparts[0])
    for c in order:
        dw = dw + parts[c]
    for c in ([0] if mut == "dbias_chunk0" else range(nchunk)):
        db = db + bparts[c]
    return dw, db


# ---------------------------------------------------------------------------------------------- cases
def _cpu_ln(a, D):
    mean, rstd = emu_stats(a)
    return (mean, rstd, D["gamma"], D["beta"])


# kernel -> (families, shape)
G, LN, SW = ref.GEMM_FAMILIES, ref.LN_FAMILIES, ref.SWIGLU_FAMILIES
KERNELS = {
    "nt": (G, (140, 170, 36)), "nt_plain": (G, (140, 170, 60)), "nt_ln": (LN, (140, 170, 36)), "nt_walk": (G, (140, 170, 100)), "nt_walk_ln": (LN, (140, 170, 132)),
    "nt_walk_long": (G, (24, 40, 1368)), "nt_walk_long_ln": (LN, (24, 40, 1368)), "nt2": (G, (140, 128, 100, 100)), "swiglu": (SW, (70, 68, 100)),
    "swiglu_ln": (("unit", "saturate"), (70, 36, 36)), "nn": (G, (140, 172, 100)), "nn_seg": (G, (140, 172, 36, 100)),
    "nn_bwd": (SW, (70, 68, 40)), "nn_bwd_k256": (SW, (40, 36, 256)), "swiglu_k260": (SW, (40, 36, 260)), "tn": (G, (600, 132, 36)), "tn_ln": (LN, (600, 36, 132)), "tn9": (G, (2592, 36, 20)),
    "stats4": (LN, (40, 4)), "stats260": (LN, (40, 260)), "stats260_off": (LN, (40, 260)), "stats1028": (LN, (24, 1028)),
}
_CACHE = {}


def case(kernel, family, mut=None):
    """[(output name, Q_EMU key, emulated result, reference dict)] of one kernel, family and planted fault."""
    key = (kernel, family, mut)
    if key in _CACHE:
        return _CACHE[key]
    shape = KERNELS[kernel][1]
    seed = 100 + len(kernel)
    if kernel.startswith("nt") and kernel != "nt2":
        M, N, K = shape
        D = ref.make_nt(family, M, N, K, seed)
        ln = _cpu_ln(D["a"], D) if kernel.endswith("_ln") else None
        plain = kernel in ("nt_walk_long", "nt_walk_long_ln", "nt_plain")
        b, r = (None, None) if plain else (D["bias"], D["resid"])
        got = emu_nt(D["a"], D["w"], b, r, ln, mut)
        out = [("c", "nt" if K <= 96 else "nt_walk", got, ref.ref_nt(D["a"], D["w"], b, r, ln))]
    elif kernel == "nt2":
        M, N1, N2, K = shape
        D = ref.make_nt(family, M, N1 + N2, K, seed)
        w1, w2, b1, b2 = D["w"][:N1], D["w"][N1:], D["bias"][:N1], D["bias"][N1:]
        R = ref.ref_nt2(D["a"], w1, b1, w2, b2)
        c1 = emu_nt(D["a"], w1, b1)
        c2 = emu_nt(D["a"], w2, b1[:N2] if mut == "bias_other_segment" else b2)
        out = [("c", "nt_walk", c1, R), ("c2", "nt_walk", c2, R)]
    elif kernel.startswith("swiglu"):
        M, H, K = shape
        D = ref.make_swiglu(family, M, H, K, seed)
        ln = _cpu_ln(D["a"], D) if kernel.endswith("_ln") else None
        g, ab = emu_swiglu(D["a"], D["w"], D["bias"], ln, mut)
        R = ref.ref_nt_swiglu(D["a"], D["w"], D["bias"], ln)
        out = [("g", "nt_swiglu", g, R), ("ab", "nt" if K <= 96 else "nt_walk", ab, R)]
    elif kernel in ("nn", "nn_seg"):
        M, N, K, K2 = shape if len(shape) == 4 else shape + (0,)
        D = ref.make_nn(family, M, N, K, seed, K2)
        got = emu_nn(D["a"], D["w"], D.get("a2"), D.get("w2"), mut)
        out = [("c", "nn", got, ref.ref_nn(D["a"], D["w"], D.get("a2"), D.get("w2")))]
    elif kernel.startswith("nn_bwd"):
        M, H, K = shape
        D = ref.make_swiglu_bwd(family, M, H, K, seed)
        out = [("dab", "nn_swiglu_bwd", emu_nn_bwd(D["dy"], D["w3"], D["ab"], mut), ref.ref_nn_swiglu_bwd(D["dy"], D["w3"], D["ab"]))]
    elif kernel.startswith("tn"):
        M, N, K = shape
        D = ref.make_tn(family, M, N, K, seed)
        P = ref.expected_path("tn", "bias", M, N, K, 0, kernel == "tn_ln", 256)
        ln = _cpu_ln(D["x"], D) if kernel == "tn_ln" else None
        dw, db = emu_tn(D["y"], D["x"], ln, P["steps_per_chunk"], P["nchunk"], mut)
        R = ref.ref_tn(D["y"], D["x"], None, ln, True, P["steps_per_chunk"], P["nchunk"])
        out = [("dw", "tn_dw", dw, R), ("db", "tn_db", db, R)]
    else:
        M, Dm = shape
        x = ref.make_act(family, M, Dm, seed)
        if kernel.endswith("_off"):                    # every row moved 200 x its largest element away from zero
            x = x + 200.0 * x.abs().amax(1, keepdim=True)
        mean, rstd = emu_stats(x, mut)
        R = ref.ref_row_stats(x)
        out = [("mean", "row_stats_mean", mean, R), ("rstd", "row_stats_rstd", rstd, R)]
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("kernel,family", [(k, f) for k, (fams, _) in KERNELS.items() for f in fams])
def test_emulation_within_half_the_hard_bound(kernel, family):
    for name, key, got, R in case(kernel, family):
        nbad, ratio, q = ref.measures(got, R, name)
        assert nbad == 0 and ratio <= 0.5, f"{kernel}/{family} {name}: the emulation reaches {ratio:.3f} of the hard bound"
        assert q <= ref.Q_EMU[key], f"{kernel}/{family} {name}: q {q:.3f} above Q_EMU[{key}] = {ref.Q_EMU[key]}"


def test_emulation_defines_q(capsys):
    """Q_EMU is the emulation's worst q per kernel over every family and shape class, rounded up by at most a tenth:
    the tight tier's measure is this emulation, never the kernel."""
    worst = {}
    for kernel, (fams, _) in KERNELS.items():
        for fam in fams:
            for name, key, got, R in case(kernel, fam):
                worst[key] = max(worst.get(key, 0.0), ref.measures(got, R, name)[2])
    with capsys.disabled():
        print("\nemulation worst q:", {k: round(v, 4) for k, v in worst.items()})
    assert set(worst) == set(ref.Q_EMU)
    for key, q in worst.items():
        assert q <= ref.Q_EMU[key] <= 1.1 * q, f"Q_EMU[{key}] = {ref.Q_EMU[key]} against the emulation's {q:.4f}"


def test_under_allowance_only_on_saturate():
    """The `under` allowance is zero on every family but saturate, and there it covers under 5 % of the elements."""
    for kernel, name in (("swiglu", "g"), ("swiglu_ln", "g"), ("nn_bwd", "dab")):
        for fam in KERNELS[kernel][0]:
            R = case(kernel, fam)[0][3]
            used = (R["under_" + name] > 0).double().mean().item()
            if fam == "saturate":
                assert 0 < used < 0.05, (kernel, fam, used)
            else:
                assert used == 0, (kernel, fam, used)


# ---------------------------------------------------------------------------------------------- planted faults
# fault -> (kernel, families it must be flagged on): every family of the kernel.  The one-pass variance E[x^2] - mean^2
# is as accurate as the two-pass form while |mean| is small against the spread, so it is planted on rows moved away from
# zero (stats260_off), where it is wrong on every family.
FAULTS = {
    "k_tail_dropped": ("nt_walk", G),
    "last_step_dropped": ("nt_walk", G),
    "row_unwritten": ("nt_plain", G),
    "group_unwritten": ("nt_ln", LN),
    "block_from_neighbour": ("nt_plain", G),
    "bias_other_segment": ("nt2", G),
    "resid_shifted_group": ("nt_walk", G),
    "ln_tail_leak": ("nt_walk_ln", LN),
    "gamma_beta_wrong_step": ("nt_walk_ln", LN),
    "one_pass_variance": ("stats260_off", LN),
    "silu_without_bias": ("swiglu", SW),
    "silu_prime_without": ("nn_bwd", SW),
    "gate_pair_shift": ("swiglu", SW),
    "chunk_missing": ("tn9", G),
    "chunk8_twice": ("tn9", G),
    "dbias_chunk0": ("tn9", G),
    "seg2_at_k": ("nn_seg", G),
}


def _flagged(kernel, family, mut):
    return sum(ref.violations(got, R, name, key) for name, key, got, R in case(kernel, family, mut)) > 0


def _changed(kernel, family, mut):
    return any(not torch.equal(g1, g0) for (_, _, g1, _), (_, _, g0, _) in zip(case(kernel, family, mut), case(kernel, family)))


@pytest.mark.parametrize("fault,family", [(m, f) for m, (_, fams) in FAULTS.items() for f in fams])
def test_planted_fault_is_flagged(fault, family):
    kernel = FAULTS[fault][0]
    assert not _flagged(kernel, family, None)
    assert _changed(kernel, family, fault), f"{fault} changes nothing on {family} inputs"
    assert _flagged(kernel, family, fault), f"{fault} on {family} inputs passes the per-element check"


def _old_passes(kernel, family, mut):
    """The criteria of tests/test_dense_gpu.py before this check: assert_close at 2e-5 on every output (global maximum
    plus the 1e-4 |ref| + 1e-5 max|ref| floor); for the row_stats mean rel_err < 1e-5 or max|mean| < 1e-6."""
    for name, key, got, R in case(kernel, family, mut):
        r = R[name]
        if key == "row_stats_mean":
            ok = rel_err(got, r) < 1e-5 or float(r.abs().max()) < 1e-6
        else:
            ok = rel_err(got, r) <= 2e-5 and elementwise_violations(got, r)[0] == 0
        if not ok:
            return False
    return True


def test_old_criteria_report(capsys):
    """Prints which planted faults the older criteria pass, on which family (nothing is asserted on the old criteria
    beyond there being such faults: that is why this check exists)."""
    report = {}
    for m, (kernel, _) in FAULTS.items():
        fams = [f for f in KERNELS[kernel][0] if _changed(kernel, f, m)]
        report[m] = {"kernel": kernel, "old_passes_on": [f for f in fams if _old_passes(kernel, f, m)],
                     "new_flags_on": [f for f in fams if _flagged(kernel, f, m)]}
    with capsys.disabled():
        print("\nplanted fault             kernel        assert_close(2e-5) passes on / per-element check flags on")
        for m, r in report.items():
            print(f"{m:25s} {r['kernel']:13s} {','.join(r['old_passes_on']) or '-'} / {','.join(r['new_flags_on']) or '-'}")
    assert sum(len(r["old_passes_on"]) for r in report.values()) > 0


# ---------------------------------------------------------------------------------------------- dispatch restatement
def test_expected_path_table():
    ep = ref.expected_path

    def row(P):
        return (P["instance"], P["tiles"], P["grid"], P["max_tiles"], P["min_tiles"], P["nchunk"], P["steps_per_chunk"])

    table = [
        (ep("nt", "bias", 1000, 192, 256), ("nt_walk<bias,0>", 16, 16, 1, 1, 0, 0)),
        (ep("nt", "bias", 1, 260, 96), ("nt<32,bias,0>", 3, 3, 1, 1, 0, 0)),
        (ep("nt", "bias", 1, 260, 100, ln=True), ("nt_walk<bias,1>", 3, 3, 1, 1, 0, 0)),
        (ep("nt", "swiglu", 1000, 1368, 256), ("nt_walk<swiglu,0>", 176, 176, 1, 1, 0, 0)),
        (ep("nt", "resid", 2305, 4036, 100, ln=True), ("nt_walk<resid,1>", 608, 512, 2, 1, 0, 0)),
        (ep("nt", "resid", 2305, 4036, 100, ln=True, cus=304), ("nt_walk<resid,1>", 608, 608, 1, 1, 0, 0)),
        (ep("nt", "bias", 3457, 2348, 128, split=1024), ("nt_walk<bias,0>", 532, 512, 2, 1, 0, 0)),
        (ep("nt", "bias", 4223, 4096, 128), ("nt_walk<bias,0>", 1056, 512, 3, 2, 0, 0)),
        (ep("nt", "bias", 4223, 4096, 128, bk=16), ("nt<16,bias,0>", 1056, 1056, 1, 1, 0, 0)),
        (ep("nt", "swiglu", 4223, 100, 128, ln=True, walk=False), ("nt<32,swiglu,1>", 66, 66, 1, 1, 0, 0)),
        (ep("nn", "bias", 257, 300, 24), ("nn<32,bias>", 9, 9, 1, 1, 0, 0)),
        (ep("nn", "swiglu_bwd", 1000, 1368, 256, bk=16), ("nn<16,swiglu_bwd>", 88, 88, 1, 1, 0, 0)),
        (ep("tn", "bias", 5000, 256, 512), ("tn<32,0>", 8, 144, 1, 1, 18, 9)),
        (ep("tn", "bias", 40000, 128, 128, ln=True), ("tn<32,1>", 1, 139, 1, 1, 139, 9)),
        (ep("tn", "bias", 40000, 128, 128, cus=304), ("tn<32,0>", 1, 139, 1, 1, 139, 9)),
        (ep("tn", "bias", 20000, 512, 512), ("tn<32,0>", 16, 256, 1, 1, 16, 40)),
        (ep("tn", "bias", 20000, 512, 640), ("tn<32,0>", 20, 500, 1, 1, 25, 25)),
        (ep("tn", "bias", 20000, 512, 640, cus=304), ("tn<32,0>", 20, 600, 1, 1, 30, 21)),
        (ep("tn", "bias", 200, 256, 128), ("tn<32,0>", 2, 2, 1, 1, 1, 7)),
        (ep("tn", "bias", 5000, 256, 512, bk=16), ("tn<16,0>", 8, 152, 1, 1, 19, 17)),
        (ep("tn", "bias", 2001, 256, 128), ("tn<32,0>", 2, 14, 1, 1, 7, 9)),
        (ep("tn", "bias", 2001, 256, 128, tn_slots=6), ("tn<32,0>", 2, 6, 1, 1, 3, 21)),
        (ep("tn", "bias", 2305, 256, 128, split=128), ("tn<32,0>", 2, 18, 1, 1, 9, 9)),
    ]
    for i, (P, want) in enumerate(table):
        assert row(P) == want, (i, row(P), want)
    stats = [(ep("row_stats", None, 5, D, 0)["nch"]) for D in (4, 256, 260, 1024, 1028, 4096)]
    assert stats == [1, 1, 4, 4, 16, 16]
    P = ep("row_stats", None, 65541, 4, 0)
    assert (P["grid"], P["max_tiles"]) == (16384, 2) and ep("row_stats", None, 65536, 4, 0)["max_tiles"] == 1


@pytest.mark.parametrize("cus", [256, 304])
def test_gpu_case_list_reaches_every_path(cus):
    cs = gpu_cases.cases(cus)
    assert len({c["id"] for c in cs}) == len(cs) and [c["id"] for c in cs] == [c["id"] for c in gpu_cases.cases(256)]
    got = set().union(*(gpu_cases.case_features(c, cus) for c in cs))
    missing = gpu_cases.required_features(cus) - got
    assert not missing, sorted(missing)
    # the reduced list of the child processes: the three products, every epilogue, a walk of two tiles per workgroup
    red = gpu_cases.reduced_cases(cus)
    inst = {gpu_cases.case_path(c, cus)["instance"] for c in red}
    assert {"nt_walk<resid,1>", "nt<32,bias,0>", "nt_walk<swiglu,1>", "nn<32,bias>", "nn<32,swiglu_bwd>", "tn<32,1>", "tn<32,0>"} <= inst
    assert max(gpu_cases.case_path(c, cus)["max_tiles"] for c in red if c["kind"] == "nt") >= 2
    assert {gpu_cases.case_path(c, cus, bk=16)["instance"].split("<")[1][:2] for c in red} == {"16"}
    tn = [c for c in red if c["id"] == "r_tn"][0]
    assert gpu_cases.case_path(tn, cus, tn_slots=6)["nchunk"] != gpu_cases.case_path(tn, cus)["nchunk"]
