"""CPU checks of the MoE checker (tests/moe_ref.py), no GPU needed.

Not too tight: an f32 emulation of each kernel's chain as read from csrc/moe.hip -- one rounded product and one
rounded add per k in k order (the short tile: its two k-halves {0..7, 16..23} and {8..15, 24..31} of every 32-deep
slab in two accumulators, folded at the end), the bias / scale after the chain, the accumulating forms' adds in a
random order, the weight gradient over the expert's pairs (rsplit 2: two halves added into zero; dbias per half-wave),
the gate gradient's 4-product groups per lane and 16-lane fold, the expert sums in pair order -- stays within half of
the hard bound on every family and shape class, and its worst q defines moe_ref.Q_EMU (asserted here).
Sensitive enough: the planted faults of MUTATIONS are flagged on at least the listed families.
test_old_criteria_report prints which of them the older criteria (max |got - want| <= 2e-5 max |want| of
test_moe_gemm_gpu.py, 1e-4 max |want| of test_moe_gpu.py) pass (AMK_MOE_OLD_REPORT=<file>: also as JSON).
expected_path is held against a hand-written table, and the GPU sweep's case list against the list of paths."""
import json
import os

import pytest
import torch

import moe_ref as ref

F32 = torch.float32
COUNTS = [1, 31, 33, 65, 97, 129, 0, 164]          # 520 pairs, E 8: partial tiles of every kind, one empty expert
E = len(COUNTS)
P = sum(COUNTS)
GEMM_FAMILIES = ref.DATA_FAMILIES[:5]
# kernel -> (N, Kd, a_div, x_div)
SHAPES = {"nt": (128, 100, 2, 2), "nt_short": (64, 256, 2, 2), "nt_acc": (128, 128, 2, 2), "nn": (128, 64, 2, 2),
          "nn_short": (256, 64, 2, 2), "nn_acc": (96, 128, 2, 2), "wgrad": (64, 64, 2, 4), "wgrad_split": (64, 128, 2, 4)}
Y_DIV = 8


def bf16_trunc(x):
    return (x.view(torch.int32) & -65536).view(F32)


def mant10(x):
    return (x.view(torch.int32) & -8192).view(F32)


# ---------------------------------------------------------------------------------------------- emulations
def _chain(a, Wk, ee, ksets):
    """sum over the k sets (one accumulator each, folded in order) of a[:, k] * Wk[k, ee]: a product and an add per k."""
    tot = None
    for ks in ksets:
        acc = torch.zeros(a.shape[0], Wk.shape[2], dtype=F32)
        for k in ks:
            acc = acc + a[:, k:k + 1] * Wk[k][ee]
        tot = acc if tot is None else tot + acc
    return tot


def _ksets(K, short):
    if not short:
        return [range(K)]
    h0 = [k for k in range(K) if (k % 16) < 8]
    return [h0, [k for k in range(K) if (k % 16) >= 8]]


def emu_grouped(kind, D, lists, N, Kd, a_div, short=False, y_div=0, mut=None):
    """The rows of the named pairs through grouped_{nt,nn}: (P or P / y_div, out) f32, rows not named NaN."""
    ids, off, perm = lists
    E, P = off.numel() - 1, ids.numel()
    pp, ee, cnt = ref.named_pairs(off, perm, E)
    pos = torch.arange(pp.numel()) - off.long()[ee]            # position of the pair inside its expert
    win, wout = (Kd, N) if kind == "nt" else (N, Kd)
    src = D["A"] if kind == "nt" else D["Gm"]
    rows = pp // a_div
    if mut == "a_div_ignored":
        rows = pp % src.shape[0]
    a = src[rows, :win].to(F32).clone()
    W = D["W"].to(F32)
    if mut == "operands_bf16":
        a, W = bf16_trunc(a), bf16_trunc(W)
    if mut == "operands_mant10":
        a, W = mant10(a), mant10(W)
    Wk = (W.permute(2, 0, 1) if kind == "nt" else W.permute(1, 0, 2)).contiguous()      # (win, E, wout)
    we = ee.clone()
    if mut == "weights_of_next_expert_first_tile":
        we = torch.where(pos < 32, (ee + 1) % E, ee)
    last = ee == int(torch.nonzero(cnt)[-1])
    if mut == "k_tail_dropped":
        a[last, 32 * (win // 32):] = 0.0
    if mut == "last_step_dropped":
        a[last, 32 * ((win - 1) // 32):] = 0.0
    y = _chain(a, Wk, we, _ksets(win, short))
    if kind == "nt":
        be = (ee + 1) % E if mut == "bias_of_next_expert" else ee
        y = y + D["bias"][be]
    else:
        sp = torch.roll(D["scale"], -1) if mut == "scale_of_next_pair" else D["scale"]
        y = y * sp[pp].view(-1, 1)
    if mut == "row_unwritten":
        y[int(torch.nonzero(last)[-1])] = 0.0
    if mut == "half_unit_writes_64":
        y[last, 64:] = 0.0
    if mut == "odd_rb_last_block_dropped":
        y[last & (pos >= 64) & (pos < 96), 64:] = 0.0
    if y_div == 0:
        out = torch.full((P, wout), float("nan"), dtype=F32)
        out[pp] = y
        return out
    out = torch.zeros((P - 1) // y_div + 1, wout, dtype=F32)
    order = torch.randperm(pp.numel(), generator=torch.Generator().manual_seed(3))      # the atomics' arrival order
    if mut == "acc_missing_pair":
        order = order[order != 5]
    if mut == "acc_adds_twice":
        order = torch.cat([order, torch.tensor([5])])
    r = pp[order] // y_div
    key = torch.sort(r, stable=True)
    rs, src_i = key[0], order[key[1]]
    j = torch.arange(rs.numel()) - torch.searchsorted(rs, rs)              # j-th arrival at its row
    for t in range(int(j.max()) + 1):
        m = j == t
        out[rs[m]] = out[rs[m]] + y[src_i[m]]
    return out


def emu_wgrad(D, lists, N, Kd, g_div, x_div, rsplit, use_scale=True, mut=None):
    ids, off, perm = lists
    E = off.numel() - 1
    o = off.long().tolist()
    dw, db = torch.zeros(E, N, Kd, dtype=F32), torch.zeros(E, N, dtype=F32)
    for e in range(E):
        rows = perm[o[e]:o[e + 1]].long()
        c = rows.numel()
        if c == 0:
            if mut == "empty_expert_unwritten":
                dw[e], db[e] = 1e-20, 1e-20
            continue
        g = D["Gm"][rows // g_div, :N].to(F32)
        gs = g * D["scale"][rows].view(-1, 1) if use_scale else g
        x = D["X"][rows // x_div, :Kd].to(F32)
        first = ((c + 63) >> 6) << 5 if rsplit == 2 else c
        parts_w, parts_b = [], []
        for lo, hi in ((0, min(first, c)), (min(first, c), c)):
            if mut == "rsplit_loses_pair" and lo > 0:
                lo += 1
            acc = torch.zeros(N, Kd, dtype=F32)
            bs = [torch.zeros(N, dtype=F32), torch.zeros(N, dtype=F32)]
            gb = g if mut == "dbias_without_scale" else gs
            for i in range(lo, hi):
                acc = acc + gs[i].view(-1, 1) * x[i].view(1, -1)
                h = ((i - lo) % 32) // 16
                bs[h] = bs[h] + gb[i]
            parts_w.append(acc)
            parts_b.append(bs[0] + bs[1])
        dw[e] = (0.0 + parts_w[0]) + parts_w[1] if rsplit == 2 else parts_w[0]
        db[e] = (0.0 + parts_b[0]) + parts_b[1] if rsplit == 2 else parts_b[0]
    return dw, db


def emu_expert_sums(A, a_div, ids, scale, G, fan, Ez, d, mut=None):
    p = torch.arange(G * fan)
    a = A[p // a_div, :d].to(F32) * scale.view(-1, 1)
    grp = p // (2 if mut == "fan_taken_as_k" else fan)
    z = torch.zeros(max(int(grp.max()) + 1, G) * Ez, d, dtype=F32)
    step = 2 if mut == "fan_taken_as_k" else fan
    for j in range(step):                                   # the j-th pair of every group: distinct slots
        sel = p[j::step]
        slot = grp[sel] * Ez + ids[sel]
        z[slot] = z[slot] + a[sel]
    return z[:G * Ez].view(G, Ez * d)


def emu_gate_grad(d_out, Y, ids, gate, Pg, k, Eg, N, g_div, mut=None):
    p = torch.arange(Pg)
    pr = d_out[p // g_div].to(F32) * Y[p].to(F32)
    pad = (-N) % 64
    pr = torch.cat([pr, torch.zeros(Pg, pad)], 1).view(Pg, -1, 16, 4)
    acc = torch.zeros(Pg, 16, dtype=F32)
    for s in range(pr.shape[1]):
        q = pr[:, s]
        acc = acc + (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])
    for w in (8, 4, 2, 1):
        acc = acc[:, :w] + acc[:, w:2 * w]
    g = gate.reshape(-1).to(F32)
    v = acc[:, 0] * g if mut == "without_one_minus_g" else acc[:, 0] * g * (1.0 - g)
    dl = torch.full((Pg // k, Eg), 1e-30 if mut == "unselected_unwritten" else 0.0, dtype=F32)
    dl[p // k, ids.reshape(-1)] = v
    return dl


# ---------------------------------------------------------------------------------------------- cases
_CACHE = {}


def _inputs(kernel, family, seed=11):
    key = (kernel, family, seed)
    if key not in _CACHE:
        N, Kd, a_div, x_div = SHAPES[kernel]
        _CACHE[key] = (ref.make_data(family, P, E, N, Kd, a_div, x_div, seed), ref.make_lists(COUNTS, seed=seed))
    return _CACHE[key]


def case(kernel, family, mut=None):
    """[(name, moe_ref kernel key, emulated result, reference dict)] of one kernel on one family."""
    if kernel in ("gate_grad", "expert_sums"):
        return _small_case(kernel, family, mut)
    N, Kd, a_div, x_div = SHAPES[kernel]
    D, lists = _inputs(kernel, family)
    ids, off, perm = lists
    base = kernel.split("_")[0]
    if base in ("nt", "nn"):
        y_div = Y_DIV if kernel.endswith("acc") else 0
        got = emu_grouped(base, D, lists, N, Kd, a_div, kernel.endswith("short"), y_div, mut)
        f = ref.ref_nt if base == "nt" else ref.ref_nn
        R = f(D["A"] if base == "nt" else D["Gm"], Kd if base == "nt" else N, a_div, D["W"],
              D["bias"] if base == "nt" else D["scale"], off, perm, P, E, N, Kd, y_div)
        return [("y", base + ("_acc" if y_div else ""), got, R)]
    rsplit = 2 if kernel == "wgrad_split" else 1
    dw, db = emu_wgrad(D, lists, N, Kd, a_div, x_div, rsplit, mut=mut)
    R = ref.ref_wgrad(D["Gm"], N, a_div, D["X"], Kd, x_div, D["scale"], off, perm, P, E, N, Kd)
    return [("dw", "dw", dw, R), ("db", "db", db, R)]


def _small_case(kernel, family, mut):
    g = torch.Generator().manual_seed(17)
    U, k, Eg, N, fan = 96, 2, 8, 100, 16
    ids = torch.argsort(torch.rand(U, Eg, generator=g), 1)[:, :k].contiguous()
    D = ref.make_data(family, U * k, Eg, N, N, k, k, 19)
    if kernel == "gate_grad":
        gate = D["scale"] if family != "gate_tiny" else 1.0 - D["scale"]
        Y = D["W"].reshape(-1, N)[:U * k].contiguous()
        got = emu_gate_grad(D["A"], Y, ids, gate, U * k, k, Eg, N, k, mut)
        return [("dlogits", "dlogits", got, ref.ref_gate_grad(D["A"], Y, ids, gate, U * k, k, Eg, N, k))]
    G = U * k // fan
    got = emu_expert_sums(D["A"], k, ids.reshape(-1), D["scale"], G, fan, Eg, N, mut)
    return [("z", "z", got, ref.ref_expert_sums(D["A"], N, k, ids.reshape(-1), D["scale"], G, fan, Eg, N))]


KERNELS = {**{k: GEMM_FAMILIES for k in ("nt", "nt_short", "nt_acc", "nn", "nn_short", "nn_acc")},
           "wgrad": ref.DATA_FAMILIES, "wgrad_split": ref.DATA_FAMILIES,
           "gate_grad": ("unit", "outlier_rows", "binade", "gate_tiny"), "expert_sums": ("unit", "outlier_rows", "binade", "gate_tiny")}


@pytest.mark.parametrize("kernel,family", [(k, f) for k, fams in KERNELS.items() for f in fams])
def test_bound_not_too_tight(kernel, family):
    for name, key, got, R in case(kernel, family):
        nbad, ratio, q = ref.measures(got, R, name)
        assert nbad == 0 and ratio <= 0.5, f"{kernel}/{family} {name}: the emulation reaches {ratio:.3f} of the hard bound"
        assert q <= ref.Q_EMU[key], f"{kernel}/{family} {name}: q {q:.3f} above Q_EMU[{key}] = {ref.Q_EMU[key]}"


def test_emulation_defines_q(capsys):
    """Q_EMU is the emulation's worst q per kernel over every family and shape class (and a K 1024 chain), rounded up
    by at most a tenth: the tight tier's measure is this emulation, never the kernel."""
    worst = {}
    for kernel, fams in KERNELS.items():
        for fam in fams:
            for name, key, got, R in case(kernel, fam):
                worst[key] = max(worst.get(key, 0.0), ref.measures(got, R, name)[2])
    # the longest chain of the sweep: Kd 1024 on a handful of rows
    cnt = [5, 0, 3]
    D, lists = ref.make_data("unit", 8, 3, 64, 1024, 1, 1, 5), ref.make_lists(cnt, seed=5)
    for short in (False, True):
        got = emu_grouped("nt", D, lists, 64, 1024, 1, short)
        R = ref.ref_nt(D["A"], 1024, 1, D["W"], D["bias"], lists[1], lists[2], 8, 3, 64, 1024)
        worst["nt"] = max(worst["nt"], ref.measures(got, R, "y")[2])
    with capsys.disabled():
        print("\nemulation worst q:", {k: round(v, 3) for k, v in worst.items()})
    for key, q in worst.items():
        assert q <= ref.Q_EMU[key] <= 1.1 * q + 0.01, f"Q_EMU[{key}] = {ref.Q_EMU[key]} against the emulation's {q:.4f}"


# mutation -> (kernel, families it must be flagged on, tier: "hard" = the hard tier alone flags it)
ALL = GEMM_FAMILIES
MUTATIONS = {
    "row_unwritten": ("nt", ALL, "hard"),
    "k_tail_dropped": ("nt", ALL, "hard"),
    "last_step_dropped": ("nt_acc", ALL, "hard"),
    "bias_of_next_expert": ("nt", ALL, "hard"),
    "weights_of_next_expert_first_tile": ("nt", ALL, "hard"),
    "a_div_ignored": ("nt", ALL, "hard"),
    "half_unit_writes_64": ("nt", ALL, "hard"),
    "odd_rb_last_block_dropped": ("nt", ALL, "hard"),
    "short:last_step_dropped": ("nt_short", ALL, "hard"),
    "nn:scale_of_next_pair": ("nn", ALL, "hard"),
    "nn:row_unwritten": ("nn", ALL, "hard"),
    "nn:last_step_dropped": ("nn_short", ALL, "hard"),
    "acc_missing_pair": ("nt_acc", ALL, "hard"),
    "acc_adds_twice": ("nn_acc", ALL, "hard"),
    "rsplit_loses_pair": ("wgrad_split", ref.DATA_FAMILIES, "hard"),
    "empty_expert_unwritten": ("wgrad", ref.DATA_FAMILIES, "hard"),
    "dbias_without_scale": ("wgrad", ref.DATA_FAMILIES, "hard"),
    "without_one_minus_g": ("gate_grad", KERNELS["gate_grad"], "hard"),
    "unselected_unwritten": ("gate_grad", KERNELS["gate_grad"], "hard"),
    "fan_taken_as_k": ("expert_sums", KERNELS["expert_sums"], "hard"),
    # lost precision: gamma_n grows with n while the truncation error does not, so the hard tier sees operands cut to
    # bf16 up to Kd of about 4096 and to a 10-bit mantissa up to about 1024 (as here); beyond, only the tight tier
    # does (test_lost_precision_needs_the_tight_tier)
    "operands_bf16": ("nt", ALL, "tight"),
    "operands_mant10": ("nt", ALL, "tight"),
    "nn:operands_bf16": ("nn", ALL, "tight"),
}


def _mut(m):
    return m.split(":", 1)[1] if ":" in m else m


def _flags(kernel, family, mut):
    """(flagged by the hard tier alone, flagged by both tiers together)."""
    hard = both = 0
    for name, key, got, R in case(kernel, family, mut):
        hard += ref.violations(got, R, name)
        both += ref.violations(got, R, name, key)
    return hard > 0, both > 0


@pytest.mark.parametrize("mutation,family", [(m, f) for m, (_, fams, _) in MUTATIONS.items() for f in fams])
def test_bound_flags_wrong_results(mutation, family):
    kernel, _, tier = MUTATIONS[mutation]
    assert _flags(kernel, family, None) == (False, False)
    hard, both = _flags(kernel, family, _mut(mutation))
    assert both, f"{mutation} on {family} inputs passes the per-element check"
    if tier == "hard":
        assert hard, f"{mutation} on {family} inputs passes the hard tier"


@pytest.mark.parametrize("mut,K", [("operands_bf16", 8192), ("operands_mant10", 4096)])
def test_lost_precision_needs_the_tight_tier(mut, K):
    """At these depths truncated operands are inside the hard bound of every element; q is 35 to 220 times its limit."""
    D, lists = ref.make_data("unit", 64, 3, 64, K, 1, 1, 5), ref.make_lists([40, 0, 24], seed=5)
    R = ref.ref_nt(D["A"], K, 1, D["W"], D["bias"], lists[1], lists[2], 64, 3, 64, K)
    assert ref.violations(emu_grouped("nt", D, lists, 64, K, 1), R, "y", "nt") == 0
    got = emu_grouped("nt", D, lists, 64, K, 1, mut=mut)
    assert ref.violations(got, R, "y") == 0 and ref.violations(got, R, "y", "nt") == 1
    assert ref.measures(got, R, "y")[2] > 20 * ref.TIGHT_FACTOR * ref.Q_EMU["nt"]


def test_combine_order_is_bitwise_visible():
    """Slot order instead of expert order changes bits (the only check that can see it), and emu_combine in expert
    order equals an fp64 sum to within f32 rounding."""
    g = torch.Generator().manual_seed(2)
    G, outer, k, N, Ec = 64, 3, 4, 32, 16
    ids = torch.argsort(torch.rand(G * outer, Ec, generator=g), 1)[:, :k].contiguous()
    Y, w = torch.randn(G * outer * k, N, generator=g), torch.rand(G * outer * k, generator=g)
    a = ref.emu_combine(Y, ids, w, G, outer, k, N)
    b = ref.emu_combine(Y, ids, w, G, outer, k, N, order="slot")
    assert not torch.equal(a, b)
    want = (w.double().view(-1, 1) * Y.double()).view(G, outer * k, N).sum(1)
    assert float((a.double() - want).abs().max()) < 1e-5
    # the v_div layout: rows per (row group, expert)
    V = torch.randn(G * outer * k // 4 * Ec, N, generator=g)
    c = ref.emu_combine(V, ids, w, G, outer, k, N, v_div=4, E=Ec)
    p = torch.arange(G * outer * k)
    want = (w.double().view(-1, 1) * V.double()[(p // 4) * Ec + ids.reshape(-1)]).view(G, outer * k, N).sum(1)
    assert float((c.double() - want).abs().max()) < 1e-5


def test_routing_references():
    """ref_topk on ties, ref_route and ref_route_distinct against plain loops."""
    lg = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0], [float("-inf")] * 3 + [0.0, float("-inf")]])
    ids, s, _ = ref.ref_topk(lg, 3)
    assert ids.tolist() == [[1, 2, 4], [3, 0, 1]]
    off, perm = ref.ref_route(ids, 5)
    assert off.tolist() == [0, 1, 3, 4, 5, 6] and perm.tolist() == [4, 0, 5, 1, 3, 2]
    off, perm = ref.ref_route_distinct(torch.tensor([0, 2, 2, 1, 1, 1, 0, 2]), 2, 4, 3)
    assert off.tolist() == [0, 2, 4, 6] and perm.tolist() == [0, 3, 1, 4, 2, 5]
    ids, off, perm = ref.make_lists([2, 0, 3], P=9, seed=1)
    assert off.tolist() == [0, 2, 2, 5] and sorted(perm.tolist()) == torch.nonzero(ids >= 0).view(-1).tolist()
    assert all(ids[p] == e for e in range(3) for p in perm[off[e]:off[e + 1]].tolist())
    assert all(perm[off[e]:off[e + 1]].tolist() == sorted(perm[off[e]:off[e + 1]].tolist()) for e in range(3))


# ---------------------------------------------------------------------------------------------- the older criteria
def _old(got, R, name, tol):
    refv = R[name]
    live = ~torch.isnan(refv)
    err = torch.where(live, (got.double() - refv).abs(), torch.zeros_like(refv))
    scale = max(float(refv[live].abs().max()), 1e-6)
    return bool(float(err.max()) <= tol * scale)      # (a NaN error compares false)


def test_old_criteria_report(capsys):
    """Reports, without asserting on the old criteria, which planted faults they pass; asserts that the new check
    passes none on a family where the fault is listed."""
    report = {}
    for m, (kernel, fams, _) in MUTATIONS.items():
        r = {"kernel": kernel, "close_2e-5_passes_on": [], "assert_close_abs_1e-4_passes_on": [], "bound_flags_on": []}
        for fam in KERNELS[kernel]:
            res = case(kernel, fam, _mut(m))
            if all(_old(got, R, name, 2e-5) for name, _, got, R in res):
                r["close_2e-5_passes_on"].append(fam)
            if all(_old(got, R, name, 1e-4) for name, _, got, R in res):
                r["assert_close_abs_1e-4_passes_on"].append(fam)
            if _flags(kernel, fam, _mut(m))[1]:
                r["bound_flags_on"].append(fam)
        assert set(fams) <= set(r["bound_flags_on"]), (m, r)
        report[m] = r
    with capsys.disabled():
        print("\nplanted fault                        kernel       close (2e-5 max) passes on / 1e-4 max passes on / per-element check flags on")
        for m, r in report.items():
            print(f"{m:36s} {r['kernel']:12s} {','.join(r['close_2e-5_passes_on']) or '-'} / "
                  f"{','.join(r['assert_close_abs_1e-4_passes_on']) or '-'} / {','.join(r['bound_flags_on'])}")
    path = os.environ.get("AMK_MOE_OLD_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(report, f, indent=1)


# ---------------------------------------------------------------------------------------------- dispatch restatement
def test_expected_path_table():
    """Every branch of grouped_nt_impl, grouped_nn_impl and amk_grouped_gemm_wgrad at 512 workgroup slots."""
    ep = lambda entry, Pn, En, N, Kd, y_div=0, counts=None, env=(): ref.expected_path(
        entry, Pn, En, N, Kd, y_div, counts if counts is not None else [Pn // En] * En, 512, env)
    table = [
        # nt: wide needs N >= 128 and Kd % 32 == 0
        (ep("nt", 256, 4, 128, 128), "nt_wide m4 full0 tail_split"),               # 4 units whatever m: ties take the taller
        (ep("nt", 256, 4, 128, 128, env=("AMK_MOE_NARROW",)), "nt_narrow<1>"),
        (ep("nt", 256, 4, 128, 128, y_div=2, env=("AMK_MOE_NARROW",)), "nt_wide_acc m4 full0 tail_split"),
        (ep("nt", 256, 4, 128, 100), "nt_narrow<1>"),                               # K tail
        (ep("nt", 256, 4, 124, 128), "nt_narrow<1>"),
        (ep("nt", 256, 4, 64, 256), "nt_narrow<1,short>"),
        (ep("nt", 256, 4, 64, 224), "nt_narrow<1>"),                                # short needs Kd >= 256
        (ep("nt", 256, 4, 68, 256), "nt_narrow<1>"),                                # ... and N <= 64
        (ep("nt", 262081, 4, 64, 256), "nt_narrow<1>"),                             # ... and (P + 63) / 64 < 4096
        (ep("nt", 262080, 4, 64, 256), "nt_narrow<1,short>"),
        # 33280 pairs over 32 experts, 8 column tiles: 1040 blocks; m 4: 2080 units = 4 rounds + 32 (split)
        (ep("nt", 33280, 32, 1024, 64), "nt_wide m4 full1 tail_split"),
        # 16 x 9 blocks, one partial round whatever m: 0.6 blocks + 0.35 is least for the 80 units of m 2 (1.8 blocks)
        (ep("nt", 4608, 16, 128, 128), "nt_wide m2 full0 tail_split"),
        # 300 blocks x 4 column tiles: m 4 300 units, whole, 4.35; m 3 400, whole, 3.35; m 2 600 = 512 + 88: 2.35 + 1.55
        (ep("nt", 9600, 1, 512, 64), "nt_wide m3 full0 tail_whole"),
        # 1536 blocks: m 4 384 units, whole, 4.35; m 3 512 = one full round, 3.35; m 2 768 = 512 + 256: 2.35 + 1.55
        (ep("nt", 49152, 1, 128, 64), "nt_wide m3 full1 tail_none"),
        # 2648 blocks: m 4 662 = 512 + 150 (split): 4.35 + 2.75; m 3 883 = 512 + 371 (whole): 2 x 3.349; m 2 1324: 3 x 2.35
        (ep("nt", 84736, 1, 128, 64), "nt_wide m3 full1 tail_whole"),
        (ep("nt", 65536, 1, 128, 64), "nt_wide m4 full1 tail_none"),                # 2048 blocks / 4 = 512 units
        (ep("nt", 0, 2, 128, 64, counts=[0, 0]), "nt_wide empty"),
        # nn: wide needs Kd >= 128 and N % 32 == 0
        (ep("nn", 256, 4, 128, 128), "nn_wide m4 full0 tail_split"),
        (ep("nn", 256, 4, 100, 128), "nn_narrow<2>"),
        (ep("nn", 256, 4, 128, 68), "nn_narrow<2>"),
        (ep("nn", 256, 4, 128, 64), "nn_narrow<1>"),
        (ep("nn", 256, 4, 256, 64), "nn_narrow<1,short>"),
        (ep("nn", 262081, 4, 256, 64), "nn_narrow<1>"),
        (ep("nn", 256, 4, 256, 128, env=("AMK_MOE_NARROW",)), "nn_narrow<2>"),
        (ep("nn", 256, 4, 256, 128, y_div=4), "nn_wide_acc m4 full0 tail_split"),
        (ep("nn", 33280, 32, 64, 1024), "nn_wide m4 full1 tail_split"),
        # wgrad: wide needs N, Kd >= 64 and N + Kd >= 192
        (ep("wgrad", 256, 4, 64, 64), "wgrad<1>"),
        (ep("wgrad", 256, 4, 60, 256), "wgrad<1>"),
        (ep("wgrad", 256, 4, 128, 64), "wgrad_wide<128,64,scale> rsplit 1"),
        (ep("wgrad_noscale", 256, 4, 64, 128), "wgrad_wide<64,128,noscale> rsplit 1"),
        (ep("wgrad", 1024, 4, 128, 128), "wgrad_wide<128,128,scale> rsplit 2"),
        (ep("wgrad", 1023, 4, 128, 128), "wgrad_wide<128,128,scale> rsplit 1"),    # P / E = 255
        (ep("wgrad", 66000, 8, 1024, 512), "wgrad_wide<128,128,scale> rsplit 2"),  # 256 tiles x 2 = 512 <= 512 ...
        (ep("wgrad", 66000, 8, 1024, 640), "wgrad_wide<128,128,scale> rsplit 1"),  # ... 320 tiles do not
        (ep("wgrad", 1024, 4, 128, 128, env=("AMK_MOE_NARROW",)), "wgrad<1>"),
    ]
    for got, want in table:
        assert got == want, (got, want)
    with pytest.raises(AssertionError):
        ep("nt", 256, 4, 64, 256, y_div=2)


def test_unit_plan_tiles():
    """The tile heights of find_unit_rb: 9 blocks at m 2 are 2 + 2 + 2 + 2 + 1, 1536 blocks at m 3 are 512 tiles of 3."""
    assert ref.unit_plan([288], 1, 512) == (2, 5, 0, 5, True, [2, 2, 2, 2, 1])
    m, units, nfull, r, split, rbs = ref.unit_plan([49152], 1, 512)
    assert (m, units, nfull, r, split, set(rbs)) == (3, 512, 512, 0, False, {3})
    assert ref.unit_plan([0, 0], 4, 512) is None


def test_gpu_sweep_covers_every_path():
    """The case list of tests/test_moe_bounds_gpu.py (imported, not run) reaches every path at 512 slots."""
    import test_moe_bounds_gpu as sweep

    missing = sweep.missing_coverage(512)
    assert not missing, f"the GPU sweep does not reach: {sorted(missing)}"
