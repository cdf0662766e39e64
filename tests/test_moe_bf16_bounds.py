"""CPU checks of the checker of the bf16 grouped expert GEMMs (tests/moe_bf16_ref.py), no GPU needed.

Not too tight: an f32 emulation of each kernel's chain as read from csrc/moe_bf16.hip -- on the bf16-valued inputs one
product and one rounded add per contraction step in order, the bias / scale after the chain; the weight gradient with
scale x G rounded to bf16 first, then one product and add per pair of the expert, dbias the sum of those rounded values --
stays inside the hard bound on every element, over every family and every shape of the GPU case list, and its worst q
defines moe_bf16_ref.Q_EMU (asserted here).
Sensitive enough: the planted faults of MUTATIONS produce violations.  The case list reaches every edge and branch of
the kernels (moe_bf16_ref.required_features)."""
import pytest
import torch

import moe_bf16_ref as ref

F32 = torch.float32


def bf16_round(x):
    return x.to(torch.bfloat16).to(F32)


# ---------------------------------------------------------------------------------------------- emulations
def emu_grouped(kind, D, lists, N, Kd, a_div, mut=None, nulls=False):
    """The rows of the named pairs through grouped_{nt,nn}_bf16: (P, out) f32, rows not named NaN."""
    ids, off, perm = lists
    E, P = off.numel() - 1, ids.numel()
    pp, ee, cnt = ref.named_pairs(off, perm, E)
    win, wout = (Kd, N) if kind == "nt" else (N, Kd)
    src = D["A"] if kind == "nt" else D["Gm"]
    a = src[pp // a_div, :win].to(F32)
    W = D["W"].to(F32)
    Wk = (W.permute(2, 0, 1) if kind == "nt" else W.permute(1, 0, 2)).contiguous()      # (win, E, wout)
    we = ee.clone()
    if mut == "pair_to_wrong_expert":
        we[0] = (we[0] + 1) % E
    acc = torch.zeros(pp.numel(), wout, dtype=F32)
    for k in range(win):
        acc = acc + a[:, k:k + 1] * Wk[k][we]          # (the product of two bf16 values is exact in f32)
        if mut == "acc_bf16":
            acc = bf16_round(acc)
    if kind == "nt":
        y = acc if (nulls or mut == "bias_dropped") else acc + D["bias"][ee]
    else:
        y = acc if nulls else acc * D["scale"][pp].view(-1, 1)
    if mut == "y_bf16":
        y = bf16_round(y)
    out = torch.full((P, wout), float("nan"), dtype=F32)
    out[pp] = y
    return out


def emu_wgrad(D, lists, N, Kd, g_div, x_div, use_scale=True, mut=None):
    ids, off, perm = lists
    E = off.numel() - 1
    o = off.long().tolist()
    dw, db = torch.zeros(E, N, Kd, dtype=F32), torch.zeros(E, N, dtype=F32)
    for e in range(E):
        rows = perm[o[e]:o[e + 1]].long()
        if mut == "wgrad_loses_pair" and rows.numel() > 1:
            rows = rows[:-1]
        if rows.numel() == 0:
            continue
        g = D["Gm"][rows // g_div, :N].to(F32)
        gs = bf16_round(g * D["scale"][rows].view(-1, 1)) if use_scale else g
        x = D["X"][rows // x_div, :Kd].to(F32)
        acc, bs = torch.zeros(N, Kd, dtype=F32), torch.zeros(N, dtype=F32)
        for i in range(rows.numel()):
            acc = acc + gs[i].view(-1, 1) * x[i].view(1, -1)
            bs = bs + (g[i] if mut == "dbias_without_scale" else gs[i])
        dw[e], db[e] = acc, bs
    return dw, db


# ---------------------------------------------------------------------------------------------- cases
_CACHE = {}


def _inputs(c, family=None):
    family = family or c["family"]
    key = (c["id"], family)
    if key not in _CACHE:
        counts, P = ref.case_counts(c)
        lists = ref.make_lists(counts, P=P, seed=7)
        pad = (lambda w, extra: w + extra) if c["pad"] else (lambda w, extra: None)
        D = ref.make_data(family, P, c["E"], c["N"], c["Kd"], c["a_div"], c["x_div"], 8, pad(c["Kd"], 8), pad(c["N"], 16), pad(c["Kd"], 24))
        _CACHE[key] = (D, lists, P)
    return _CACHE[key]


def results(c, family=None, mut=None, kinds=("nt", "nn", "wgrad")):
    """[(name, kernel key, emulated result, reference dict)] of one case."""
    D, lists, P = _inputs(c, family)
    ids, off, perm = lists
    E, N, Kd, a_div, x_div = c["E"], c["N"], c["Kd"], c["a_div"], c["x_div"]
    out = []
    if "nt" in kinds:
        bias = None if c["nulls"] else D["bias"]
        out.append(("y", "nt", emu_grouped("nt", D, lists, N, Kd, a_div, mut, c["nulls"]),
                    ref.ref_nt(D["A"], D["A"].stride(0), a_div, D["W"], bias, off, perm, P, E, N, Kd)))
    if "nn" in kinds:
        scale = None if c["nulls"] else D["scale"]
        out.append(("y", "nn", emu_grouped("nn", D, lists, N, Kd, a_div, mut, c["nulls"]),
                    ref.ref_nn(D["Gm"], D["Gm"].stride(0), a_div, D["W"], scale, off, perm, P, E, N, Kd)))
    if "wgrad" in kinds:
        use_scale = not c["nulls"]
        dw, db = emu_wgrad(D, lists, N, Kd, a_div, x_div, use_scale, mut)
        R = ref.ref_wgrad(D["Gm"], D["Gm"].stride(0), a_div, D["X"], D["X"].stride(0), x_div, D["scale"] if use_scale else None,
                          off, perm, P, E, N, Kd)
        out += [("dw", "dw", dw, R), ("db", "db", db, R)]
    return out


BY_ID = {c["id"]: c for c in ref.CASES}


@pytest.mark.parametrize("c", ref.CASES, ids=lambda c: c["id"])
def test_bound_not_too_tight(c):
    """The emulation of every kernel is inside the hard bound on every element of every case of the GPU list."""
    for name, key, got, R in results(c):
        nbad, ratio, q = ref.measures(got, R, name)
        assert nbad == 0 and ratio <= 1.0, f"{c['id']} {key}: the emulation reaches {ratio:.3f} of the hard bound"


@pytest.mark.parametrize("family", ref.DATA_FAMILIES)
def test_bound_not_too_tight_every_family(family):
    """... and on every family at every shape of the list."""
    for c in ref.CASES:
        for name, key, got, R in results(c, family):
            nbad, ratio, q = ref.measures(got, R, name)
            assert nbad == 0, f"{c['id']} / {family} {key}: the emulation reaches {ratio:.3f} of the hard bound"


def test_emulation_defines_q(capsys):
    """Q_EMU is the emulation's worst q of nt and nn over every case of the GPU list and every family, rounded up by at
    most a tenth: the tight tier's measure is this emulation, never the kernel."""
    worst = {"nt": 0.0, "nn": 0.0}
    for c in ref.CASES:
        for fam in ref.DATA_FAMILIES:
            for name, key, got, R in results(c, fam, kinds=("nt", "nn")):
                worst[key] = max(worst[key], ref.measures(got, R, name)[2])
    with capsys.disabled():
        print("\nemulation worst q:", {k: round(v, 3) for k, v in worst.items()})
    for key, q in worst.items():
        assert q <= ref.Q_EMU[key] <= 1.1 * q + 0.01, f"Q_EMU[{key}] = {ref.Q_EMU[key]} against the emulation's {q:.4f}"


# mutation -> (case id, kernel keys that must flag it)
MUTATIONS = {
    "y_bf16": ("edge_136x128", ("nt", "nn")),
    "acc_bf16": ("edge_136x128", ("nt", "nn")),
    "pair_to_wrong_expert": ("edge_136x128", ("nt", "nn")),
    "bias_dropped": ("holes_64x72", ("nt",)),
    "wgrad_loses_pair": ("holes_64x72", ("dw", "db")),
    "dbias_without_scale": ("holes_64x72", ("db",)),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_bound_flags_wrong_results(mutation):
    cid, keys = MUTATIONS[mutation]
    c = BY_ID[cid]
    clean = {key: ref.violations(got, R, name, key) for name, key, got, R in results(c)}
    assert all(v == 0 for v in clean.values()), clean
    flagged = {key: ref.violations(got, R, name, key) for name, key, got, R in results(c, mut=mutation)}
    for key in keys:
        assert flagged[key] > 0, f"{mutation} passes the per-element check of {key}"


def test_y_bf16_at_depth_1024_needs_the_tight_tier():
    """At Kd 1024 a Y rounded to bf16 can hide inside gamma_n S where the sum cancels little; q is far above its limit."""
    c = BY_ID["strides_1024"]
    (name, key, got, R), = results(c, mut="y_bf16", kinds=("nt",))
    assert ref.violations(got, R, name, key) > 0
    assert ref.measures(got, R, name)[2] > 20 * ref.TIGHT_FACTOR * ref.Q_EMU["nt"]


def test_case_list_covers_the_kernels():
    missing = ref.missing_coverage()
    assert not missing, f"the GPU case list does not reach: {sorted(missing)}"


def test_op_reference_composes():
    """ref_op on a CPU restatement of the op (f32 emulation of the three products, moe_ref.emu_combine, the f32 gate
    gradient) stays inside the composed bounds."""
    import moe_ref as mref

    g = torch.Generator().manual_seed(3)
    U_, D_, E, k = 97, 40, 5, 3
    x, W, bias = torch.randn(U_, D_, generator=g), torch.randn(E, D_, D_, generator=g) / 6, torch.randn(E, D_, generator=g)
    logits, d_out = torch.randn(U_, E, generator=g), torch.randn(U_, D_, generator=g)
    ids, s, _ = mref.ref_topk(logits, k)
    off, perm = mref.ref_route(ids, E)
    route = dict(ids=ids, gate=s.float(), offsets=off, perm=perm)
    R = ref.ref_op(x, logits, W, bias, d_out, route, k)
    D = {"A": bf16_round(x), "W": bf16_round(W), "bias": bias, "Gm": bf16_round(d_out), "X": bf16_round(x), "scale": route["gate"].reshape(-1)}
    lists = (ids.reshape(-1), off, perm)
    Y = emu_grouped("nt", D, lists, D_, D_, k)
    out = mref.emu_combine(Y, ids, route["gate"], U_, 1, k, D_)
    dxp = emu_grouped("nn", D, lists, D_, D_, k)
    dx = mref.emu_combine(dxp, ids, None, U_, 1, k, D_)
    gt = route["gate"].reshape(-1)
    dl = torch.zeros(U_, E)
    dl[torch.arange(U_ * k) // k, ids.reshape(-1)] = (d_out[torch.arange(U_ * k) // k] * Y).sum(1) * gt * (1 - gt)
    dw, db = emu_wgrad(D, lists, D_, D_, k, k)
    for name, got in (("out", out), ("dx", dx), ("dlogits", dl), ("dw", dw), ("db", db)):
        ref.assert_bounded(got, R, name, "cpu restatement")
    with pytest.raises(AssertionError):
        ref.assert_bounded(bf16_round(out), R, "out", "planted: out rounded to bf16")
