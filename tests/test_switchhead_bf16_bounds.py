"""CPU checks of the checker of SwitchHead's bf16 expert kernels (tests/switchhead_bf16_ref.py), no GPU needed.

Not too tight: an f32 emulation of each kernel's chain as read from csrc/moe_bf16.hip -- the grouped products as
tests/test_moe_bf16_bounds.py emulates them (the narrow tile forms run the same chains), the per-expert sums as one
rounded product and one rounded add per pair in ascending order and one rounding to bf16 -- stays inside the hard bound
on every element, over every family and every case of the GPU list, and its worst q defines switchhead_bf16_ref.Q_EMU.
The two Functions restated on the CPU from those emulations stay inside the composed bounds.
Sensitive enough: planted faults produce violations.  The case list reaches every tile edge of the narrow kernels, and
the ctypes bindings carry the documented argument counts."""
import pytest
import torch

import moe_ref as mref
import switchhead_bf16_ref as ref
from test_moe_bf16_bounds import bf16_round, emu_grouped, emu_wgrad

F32 = torch.float32
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------- emulations
def emu_sums(A, lda, a_div, ids, scale, G, fan, E, d, mut=None):
    """expert_sums_bf16_kernel: (G, E d) bf16.  mut: "lost_pair" (the last pair of a row), "partial_sums_bf16" (every
    partial sum rounded to bf16, not the last one alone)."""
    a = A[:, :d].to(F32)
    ids2 = ids.view(G, fan)
    acc = torch.zeros(G, E, d, dtype=F32)
    rows = torch.arange(G)
    for j in range(fan - 1 if mut == "lost_pair" else fan):
        p = rows * fan + j
        w = scale[p].view(-1, 1) if scale is not None else 1.0
        acc[rows, ids2[:, j]] = acc[rows, ids2[:, j]] + w * a[p // a_div]
        if mut == "partial_sums_bf16":
            acc = bf16_round(acc)
    return acc.view(G, E * d).to(BF16)


_CACHE = {}


def _inputs(c, family=None):
    """{"v": data with N = d, Kd = w (nt64, wgrad64), "o": data with N = w, Kd = d (nn64, wgrad64)}, lists, P."""
    family = family or c["family"]
    key = (c["id"], family)
    if key not in _CACHE:
        ids, off, perm, P = ref.case_lists(c)
        d, w = c["d"], c["w"]
        pad = (lambda n, extra: n + extra) if c["pad"] else (lambda n, extra: None)
        Dv = ref.make_data(family, P, c["E"], d, w, c["a_div"], c["x_div"], 8, pad(w, 8), pad(d, 16), pad(w, 24))
        Do = ref.make_data(family, P, c["E"], w, d, c["a_div"], c["x_div"], 9, pad(d, 8), pad(w, 16), pad(d, 24))
        _CACHE[key] = ({"v": Dv, "o": Do}, (ids, off, perm), P)
    return _CACHE[key]


def results(c, family=None, mut=None, kinds=("nt64", "nn64", "wgrad64")):
    """[(name, kernel key, emulated result, reference dict)] of one case."""
    DD, lists, P = _inputs(c, family)
    ids, off, perm = lists
    E, d, w, a_div, x_div = c["E"], c["d"], c["w"], c["a_div"], c["x_div"]
    out = []
    if "nt64" in kinds:
        D = DD["v"]
        out.append(("y", "nt64", emu_grouped("nt", D, lists, d, w, a_div, mut, c["nulls"]),
                    ref.ref_nt(D["A"], D["A"].stride(0), a_div, D["W"], None if c["nulls"] else D["bias"], off, perm, P, E, d, w)))
    if "nn64" in kinds:
        D = DD["o"]
        out.append(("y", "nn64", emu_grouped("nn", D, lists, w, d, a_div, mut, c["nulls"]),
                    ref.ref_nn(D["Gm"], D["Gm"].stride(0), a_div, D["W"], None if c["nulls"] else D["scale"], off, perm, P, E, w, d)))
    if "wgrad64" in kinds:
        use_scale = not c["nulls"]
        for o, (N, Kd) in (("v", (d, w)), ("o", (w, d))):
            D = DD[o]
            dw, _ = emu_wgrad(D, lists, N, Kd, a_div, x_div, use_scale, mut)
            R = ref.ref_wgrad(D["Gm"], D["Gm"].stride(0), a_div, D["X"], D["X"].stride(0), x_div, D["scale"] if use_scale else None,
                              off, perm, P, E, N, Kd)
            out.append(("dw", "dw64", dw, R))
    return out


BY_ID = {c["id"]: c for c in ref.CASES}


def test_emulation_stays_under_every_bound(capsys):
    """Every kernel's emulation on every case of the GPU list and every family; prints the worst ratios."""
    worst = {}
    for c in ref.CASES:
        for fam in ref.DATA_FAMILIES:
            for name, key, got, R in results(c, fam):
                nbad, ratio, q = ref.measures(got, R, name)
                assert nbad == 0, f"{c['id']} / {fam} {key}: the emulation reaches {ratio:.3f} of the hard bound"
                worst[key] = max(worst.get(key, 0.0), ratio)
    for c in ref.SUM_CASES:
        A, ids, scale = ref.sum_inputs(c)
        R = ref.ref_expert_sums(A, A.stride(0), c["a_div"], ids, scale, c["G"], c["fan"], c["E"], c["d"])
        got = emu_sums(A, A.stride(0), c["a_div"], ids, scale, c["G"], c["fan"], c["E"], c["d"])
        nbad, ratio, _ = ref.measures(got, R, "z")
        assert nbad == 0, f"{c['id']}: the emulated sums reach {ratio:.3f} of the bound"
        worst["sums"] = max(worst.get("sums", 0.0), ratio)
    with capsys.disabled():
        print("\nemulation worst |err| / bound:", {k: round(v, 4) for k, v in sorted(worst.items())})


def test_emulation_defines_q(capsys):
    """Q_EMU is the emulation's worst q of nt64 and nn64 over every case and family, rounded up by at most a tenth."""
    worst = {"nt64": 0.0, "nn64": 0.0}
    for c in ref.CASES:
        for fam in ref.DATA_FAMILIES:
            for name, key, got, R in results(c, fam, kinds=("nt64", "nn64")):
                worst[key] = max(worst[key], ref.measures(got, R, name)[2])
    with capsys.disabled():
        print("\nemulation worst q:", {k: round(v, 3) for k, v in worst.items()})
    for key, q in worst.items():
        assert q <= ref.Q_EMU[key] <= 1.1 * q + 0.01, f"Q_EMU[{key}] = {ref.Q_EMU[key]} against the emulation's {q:.4f}"


MUTATIONS = {
    "y_bf16": ("edge_d64_w128", ("nt64", "nn64")),
    "acc_bf16": ("edge_d64_w128", ("nt64", "nn64")),
    "pair_to_wrong_expert": ("edge_d64_w128", ("nt64", "nn64")),
    "bias_dropped": ("holes_d8_w136", ("nt64",)),
    "wgrad_loses_pair": ("holes_d8_w136", ("dw64",)),
}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_bound_flags_wrong_results(mutation):
    cid, keys = MUTATIONS[mutation]
    c = BY_ID[cid]
    flagged = {}
    for name, key, got, R in results(c, mut=mutation):
        flagged[key] = flagged.get(key, 0) + ref.violations(got, R, name, key)
    for key in keys:
        assert flagged[key] > 0, f"{mutation} passes the per-element check of {key}"


@pytest.mark.parametrize("mutation", ["lost_pair", "gate_dropped", "partial_sums_bf16"])
def test_sums_bound_flags_wrong_results(mutation):
    c = ref.SUM_CASES[1]
    A, ids, scale = ref.sum_inputs(c)
    args = [A, A.stride(0), c["a_div"], ids, scale, c["G"], c["fan"], c["E"], c["d"]]
    R = ref.ref_expert_sums(*args)
    assert ref.measures(emu_sums(*args), R, "z")[0] == 0
    if mutation == "gate_dropped":
        args[4] = None
    got = emu_sums(*args, mut=mutation)
    assert ref.measures(got, R, "z")[0] > 0, f"{mutation} passes the per-element check of the sums"


def test_case_list_covers_the_kernels():
    missing = ref.missing_coverage()
    assert not missing, f"the GPU case list does not reach: {sorted(missing)}"
    for c in ref.CASES:
        assert c["d"] <= ref.NARROW and c["d"] % 8 == 0 and c["w"] % 8 == 0


# ---------------------------------------------------------------------------------------------- op level
def _op_case(G, H, k, E, dim, d, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(G, dim), logits=r(G * H, E), Wv=r(E, d, dim) / dim ** 0.5, dv=r(G * H, d),
                a=r(G * H, d), Wo=r(E, dim, d) / d ** 0.5, do=r(G, dim))


def emu_lib_gemm(z16, w16):
    """The library's bf16 GEMM as an f32 product of the bf16 values, rounded to bf16."""
    return (z16.float() @ w16.float()).to(BF16)


@pytest.mark.parametrize("shape", [(33, 4, 2, 4, 64, 16), (21, 4, 3, 5, 72, 8)])
def test_op_references_compose(shape):
    """ref_shared_row / ref_summed on a CPU restatement of the two Functions stay inside the composed bounds, and a
    planted fault (out left unrounded is fine; Z summed without its gate is not) leaves them."""
    G, H, k, E, dim, d = shape
    T = _op_case(G, H, k, E, dim, d, 3)
    U_, fan = G * H, H * k
    ids, s, _ = mref.ref_topk(T["logits"], k)
    gate = s.float()
    off, perm = mref.ref_route_distinct(ids, G, fan, E)
    idv = torch.full((G * E,), -1, dtype=torch.int64)
    idv[perm.long()] = perm.long() % E
    lists = (idv, off, perm)
    rows = ref._rows_of(ids, H, E)
    # V experts
    x16, wv16 = bf16_round(T["x"]), bf16_round(T["Wv"])
    Dv = {"A": x16, "W": wv16, "X": x16}
    V = emu_grouped("nt", Dv, lists, d, dim, E, nulls=True)
    out = mref.emu_combine(V, ids, gate, U_, 1, k, d, v_div=H * k, E=E)
    f = gate * (1 - gate)
    dl = torch.zeros(U_, E)
    dl[torch.arange(U_).view(-1, 1).expand(U_, k), ids] = (T["dv"].view(U_, 1, d) * V[rows]).sum(2) * f
    Z16 = emu_sums(T["dv"], d, k, ids.reshape(-1), gate.reshape(-1), G, fan, E, d)
    dx = emu_lib_gemm(Z16, wv16.reshape(E * d, dim))
    Dv["Gm"] = Z16.float().view(G * E, d)
    dw, _ = emu_wgrad(Dv, lists, d, dim, 1, E, use_scale=False)
    R = ref.ref_shared_row(T["x"], T["logits"], T["Wv"], T["dv"], ids, gate, k, H)
    for name, got in (("out", out), ("dx", dx), ("dlogits", dl), ("dw", dw)):
        ref.assert_bounded(got, R, name, "cpu restatement, V experts")
    with pytest.raises(AssertionError):
        Zbad = emu_sums(T["dv"], d, k, ids.reshape(-1), None, G, fan, E, d)
        ref.assert_bounded(emu_lib_gemm(Zbad, wv16.reshape(E * d, dim)), R, "dx", "planted: the gate left out of Z")
    # output experts
    wo16, d16 = bf16_round(T["Wo"]), bf16_round(T["do"])
    Zo = emu_sums(T["a"], d, k, ids.reshape(-1), None, G, fan, E, d)
    out_o = emu_lib_gemm(Zo, wo16.permute(0, 2, 1).reshape(E * d, dim))
    Do = {"Gm": d16, "W": wo16, "X": Zo.float().view(G * E, d)}
    D = emu_grouped("nn", Do, lists, dim, d, E, nulls=True)
    da = mref.emu_combine(D, ids, None, U_, 1, k, d, v_div=H * k, E=E)
    dwo, _ = emu_wgrad(Do, lists, dim, d, E, 1, use_scale=False)
    Ro = ref.ref_summed(T["a"], T["logits"], T["Wo"], T["do"], ids, k, H)
    for name, got in (("out", out_o), ("da", da), ("dw", dwo)):
        ref.assert_bounded(got, Ro, name, "cpu restatement, output experts")
    with pytest.raises(AssertionError):
        ref.assert_bounded(bf16_round(da), Ro, "da", "planted: da rounded to bf16")


def test_op_shapes_take_the_distinct_form():
    from amk import ops

    for G, H, k, E, dim, d in ref.OP_SHAPES:
        assert ops.distinct_experts_ok(dim, d, H * k, E) and d <= ref.NARROW and d % 8 == 0 and dim % 8 == 0


def test_attention_backward_bound_holds_for_an_f32_core():
    """attention_backward's bounds hold for an f32 attention backward (autograd on the CPU) reading q, k exactly and v,
    d_o perturbed by up to their bounds; a dq row with the wrong sign leaves them."""
    g = torch.Generator().manual_seed(4)
    B, h, T, D, scale = 2, 3, 65, 64, 0.125
    q, k = (bf16_round(torch.randn(B, h, T, D, generator=g) * 0.6) for _ in range(2))     # the projections' size in the model
    v, do = torch.randn(B, h, T, D, generator=g), torch.randn(B, h, T, D, generator=g)
    Bv, Bdo = v.abs() * 2.0 ** -12 + 1e-6, do.abs() * 2.0 ** -10 + 1e-6
    R = ref.attention_backward(q, k, v, Bv, do, Bdo, scale)
    sg = lambda t: torch.where(torch.rand(t.shape, generator=g) < 0.5, -1.0, 1.0)
    q32, k32 = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    v32 = (v.double() + sg(v) * Bv.double()).float()
    o = torch.softmax(scale * (q32 @ k32.transpose(-1, -2)), -1) @ v32
    o.backward((do.double() + sg(do) * Bdo.double()).float())
    ref.assert_bounded(q32.grad, R, "dq", "cpu f32 attention")
    ref.assert_bounded(k32.grad, R, "dk", "cpu f32 attention")
    bad = q32.grad.clone()
    bad[0, 0, 3] = -bad[0, 0, 3]
    with pytest.raises(AssertionError):
        ref.assert_bounded(bad, R, "dq", "planted: one dq row with the wrong sign")
    # sensitive enough behind the projection too: the same row through the bf16 rounding and the library's weight gradient
    x16 = bf16_round(torch.randn(B * T, 32, generator=g))
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B * T, h * D)
    r, b = rows(R["dq"]), rows(R["bound_dq"])
    wr, wb = ref.lib_wgrad(r, b + ref.U * (r.abs() + b), x16)
    Rw = {"w": wr, "bound_w": wb}
    ref.assert_bounded(bf16_round(bf16_round(rows(q32.grad)).t() @ x16), Rw, "w", "cpu projection")
    with pytest.raises(AssertionError):
        ref.assert_bounded(bf16_round(bf16_round(rows(bad)).t() @ x16), Rw, "w", "planted: the same row, behind the projection")


def test_bindings_have_the_documented_argument_counts():
    from amk import lib

    want = {"amk_grouped_gemm_nt64_bf16": 13, "amk_grouped_gemm_nn64_bf16": 13, "amk_grouped_gemm_wgrad64_bf16": 15,
            "amk_moe_expert_sums_bf16": 12}
    declared = set(lib.declared_symbols())
    for name, n in want.items():
        assert name in declared, f"{name} is not declared in include/amk.h"
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n, name
    L = lib.load()
    for name in want:
        assert hasattr(L, name), f"libamk.so does not export {name}"
    from amk import ops
    assert isinstance(ops.SWITCHHEAD_BF16, bool)
