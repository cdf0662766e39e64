"""The MoE routing kernels and grouped expert GEMMs of csrc/moe.hip on the MI355X, called through the C ABI and held
element by element to the two tiers of tests/moe_ref.py (the hard f32 bound and 4 x the CPU emulation's q) against
vectorised fp64 references, over the input families, routing families and the shapes at the edges of the host dispatch.

Every output is written into a NaN canvas (the accumulating forms: a canvas of known values) with guard rows before
and after: the guards and the rows the lists do not name must be untouched.  No element is left out of a check.
The non-atomic forms and the weight gradient (rsplit 2 adds two halves into zero: order-free) must repeat bit for
bit.  A pair's row of grouped_nt / _nn is a chain over k that depends on the expert and the output tile (the wide
kernels start their walk over K at (e ncol + ct) % nk) but not on the pair's position in the expert, on every
non-atomic path (narrow, short: the two k-halves are fixed sets; wide: whatever the tile height): test_position_free.
test_paths_cover_dispatch proves with the device's CU count that the case list reaches every path of the host code.
AMK_MOE_BOUNDS_REPORT=<file>: the worst hard ratio and q / limit per kernel as JSON."""
import ctypes
import json
import os

import pytest
import torch

import moe_ref as ref

pytestmark = pytest.mark.gpu

EDGE = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 257]          # per-expert counts at the tile edges
HOLES = [0, 1, 31, 0, 33, 65, 0, 0, 97, 129, 164, 0]                         # empty experts first, in the middle, last


def _uniform(P, E):
    return [P // E + (1 if e < P % E else 0) for e in range(E)]


def _rand_counts(P, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.bincount(torch.randint(0, E, (P,), generator=g), minlength=E).tolist()


def C(id, family, route, E, N, Kd, a_div=1, x_div=1, pad=False, nulls=False, narrow=False, entries=("nt", "nn", "wgrad")):
    return dict(id=id, family=family, route=route, E=E, N=N, Kd=Kd, a_div=a_div, x_div=x_div, pad=pad, nulls=nulls,
                narrow=narrow, entries=entries)


# route: ("counts", counts) | ("sparse", counts, P) | ("ops", units, k, skew) | ("distinct", groups, units per group, k)
CASES = [
    C("edge_wide", "unit", ("counts", EDGE), 14, 128, 128, 2, 2),
    C("holes_short", "expert_scale", ("counts", HOLES), 12, 64, 256, 16, 2),
    C("split_64x256", "expert_scale", ("counts", _uniform(1500, 4)), 4, 64, 256, 2, 2),
    C("split_128", "binade", ("counts", [300, 260, 256, 208]), 4, 128, 128, 2, 2),
    C("skew_256x64", "cancel", ("counts", ref.skewed_counts(5000, 16)), 16, 256, 64, 1, 1),
    C("one_takes_all", "gate_tiny", ("counts", [0, 0, 777, 0]), 4, 256, 256, 3, 3),
    C("div3", "outlier_rows", ("counts", _rand_counts(192, 5, 1)), 5, 256, 256, 3, 3),
    C("ktail", "unit", ("counts", HOLES), 12, 128, 100, 2, 2),
    C("ktail_scale", "expert_scale", ("counts", EDGE), 14, 64, 36, 2, 16),
    C("n132_k36", "binade", ("counts", HOLES), 12, 132, 36, 1, 1),
    C("n20_k160", "cancel", ("counts", EDGE), 14, 20, 160, 2, 2),
    C("n4_k4", "unit", ("counts", HOLES), 12, 4, 4, 1, 1),
    C("n60_k96", "expert_scale", ("counts", HOLES), 12, 60, 96, 3, 1),
    C("n68_k64", "outlier_rows", ("counts", EDGE), 14, 68, 64, 2, 2),
    C("e70", "expert_scale", ("counts", _rand_counts(194, 70, 2)), 70, 128, 256, 2, 2),
    C("e200", "binade", ("counts", _rand_counts(900, 200, 3)), 200, 192, 160, 2, 2),
    C("strides_wide", "outlier_rows", ("counts", EDGE), 14, 128, 128, 2, 2, pad=True, nulls=True),
    C("strides_narrow", "gate_tiny", ("counts", HOLES), 12, 64, 100, 2, 2, pad=True, nulls=True),
    C("strides_n1024", "unit", ("counts", _rand_counts(300, 6, 4)), 6, 1024, 1024, 16, 2, pad=True),
    C("narrow_env", "cancel", ("counts", EDGE), 14, 256, 128, 2, 2, narrow=True),
    C("narrow_env_split", "expert_scale", ("counts", _uniform(1500, 4)), 4, 128, 128, 2, 2, narrow=True),
    C("sparse_wide", "expert_scale", ("sparse", [40, 0, 100, 33, 127], 520), 5, 128, 128, 2, 2),
    C("sparse_narrow", "binade", ("sparse", [40, 0, 100, 33, 127], 520), 5, 64, 36, 1, 1),
    C("ops_skewed", "unit", ("ops", 2500, 2, True), 16, 128, 64, 2, 2),
    C("distinct_v", "expert_scale", ("distinct", 130, 8, 2), 32, 64, 256, 32, 32),
    C("distinct_out", "unit", ("distinct", 130, 8, 2), 32, 256, 64, 32, 1),
    # more units than workgroup slots: the ViTMoE SwitchHead layer and its transpose; a whole (unsplit) last round
    C("switchhead_out", "expert_scale", ("counts", _uniform(33280, 32)), 32, 1024, 64, 1, 1),
    C("switchhead_v", "unit", ("counts", _uniform(33280, 32)), 32, 64, 1024, 16, 2),
    C("rounds_whole_nt", "unit", ("counts", [84736]), 1, 128, 64, 16, 16, entries=("nt",)),
    C("rounds_whole_nn", "unit", ("counts", [84736]), 1, 64, 128, 16, 16, entries=("nn",)),
    C("rounds_none", "expert_scale", ("counts", [49152, 0]), 2, 128, 64, 16, 16, entries=("nt",)),
    # past the size limit of the short rule ((P + 63) / 64 >= 8 x slots)
    C("long_narrow_nt", "expert_scale", ("counts", _uniform(262144, 8)), 8, 64, 256, 16, 16, entries=("nt",)),
    C("long_narrow_nn", "unit", ("counts", _uniform(262144, 8)), 8, 256, 64, 16, 16, entries=("nn",)),
]
Y_DIVS = (2, 8)


def _case_counts(c):
    """Per-expert counts and P of a case without a GPU (ops / distinct routes: uniform counts of the same total, which
    decide no path of these cases)."""
    r = c["route"]
    if r[0] == "counts":
        return r[1], sum(r[1])
    if r[0] == "sparse":
        return r[1], r[2]
    if r[0] == "ops":
        return _uniform(r[1] * r[2], c["E"]), r[1] * r[2]
    G, E = r[1], c["E"]
    return _uniform(G * 13, E), G * E


def case_paths(c, slots, counts=None, P=None):
    """{path or feature name} that the case reaches."""
    if counts is None:
        counts, P = _case_counts(c)
    E, N, Kd = c["E"], c["N"], c["Kd"]
    env = ("AMK_MOE_NARROW",) if c["narrow"] else ()
    out = set()
    for entry in c["entries"]:
        if entry == "wgrad":
            out.add(ref.expected_path("wgrad", P, E, N, Kd, 0, counts, slots, env))
            out.add(ref.expected_path("wgrad_noscale", P, E, N, Kd, 0, counts, slots, env))
            continue
        wout, win, ok_acc = (N, Kd, N >= 128 and Kd % 32 == 0) if entry == "nt" else (Kd, N, Kd >= 128 and N % 32 == 0)
        name = ref.expected_path(entry, P, E, N, Kd, 0, counts, slots, env)
        out.add(name)
        if ok_acc:
            out.add(ref.expected_path(entry, P, E, N, Kd, Y_DIVS[0], counts, slots, env).split(" ")[0])
        if "_wide" in name and "empty" not in name:
            head, m, full, tail = name.split(" ")
            m_, units, nfull, r, split, rbs = ref.unit_plan(counts, (wout + 127) // 128, slots)
            out |= {f"{head} {m}", f"{head} {tail}", f"{head} {full} {tail}"}
            if split:
                out |= {f"{head} half rb{rb}" for rb in rbs[nfull:]}
            if wout % 128:
                out.add(f"{head} partial column tile")
        else:
            if win % 32:
                out.add(f"{name} k tail")
            if wout > 64 * (2 if name == "nn_narrow<2>" else 1):
                out.add(f"{name} ncol > 1")
            if wout < 64:
                out.add(f"{name} out < 64")
            if wout % 64 and wout > 64:
                out.add(f"{name} out ends inside a tile")
            if (P + 63) // 64 >= 8 * slots:
                out.add(f"{name} past the short limit")
    out.add(f"a_div {'E' if c['a_div'] == E and E > 16 else c['a_div']}")
    out.add(f"family {c['family']}")
    if E > 64:
        out.add("E > 64")
    if E > 128:
        out.add("E > 128")
    for flag in ("pad", "nulls"):
        if c[flag]:
            out.add(flag)
    out.add("route " + c["route"][0])
    return out


def required_paths():
    req = set(ref.NT_PATHS + ref.NN_PATHS + ref.WGRAD_PATHS + ["nt_wide_acc", "nn_wide_acc"])
    for head in ("nt_wide", "nn_wide"):
        req |= {f"{head} m{m}" for m in (2, 3, 4)} | {f"{head} tail_{t}" for t in ("split", "whole")}
        req |= {f"{head} full1 tail_split", f"{head} full1 tail_whole", f"{head} half rb1", f"{head} half rb3",
                f"{head} half rb2", f"{head} half rb4", f"{head} partial column tile"}
    req |= {"nt_wide tail_none", "nt_narrow<1> k tail", "nt_narrow<1> ncol > 1", "nt_narrow<1> out < 64",
            "nt_narrow<1> out ends inside a tile", "nt_narrow<1> past the short limit", "nn_narrow<1> past the short limit",
            "nn_narrow<2> k tail", "nn_narrow<1> k tail", "nn_narrow<1> out < 64", "nn_narrow<2> ncol > 1", "E > 64", "E > 128",
            "pad", "nulls", "route counts", "route sparse", "route ops", "route distinct"}
    req |= {f"a_div {d}" for d in (1, 2, 3, 16, "E")} | {f"family {f}" for f in ref.DATA_FAMILIES}
    return req


def missing_coverage(slots, resolved=None):
    seen = set()
    for c in CASES:
        seen |= case_paths(c, slots, *(resolved or {}).get(c["id"], (None, None)))
    return required_paths() - seen


# ---------------------------------------------------------------------------------------------- helpers
GUARD = 3


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def canvas(rows, width, dev, init=None, dtype=torch.float32, fill=float("nan")):
    """(whole, inner): `rows` rows between GUARD guard rows, everything `fill` (inner: init, if given)."""
    whole = torch.full((rows + 2 * GUARD, width), fill, device=dev, dtype=dtype)
    inner = whole[GUARD:GUARD + rows]
    if init is not None:
        inner.copy_(init)
    return whole, inner


def guards_untouched(whole, rows, fill=None):
    g = torch.cat([whole[:GUARD], whole[GUARD + rows:]])
    return bool(torch.isnan(g).all()) if fill is None else bool((g == fill).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _lists(c, dev, seed):
    """(offsets, perm, P) on the device."""
    from amk import ops

    r = c["route"]
    if r[0] in ("counts", "sparse"):
        ids, off, perm = ref.make_lists(r[1], P=r[2] if r[0] == "sparse" else None, seed=seed)
        return off.to(dev), perm.to(dev), ids.numel()
    g = torch.Generator().manual_seed(seed)
    if r[0] == "ops":
        lg = torch.randn(r[1], c["E"], generator=g) + (torch.linspace(-7.0, 3.0, c["E"]) if r[3] else 0.0)
        rt = ops.moe_route(lg.to(dev), r[2])
        ids_ref, _, _ = ref.ref_topk(lg.to(dev), r[2])
        off_ref, perm_ref = ref.ref_route(ids_ref, c["E"])
        assert torch.equal(rt["offsets"], off_ref) and torch.equal(rt["perm"], perm_ref)
        return rt["offsets"], rt["perm"], r[1] * r[2]
    G, upg, k = r[1:]
    ids, _ = ops._topk(torch.randn(G * upg, c["E"], generator=g).to(dev), k)
    off, perm = ops._route_distinct(ids, G, upg * k, c["E"])
    off_ref, perm_ref = ref.ref_route_distinct(ids, G, upg * k, c["E"])
    L = int(off_ref[-1])
    assert torch.equal(off, off_ref) and torch.equal(perm[:L], perm_ref)
    return off, perm, G * c["E"]


def _run_grouped(L, kind, c, D, off, perm, P, y_div, y0, set_env):
    """One launch of grouped_nt / _nn (y_div > 0: the accumulating form): (whole canvas, inner view, reference)."""
    from amk import lib as L_

    E, N, Kd, a_div = c["E"], c["N"], c["Kd"], c["a_div"]
    src = D["A"] if kind == "nt" else D["Gm"]
    vec = None if c["nulls"] else (D["bias"] if kind == "nt" else D["scale"])
    wout = N if kind == "nt" else Kd
    rows = P if y_div == 0 else (P - 1) // y_div + 1
    whole, inner = canvas(rows, wout, src.device, y0)
    fn = getattr(L, f"amk_grouped_gemm_{kind}" + ("_acc" if y_div else ""))
    args = [_ptr(src), src.stride(0), a_div, _ptr(D["W"]), _ptr(vec), _ptr(off), _ptr(perm), P, E, N, Kd, _ptr(inner)]
    with set_env(c["narrow"]):
        L_.check(fn(*args, *((y_div,) if y_div else ()), _stream()), fn.__name__ if hasattr(fn, "__name__") else kind)
    R = (ref.ref_nt if kind == "nt" else ref.ref_nn)(src, src.stride(0), a_div, D["W"], vec, off, perm, P, E, N, Kd, y_div, y0)
    return whole, inner, R


@pytest.fixture
def set_env(monkeypatch):
    import contextlib

    @contextlib.contextmanager
    def ctx(narrow):
        with monkeypatch.context() as m:
            if narrow:
                m.setenv("AMK_MOE_NARROW", "1")      # read per call by the host code
            else:
                m.delenv("AMK_MOE_NARROW", raising=False)
            yield
    return ctx


def _slots():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------- the sweep
def test_paths_cover_dispatch(device):
    """With this device's CU count the case list reaches every path of the host dispatch (a card with another CU
    count fails here, loudly, and is not tested thinner in silence)."""
    missing = missing_coverage(_slots())
    assert not missing, f"at {_slots()} workgroup slots the sweep does not reach: {sorted(missing)}"


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_grouped_gemms(device, c, set_env):
    from amk import lib as L_

    L = L_.load()
    dev = device
    E, N, Kd, a_div, x_div = c["E"], c["N"], c["Kd"], c["a_div"], c["x_div"]
    off, perm, P = _lists(c, dev, seed=7)
    pad = (lambda w, extra: w + extra) if c["pad"] else (lambda w, extra: None)
    D = {k: v.to(dev) for k, v in ref.make_data(c["family"], P, E, N, Kd, a_div, x_div, 8, pad(Kd, 12), pad(N, 8), pad(Kd, 4)).items()}
    counts = (off[1:] - off[:-1]).tolist()
    what = lambda s: f"{c['id']} {s} [{ref.expected_path(*s_args(s))}]"

    def s_args(s):
        entry = s.split("_")[0] if not s.startswith("wgrad") else s
        return entry, P, E, N, Kd, (Y_DIVS[0] if s.endswith("acc") else 0), counts, _slots(), ("AMK_MOE_NARROW",) if c["narrow"] else ()

    for kind in ("nt", "nn"):
        if kind not in c["entries"]:
            continue
        whole, Y, R = _run_grouped(L, kind, c, D, off, perm, P, 0, None, set_env)
        ref.assert_within(Y, R, "y", kind, what(kind))
        assert guards_untouched(whole, P), f"{what(kind)}: a guard row was written"
        assert bool(torch.isnan(Y[~R["named_y"]]).all()), f"{what(kind)}: a row the lists do not name was written"
        _, Y2, _ = _run_grouped(L, kind, c, D, off, perm, P, 0, None, set_env)
        assert same_bits(Y, Y2), f"{what(kind)}: two calls differ"
        wide_ok = (N >= 128 and Kd % 32 == 0) if kind == "nt" else (Kd >= 128 and N % 32 == 0)
        for y_div in Y_DIVS if wide_ok else ():
            rows = (P - 1) // y_div + 1
            y0 = torch.randn(rows, Y.shape[1], generator=torch.Generator().manual_seed(y_div)).to(dev)
            whole, Ya, R = _run_grouped(L, kind, c, D, off, perm, P, y_div, y0, set_env)
            ref.assert_within(Ya, R, "y", kind + "_acc", what(kind + "_acc") + f" y_div {y_div}")
            assert guards_untouched(whole, rows), f"{what(kind + '_acc')}: a guard row was written"
            assert same_bits(Ya[~R["named_y"]], y0[~R["named_y"]]), f"{what(kind + '_acc')}: a row without pairs changed"
    if "wgrad" not in c["entries"]:
        return
    for use_scale in (True, False):
        name = "wgrad" if use_scale else "wgrad_noscale"
        scale = D["scale"] if use_scale else None
        want_db = not (c["nulls"] and use_scale)
        outs = []
        for rep in range(2):
            wW, dW = canvas(E * N, Kd, dev)
            wb, db = canvas(E, N, dev)
            with set_env(c["narrow"]):
                L_.check(L.amk_grouped_gemm_wgrad(_ptr(D["Gm"]), D["Gm"].stride(0), a_div, _ptr(D["X"]), D["X"].stride(0), x_div,
                                                  _ptr(scale), _ptr(off), _ptr(perm), P, E, N, Kd, _ptr(dW),
                                                  _ptr(db) if want_db else None, _stream()), "amk_grouped_gemm_wgrad")
            outs.append((dW, db))
            assert guards_untouched(wW, E * N) and guards_untouched(wb, E), f"{what(name)}: a guard row was written"
        R = ref.ref_wgrad(D["Gm"], D["Gm"].stride(0), a_div, D["X"], D["X"].stride(0), x_div, scale, off, perm, P, E, N, Kd)
        dW, db = outs[0]
        ref.assert_within(dW.view(E, N, Kd), R, "dw", "dw", what(name))
        empty = torch.tensor(counts, device=dev) == 0
        assert bool((dW.view(E, N, Kd)[empty] == 0).all()), f"{what(name)}: an expert without pairs is not exactly zero"
        assert same_bits(dW, outs[1][0]), f"{what(name)}: two calls differ in dW"
        if want_db:
            ref.assert_within(db, R, "db", "db", what(name))
            assert bool((db[empty] == 0).all()) and same_bits(db, outs[1][1]), f"{what(name)}: dbias of an empty expert / two calls"
        else:
            assert bool(torch.isnan(db).all()), f"{what(name)}: dbias written although null was passed"


@pytest.mark.parametrize("shape", [(128, 128, False), (64, 256, False), (64, 100, False), (256, 64, False), (256, 128, True)],
                         ids=lambda s: "N{}K{}{}".format(s[0], s[1], "narrow" if s[2] else ""))
def test_position_free(device, shape, set_env):
    """The rows of the pairs that two lists share (same expert, another position, another tile plan) are equal bit
    for bit: wide, narrow <1>, <1, short>, <2>."""
    from amk import lib as L_

    L = L_.load()
    N, Kd, narrow = shape
    ids, off, perm = ref.make_lists(EDGE, seed=5)
    P, E = ids.numel(), len(EDGE)
    keep = torch.rand(P, generator=torch.Generator().manual_seed(6)) < 0.7
    cnt2 = torch.bincount(ids[keep], minlength=E)
    off2 = torch.zeros(E + 1, dtype=torch.int32)
    off2[1:] = torch.cumsum(cnt2, 0)
    rows = torch.nonzero(keep).view(-1)
    perm2 = rows[torch.sort(ids[rows], stable=True)[1]].int()
    c = C("pos", "unit", None, E, N, Kd, 2, 2, narrow=narrow)
    D = {k: v.to(device) for k, v in ref.make_data("binade", P, E, N, Kd, 2, 2, 9).items()}
    for kind in ("nt", "nn"):
        _, Y1, _ = _run_grouped(L, kind, c, D, off.to(device), perm.to(device), P, 0, None, set_env)
        _, Y2, R2 = _run_grouped(L, kind, c, D, off2.to(device), perm2.to(device), P, 0, None, set_env)
        assert torch.equal(R2["named_y"].cpu(), keep)
        assert same_bits(Y1[keep.to(device)], Y2[keep.to(device)]), f"{kind} N{N} K{Kd}: a row depends on its position"


# ---------------------------------------------------------------------------------------------- routing
def _tie_logits(name, g):
    q = lambda U, E: torch.round(torch.randn(U, E, generator=g) * 2) / 2          # few distinct values: ties everywhere
    if name == "ties_E33_k2":
        return q(257, 33), 2
    if name == "ties_E64_k8":
        return q(129, 64), 8
    if name == "ties_E40_k6":                                                      # route_topk_kernel<6>, <7>: launch_topk's
        return q(129, 40), 6                                                       # switch over k, csrc/moe.hip:1369-1378
    if name == "ties_E33_k7":
        return q(131, 33), 7
    if name == "boundary_31_32":
        lg = q(130, 96)
        lg[:, 31] = lg[:, 32] = lg[:, 63] = lg[:, 64] = 9.0                        # ties across the staging chunks
        return lg, 3
    if name == "kth_tie":
        lg = torch.randn(200, 40, generator=g)
        lg[:, 7] = lg[:, 29] = lg[:, 35] = lg.max(1)[0] - 0.25                     # the k-th and (k + 1)-th value equal
        return lg, 2
    if name == "all_equal":
        return torch.zeros(129, 70), 4
    if name == "neg_inf":
        lg = q(300, 40)
        lg[torch.rand(300, 40, generator=g) < 0.9] = float("-inf")                 # often fewer than k finite values
        lg[:5] = float("-inf")
        return lg, 5
    if name == "k_eq_E":
        lg = q(129, 4)
        lg[0] = torch.tensor([80.0, -80.0, 0.0, float("-inf")])
        lg[1] = torch.tensor([-80.0, -87.0, 88.0, -60.0])
        return lg, 4
    if name == "E1":
        return torch.randn(257, 1, generator=g), 1
    if name == "E1024_k8":
        lg = q(129, 1024)
        lg[:, 1023] = lg[:, 0] = 7.0
        return lg, 8
    raise ValueError(name)


@pytest.mark.parametrize("name", ["ties_E33_k2", "ties_E64_k8", "boundary_31_32", "kth_tie", "all_equal", "neg_inf", "k_eq_E",
                                  "E1", "E1024_k8", "ties_E40_k6", "ties_E33_k7"])
def test_topk_and_route(device, name):
    """ids against a stable descending sort (lowest index first on ties), the gate under its bound, offsets and perm
    exact; every output and workspace between guards."""
    from amk import lib as L_

    L = L_.load()
    lg, k = _tie_logits(name, torch.Generator().manual_seed(3))
    lg = lg.to(device).contiguous()
    U, E = lg.shape
    ids_ref, s, bound = ref.ref_topk(lg, k)
    wi, ids = canvas(U, k, device, dtype=torch.int64, fill=-7)
    wg, gate = canvas(U, k, device)
    L_.check(L.amk_moe_topk(_ptr(lg), U, E, k, _ptr(ids), _ptr(gate), _stream()), "amk_moe_topk")
    assert torch.equal(ids, ids_ref), f"{name}: ids differ from the stable descending order"
    err = (gate.double() - s).abs()
    assert bool((err <= bound).all()), f"{name}: gate off by {float((err / bound).max()):.3g}x its bound"
    assert guards_untouched(wi, U, -7) and guards_untouched(wg, U)
    # the whole route: the same selection, then offsets / perm
    nws = int(L.amk_moe_route_ws_ints(U, E, k))
    wi, ids2 = canvas(U, k, device, dtype=torch.int64, fill=-7)
    wg, gate2 = canvas(U, k, device)
    ints = {n: canvas(r, 1, device, dtype=torch.int32, fill=-7) for n, r in
            (("counts", E), ("rank", U * k), ("blockhist", nws), ("offsets", E + 1), ("perm", U * k))}
    L_.check(L.amk_moe_route(_ptr(lg), U, E, k, _ptr(ids2), _ptr(gate2), *(_ptr(ints[n][1]) for n in ("counts", "rank", "blockhist", "offsets", "perm")),
                             _stream()), "amk_moe_route")
    assert torch.equal(ids2, ids_ref) and same_bits(gate2, gate)
    off_ref, perm_ref = ref.ref_route(ids_ref, E)
    assert torch.equal(ints["offsets"][1].view(-1), off_ref) and torch.equal(ints["perm"][1].view(-1), perm_ref)
    assert torch.equal(ints["counts"][1].view(-1), off_ref[1:] - off_ref[:-1])
    for n, (whole, inner) in ints.items():
        assert guards_untouched(whole, inner.shape[0], -7), f"{name}: a guard of {n} was written"
    assert guards_untouched(wi, U, -7) and guards_untouched(wg, U)


@pytest.mark.parametrize("G,fan,E", [(130, 16, 32), (1025, 2, 64), (7, 300, 5), (3, 4096, 64), (300, 1, 1)])
def test_route_distinct(device, G, fan, E):
    from amk import lib as L_

    L = L_.load()
    ids = torch.randint(0, E, (G * fan,), generator=torch.Generator().manual_seed(4)).to(device)
    off_ref, perm_ref = ref.ref_route_distinct(ids, G, fan, E)
    n = G * min(fan, E)
    wm, mask = canvas(G, 1, device, dtype=torch.int64, fill=-7)
    wo, off = canvas(E + 1, 1, device, dtype=torch.int32, fill=-7)
    wp, perm = canvas(n, 1, device, dtype=torch.int32, fill=-7)
    L_.check(L.amk_moe_route_distinct(_ptr(ids), G, fan, E, _ptr(mask), _ptr(off), _ptr(perm), _stream()), "amk_moe_route_distinct")
    Ln = int(off_ref[-1])
    assert torch.equal(off.view(-1), off_ref) and torch.equal(perm.view(-1)[:Ln], perm_ref)
    assert bool((perm.view(-1)[Ln:] == -7).all()), "entries past offsets[E] were written"
    assert guards_untouched(wm, G, -7) and guards_untouched(wo, E + 1, -7) and guards_untouched(wp, n, -7)


@pytest.mark.parametrize("rows_layout", [False, True], ids=["pairs", "rows"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("outer", [1, 3, 8])
def test_combine_bitwise(device, outer, k, weighted, rows_layout):
    """combine_kernel equals the f32 emulation in its own order bit for bit (w y and every sum rounded separately,
    ascending expert id, then over `outer`)."""
    from amk import lib as L_

    L = L_.load()
    g = torch.Generator().manual_seed(11)
    G, N, E, v_div = 67, 36, 16, (4 * k if rows_layout else 0)
    Pn = G * outer * k
    ids = torch.argsort(torch.rand(G * outer, E, generator=g), 1)[:, :k].contiguous()
    Y = torch.randn(((Pn - 1) // v_div + 1) * E if v_div else Pn, N, generator=g) * torch.exp2(torch.randint(-8, 9, (1, N), generator=g).float())
    w = torch.rand(Pn, generator=g) if weighted else None
    want = ref.emu_combine(Y, ids, w, G, outer, k, N, v_div, E)
    whole, out = canvas(G, N, device)
    dv = lambda t: None if t is None else t.to(device)
    Yd, idsd, wd = dv(Y), dv(ids), dv(w)
    if rows_layout:
        rc = L.amk_moe_combine_rows(_ptr(Yd), _ptr(idsd), _ptr(wd), G, outer, k, N, v_div, E, _ptr(out), _stream())
    else:
        rc = L.amk_moe_combine(_ptr(Yd), _ptr(idsd), _ptr(wd), G, outer, k, N, _ptr(out), _stream())
    L_.check(rc, "amk_moe_combine")
    assert same_bits(out.cpu(), want), f"combine differs from its f32 emulation by {float((out.cpu() - want).abs().max()):.3g}"
    assert guards_untouched(whole, G)


@pytest.mark.parametrize("family", ["unit", "outlier_rows", "binade", "gate_tiny"])
@pytest.mark.parametrize("U,k,E,N,g_div,rows_layout", [(300, 2, 8, 64, 2, False), (129, 8, 33, 100, 1, False), (65, 1, 1, 4, 1, False),
                                                       (130, 2, 32, 1024, 16, False), (128, 2, 32, 64, 2, True)])
def test_gate_grad(device, family, U, k, E, N, g_div, rows_layout):
    from amk import lib as L_

    L = L_.load()
    g = torch.Generator().manual_seed(13)
    Pn = U * k
    ids = torch.argsort(torch.rand(U, E, generator=g), 1)[:, :k].contiguous().to(device)
    v_div = 16 if rows_layout else 0
    ny = ((Pn - 1) // v_div + 1) * E if v_div else Pn                # rows of Y: per (row group, expert) or per pair
    D = ref.make_data(family, max(Pn, ny), 1, N, N, g_div, 1, 14)
    d_out, gate, Y = D["A"].to(device), D["scale"][:Pn].contiguous().to(device), D["X"][:ny].contiguous().to(device)
    if family == "gate_tiny":
        gate = 1.0 - gate                                          # 1 - g then cancels
    whole, dl = canvas(U, E, device)
    if rows_layout:
        rc = L.amk_moe_gate_grad_rows(_ptr(d_out), _ptr(Y), _ptr(ids), _ptr(gate), Pn, k, E, N, g_div, v_div, _ptr(dl), _stream())
    else:
        rc = L.amk_moe_gate_grad(_ptr(d_out), _ptr(Y), _ptr(ids), _ptr(gate), Pn, k, E, N, g_div, _ptr(dl), _stream())
    L_.check(rc, "amk_moe_gate_grad")
    R = ref.ref_gate_grad(d_out, Y, ids, gate, Pn, k, E, N, g_div, v_div)
    assert bool(torch.isfinite(dl).all()), "an entry of dlogits was left unwritten"
    ref.assert_within(dl, R, "dlogits", "dlogits", f"gate_grad {family} U{U} k{k} E{E} N{N}")
    assert bool((dl[R["S_dlogits"] == 0] == 0).all()), "an entry no slot selected (or with a zero product) is not exactly zero"
    assert guards_untouched(whole, U)


@pytest.mark.parametrize("family", ["unit", "binade", "gate_tiny"])
@pytest.mark.parametrize("G,fan,E,d,a_div,scaled", [(3, 1, 1, 8, 1, True), (130, 16, 32, 64, 2, True), (5, 300, 4096, 4, 1, True),
                                                    (2, 4096, 32, 20, 2, False), (40, 16, 4096, 4, 16, True)])
def test_expert_sums(device, family, G, fan, E, d, a_div, scaled):
    from amk import lib as L_

    L = L_.load()
    Pn = G * fan
    ids = torch.randint(0, E, (Pn,), generator=torch.Generator().manual_seed(15)).to(device)
    D = ref.make_data(family, Pn, 1, 4, d, a_div, 1, 16, lda=d + 8)
    A, scale = D["A"].to(device), (D["scale"].to(device) if scaled else None)
    whole, Z = canvas(G, E * d, device)
    L_.check(L.amk_moe_expert_sums(_ptr(A), A.stride(0), a_div, _ptr(ids), _ptr(scale), G, fan, E, d, _ptr(Z), _stream()), "amk_moe_expert_sums")
    R = ref.ref_expert_sums(A, A.stride(0), a_div, ids, scale, G, fan, E, d)
    ref.assert_within(Z, R, "z", "z", f"expert_sums {family} G{G} fan{fan} E{E} d{d}")
    assert bool((Z[R["S_z"] == 0] == 0).all()) and guards_untouched(whole, G)


def test_zz_report(device, capsys):
    """Prints the worst figures of the run (last in the file); AMK_MOE_BOUNDS_REPORT=<file>: also as JSON."""
    with capsys.disabled():
        print("\nkernel: worst hard ratio, worst q / limit")
        for key, (ratio, q) in sorted(ref.WORST.items()):
            print(f"  {key:8s} {ratio:.4f}  {q:.4f}")
    path = os.environ.get("AMK_MOE_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(ref.WORST, f, indent=1)
