"""csrc/vq.hip held to tests/vq_ref.py through the raw C ABI, so that the number of codebook slices can be forced:
every (C, K, nsplit) of vq_ref.CASES -- full and partial LDS tiles, the non-pipelined branch with several slices, slices
made of padding only, 16 slices and the finalize loop beyond 16 (20, 24, 32), K = 1 -- on the gaussian, clustered, scaled
and tiny_norm families at N = 1 .. 257: the index inside the licence on every row and equal to the fp64 argmax where the
margin exceeds tau; zn, zq, out and the mean squared error inside per-element bounds at the kernel's own index.  Planted
winners (every code position wins once) and planted exact ties (the first copy must win) with no licence at all.  Bitwise:
the outputs do not depend on nsplit, on the order of the rows or on the number of rows.  The backward (atomics and the
per-row form summed as ops sums it) and the gather against their bounds.  Workspaces are poisoned with NaN, results sit
between guard rows of 3e38.

AMK_VQ_BOUND_REPORT=<file>: write the worst |got - ref| / bound per output over this module to that JSON file."""
import ctypes
import json
import os

import pytest
import torch

import vq_ref as ref

pytestmark = pytest.mark.gpu
POISON = 3e38
GUARD = 4
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    worst = {k: v for k, v in ref.WORST.items() if k.startswith("vq.")}
    print("worst |got - ref| / bound:", {k: round(v, 4) for k, v in sorted(worst.items())})
    path = os.environ.get("AMK_VQ_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(worst, f, indent=1, sort_keys=True)


def _P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _L():
    from amk import lib

    return lib.load()


def _chk(rc, what):
    from amk import lib

    lib.check(rc, what)


class Canvas:
    """(rows, cols) result region inside a buffer of 3e38 with GUARD rows before and after it."""

    def __init__(self, rows, cols, device, dtype=torch.float32, fill=POISON):
        self.full = torch.full((rows + 2 * GUARD, cols), fill, device=device, dtype=dtype)
        self.view = self.full[GUARD:GUARD + rows]
        self.fill = self.full[0, 0].clone()

    def check(self, what):
        assert bool((self.full[:GUARD] == self.fill).all() and (self.full[-GUARD:] == self.fill).all()), \
            f"{what}: wrote outside its result region"
        assert bool((self.view != self.fill).all()), f"{what}: result region not fully written"


def _fwd(device, z, E, nsplit):
    """amk_vq_lookup_fwd on NaN workspaces -> {idx, zn, zq, out, partial, mean_sq} (device tensors)."""
    L = _L()
    N, C = z.shape
    K = E.shape[0]
    kp = L.amk_vq_padded_codes(K, nsplit)
    assert kp == ref.padded_codes(K, nsplit)
    zd, Ed = z.to(device), E.to(device)
    en = torch.full((kp, C), NAN, device=device)
    ee = torch.full((kp,), NAN, device=device)
    pmin = torch.full((N, nsplit), NAN, device=device)
    pidx = torch.full((N, nsplit), -2 ** 31 + 5, device=device, dtype=torch.int32)
    c = {n: Canvas(N, C, device) for n in ("out", "zq", "zn")}
    c["idx"] = Canvas(N, 1, device, torch.int64, -7)
    c["partial"] = Canvas(ref.num_partials(N), 1, device)
    assert L.amk_vq_num_partials(N) == ref.num_partials(N)
    _chk(L.amk_vq_lookup_fwd(_P(zd), _P(Ed), N, K, C, nsplit, _P(en), _P(ee), _P(pmin), _P(pidx), _P(c["idx"].view),
                             _P(c["out"].view), _P(c["zq"].view), _P(c["zn"].view), _P(c["partial"].view), _S()), "amk_vq_lookup_fwd")
    torch.cuda.synchronize()
    for n, cv in c.items():
        cv.check(f"vq fwd {n}")
    got = {n: cv.view for n, cv in c.items()}
    got["idx"] = got["idx"][:, 0]
    got["partial"] = got["partial"][:, 0]
    got["mean_sq"] = (got["partial"].sum() / float(N * C)).view(1)      # as ops._VQLookup.forward
    return got


def _within(got, R, names, what, key):
    return ref.assert_within(got, R, names, what, key="vq." + key)


_IDS = [f"C{C}-K{K}-s{ns}" for C, K, ns in ref.ALL_CASES]


@pytest.mark.parametrize("C,K,ns", ref.ALL_CASES, ids=_IDS)
def test_fwd_licence_and_bounds(device, C, K, ns):
    licensed = 0
    for fam in ref.FAMILIES:
        for N in ref.NS:
            z, E = ref.make_fwd(fam, N, K, C, 100 + N + K)
            got = _fwd(device, z, E, ns)
            what = f"vq fwd {fam} N{N} K{K} C{C} nsplit{ns}"
            R = ref.ref_scores(z, E)
            nd, _ = ref.check_indices(R, got["idx"], what)
            licensed += nd
            _within(got, ref.ref_outputs(R, got["idx"].cpu()), ref.FWD_OUT, what, "fwd")
    print(f"C{C} K{K} nsplit{ns}: {licensed} rows differ from the fp64 argmax inside the licence")


@pytest.mark.parametrize("C,K,ns", ref.ALL_CASES, ids=_IDS)
def test_planted_winners(device, C, K, ns):
    z, E, target = ref.make_planted(C, K, 7 + K)
    got = _fwd(device, z, E, ns)
    assert torch.equal(got["idx"].cpu(), target), (got["idx"].cpu() != target).nonzero().view(-1)[:8]


@pytest.mark.parametrize("C,K,ns", [c for c in ref.ALL_CASES if c[1] > 1], ids=[i for i, c in zip(_IDS, ref.ALL_CASES) if c[1] > 1])
def test_planted_ties(device, C, K, ns):
    z, E, want, kinds = ref.make_ties(C, K, ns, 11 + K)
    got = _fwd(device, z, E, ns)["idx"].cpu()
    wrong = [(kinds[r], int(want[r]), int(got[r])) for r in range(len(want)) if int(got[r]) != int(want[r])]
    assert not wrong, f"(kind, expected first copy, got): {wrong}"


@pytest.mark.parametrize("C", ref.CS)
def test_bitwise_invariances(device, C):
    K, N = 1000, 257
    zc, E = ref.make_fwd("clustered", N, K, C, 3)
    zt, Et, want, _ = ref.make_ties(C, K, 4, 5)
    names = ("idx", "zn", "zq", "out", "partial")
    for what, z, Ex in (("clustered", zc, E), ("ties", zt, Et)):
        base = _fwd(device, z, Ex, 1)
        for ns in ref.NSPLITS_INVARIANT[1:]:
            got = _fwd(device, z, Ex, ns)
            for n in names:
                assert torch.equal(base[n], got[n]), f"{what} {n}: nsplit {ns} differs from nsplit 1"
    # rows permuted -> outputs permuted; a row alone -> the same row
    base = _fwd(device, zc, E, 4)
    perm = torch.randperm(N, generator=ref._gen(1))
    got = _fwd(device, zc[perm], E, 4)
    for n in ("idx", "zn", "zq", "out"):
        assert torch.equal(base[n][perm.to(device)], got[n]), f"{n}: permuting the rows changes them"
    for r in (0, 130, 256):
        one = _fwd(device, zc[r:r + 1], E, 4)
        for n in ("idx", "zn", "zq", "out"):
            assert torch.equal(base[n][r:r + 1], one[n]), f"{n}: row {r} alone differs"


# ---------------------------------------------------------------------------------------------- backward
def _ordered_sum(ge, idx, K):
    """The codebook gradient from per-row contributions, as ops._VQLookup.backward sums them."""
    srt, order = torch.sort(idx.clamp(0, K - 1), stable=True)
    bounds = torch.searchsorted(srt, torch.arange(K + 1, device=srt.device, dtype=srt.dtype))
    return torch.segment_reduce(ge.index_select(0, order), "sum", offsets=bounds, axis=0, unsafe=True)


def _gather(device, idx, E, count_bad=True):
    L = _L()
    N, (K, C) = idx.numel(), E.shape
    out = Canvas(N, C, device)
    bad = torch.zeros(1, device=device, dtype=torch.int32)
    idx_d, E_d = idx.to(device), E.to(device)            # (held until the synchronize below)
    _chk(L.amk_vq_gather(_P(idx_d), _P(E_d), N, K, C, _P(out.view), _P(bad) if count_bad else _P(None), _S()),
         "amk_vq_gather")
    torch.cuda.synchronize()
    out.check("vq gather")
    return out.view, int(bad.item())


def _bwd(device, z, E, idx, go, gl, beta, zn, zq, rows):
    L = _L()
    N, C = z.shape
    K = E.shape[0]
    dz = Canvas(N, C, device)
    last = Canvas(N if rows else K, C, device)
    fn = L.amk_vq_lookup_bwd_rows if rows else L.amk_vq_lookup_bwd
    _chk(fn(_P(z), _P(E), _P(zn), _P(zq), _P(idx), _P(go), _P(gl), beta, N, K, C, _P(dz.view), _P(last.view), _S()), "vq bwd")
    torch.cuda.synchronize()
    dz.check("vq bwd dz")
    last.check("vq bwd " + ("ge_rows" if rows else "dE"))
    return dz.view, last.view


@pytest.mark.parametrize("C", ref.CS)
@pytest.mark.parametrize("N,K", ref.BWD_NK, ids=lambda v: str(v))
def test_bwd_bounds(device, C, N, K):
    for i, mode in enumerate(ref.BWD_MODES):
        beta = ref.BETAS[(i + N) % 3]
        z, E, idx, go, gl = ref.make_bwd(mode, N, K, C, 50 + N + K + i)
        what = f"vq bwd {mode} N{N} K{K} C{C} beta{beta}"
        R = ref.ref_bwd(z, E, idx, go, gl, beta)
        zd, Ed, id_, god, gld = (t.to(device) for t in (z, E, idx, go, gl.view(1)))
        zn = _fwd(device, z, E, 1)["zn"].contiguous()                # the forward's own f32 zn ...
        zq, nbad = _gather(device, idx, E)                           # ... and zq = l2norm(E[idx]) at the given index
        assert nbad == 0
        zq = zq.contiguous()
        _within({"zn": zn, "zq": zq}, {"zn": R["zn"], "zq": R["zq"], **_fwd_bounds(R, C)}, ("zn", "zq"), what, "bwd_in")
        dz, dE = _bwd(device, zd, Ed, id_, god, gld, beta, zn, zq, rows=False)
        dz2, ge = _bwd(device, zd, Ed, id_, god, gld, beta, zn, zq, rows=True)
        assert torch.equal(dz, dz2)
        dE2 = _ordered_sum(ge, id_, K)
        _within({"dz": dz, "ge": ge, "dE": dE}, R, ("dz", "ge", "dE"), what, "bwd")
        _within({"dE": dE2}, R, ("dE",), what + " ordered", "bwd")
        unused = (R["count"] == 0).to(device)
        assert bool((dE[unused] == 0).all() and (dE2[unused] == 0).all()), "a code no row chose has a gradient"
        dz3, ge3 = _bwd(device, zd, Ed, id_, god, gld, beta, zn, zq, rows=True)
        assert torch.equal(dz2, dz3) and torch.equal(ge, ge3) and torch.equal(dE2, _ordered_sum(ge3, id_, K)), \
            "the ordered path is not bitwise repeatable"
        if mode == "g_loss0":
            assert bool((ge == 0).all()) and bool((dE == 0).all())


def _fwd_bounds(R, C):
    L = ref._l(C)
    return {"bound_zn": ((C / 16 + 3.5) * ref.U32 + ref.U32) * R["zn"].abs(),
            "bound_zq": ((3 + L / 2) * ref.U32 + ref.U32) * R["zq"].abs()}


@pytest.mark.parametrize("C", ref.CS)
def test_gather(device, C):
    K, N = 77, 300
    g = ref._gen(C)
    E = torch.randn(K, C, generator=g)
    E[5] = 0.0
    E[6] *= 1e-14 / C ** 0.5
    idx = torch.randint(0, K, (N,), generator=g)
    idx[:7] = torch.arange(7)
    got, nbad = _gather(device, idx, E)
    assert nbad == 0
    _within({"gather": got}, ref.ref_gather(idx, E), ("gather",), f"vq gather C{C}", "gather")
    # indices outside the codebook are counted and clamped, never dereferenced
    wild = idx.clone()
    wild[10], wild[11], wild[12], wild[13] = -1, K, 2 ** 40, -2 ** 62
    got, nbad = _gather(device, wild, E)
    assert nbad == 4
    _within({"gather": got}, ref.ref_gather(wild.clamp(0, K - 1), E), ("gather",), f"vq gather C{C} clamped", "gather")
    got2, _ = _gather(device, wild, E, count_bad=False)
    assert torch.equal(got, got2)
