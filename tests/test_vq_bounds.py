"""tests/vq_ref.py without a GPU: the share of rows inside the index licence stays under its cap on every family and
case the GPU tests run (from the fp64 reference alone); the planted winners and ties are what the module says they are;
an f32 forward and backward on the CPU (torch's summation order) stay inside the licence and the bounds; the analytic
fp64 backward equals fp64 autograd; defects planted in the specification land outside; the C ABI's refusals."""
import ctypes

import pytest
import torch

import vq_ref as ref

F64 = torch.float64
CK = sorted({(C, K) for C, K, _ in ref.ALL_CASES})


@pytest.mark.parametrize("C,K", CK, ids=lambda v: str(v))
def test_licensed_share_and_f32_forward(C, K):
    worst_share = 0.0
    for fam in ref.FAMILIES:
        licensed = 0
        for N in ref.NS:
            z, E = ref.make_fwd(fam, N, K, C, 100 + N + K)
            R = ref.ref_scores(z, E)
            tau, margin = ref.tau_row(R)
            licensed += int((margin <= tau).sum())
            em = ref.emulate_fwd(z, E)
            ref.check_indices(R, em["idx"], f"f32 forward {fam} N{N}")
            Ro = ref.ref_outputs(R, em["idx"])
            ref.assert_within(em, Ro, ref.FWD_OUT, f"f32 forward {fam} N{N}", key="vq_cpu")
            for n in ref.FWD_OUT:
                assert bool(torch.isfinite(Ro["bound_" + n]).all())
        # the cap: over the rows of the case (every N of the list: 690 rows), zero rows and all
        share = licensed / sum(ref.NS)
        worst_share = max(worst_share, share)
        assert share <= ref.MAX_LICENSED, (fam, share)
    print(f"C{C} K{K}: worst licensed share {worst_share:.4f}")


@pytest.mark.parametrize("C", ref.CS)
def test_planted_winners_have_a_wide_margin(C):
    for K, ns in ref.CASES[C]:
        z, E, target = ref.make_planted(C, K, 7 + K)
        R = ref.ref_scores(z, E)
        assert torch.equal(R["argmax"], target)
        tau, margin = ref.tau_row(R)
        assert bool((margin > 1000 * tau).all()), (K, float(margin.min()), float(tau.max()))
        # every position of the sweep is a target once
        pos = {ref.position(C, K, ns, k) for k in range(K)}
        assert len(pos) == K


@pytest.mark.parametrize("C", ref.CS)
def test_planted_ties(C):
    seen = set()
    for K, ns in ref.CASES[C]:
        made = ref.make_ties(C, K, ns, 11 + K)
        if made is None:
            assert K < 2
            continue
        z, E, want, kinds = made
        seen |= set(kinds)
        R = ref.ref_scores(z, E)
        n = torch.arange(len(want))
        # the copies are the same f32 row, so every arithmetic scores them alike; the fp64 matrix product itself may
        # differ in the last bit between two columns, hence 1e-12.  They sit behind the expected index.
        ties = (R["score"] - R["score"].max(1, keepdim=True).values).abs() < 1e-12
        assert bool(ties[n, want].all())
        for r in range(len(want)):
            for j in ties[r].nonzero().view(-1).tolist():
                assert torch.equal(E[j], E[int(want[r])])
        assert bool((ties.sum(1) >= 2).all())
        last = ties.shape[1] - 1 - ties.flip(1).to(torch.uint8).argmax(1)
        assert bool((last > want).all())
        for r, kind in enumerate(kinds):
            copies = ties[r].nonzero().view(-1).tolist()
            assert len(copies) == (3 if kind == "three" else 2), (kind, copies)
            if kind != "three":
                got = ref._tie_kind(ref.position(C, K, ns, copies[0]), ref.position(C, K, ns, copies[1]))
                assert got == kind
    need = set(ref.TIE_KINDS) - ({"subtiles"} if ref.CODES_LDS[C] == 32 else set())
    assert seen >= need, need - seen


def test_defects_land_outside():
    C, K, N = 32, 416, 129
    z, E = ref.make_fwd("clustered", N, K, C, 5)
    R = ref.ref_scores(z, E)
    # the second best code everywhere: rows with a margin above tau are caught
    with pytest.raises(AssertionError):
        ref.check_indices(R, R["top"].indices[:, 1], "second best")
    # the last of equal maxima instead of the first
    zt, Et, want, _ = ref.make_ties(C, K, 1, 3)
    Rt = ref.ref_scores(zt, Et)
    last = K - 1 - ((Rt["score"] - Rt["score"].max(1, keepdim=True).values).abs() < 1e-12).flip(1).to(torch.uint8).argmax(1)
    assert not torch.equal(last, want)
    # a relative error of a few u32 more than the roundings the source holds (mean_sq: d = zq - zn cancels to 1e-2 on
    # this family, so its roundings weigh 1e-4 of it)
    em = ref.emulate_fwd(z, E)
    Ro = ref.ref_outputs(R, em["idx"])
    for name, f in (("zn", 1 + 2e-6), ("zq", 1 - 2e-6), ("out", 1 + 2e-6), ("mean_sq", 1 + 1e-3)):
        bad = dict(em)
        bad[name] = em[name] * f
        q = ref.ratios(bad, Ro, (name,))
        assert q[name][0] > 0, name


@pytest.mark.parametrize("C", ref.CS)
def test_backward_reference_and_f32_backward(C):
    for N, K in ref.BWD_NK:
        for i, mode in enumerate(ref.BWD_MODES):
            beta = ref.BETAS[(i + N) % 3]
            z, E, idx, go, gl = ref.make_bwd(mode, N, K, C, 50 + N + K + i)
            R = ref.ref_bwd(z, E, idx, go, gl, beta)
            dz, dE = ref.autograd_bwd(z, E, idx, go, gl, beta)
            ok_r = torch.isfinite(dz).all(1)
            ok_c = torch.isfinite(dE).all(1)
            assert int((~ok_r).sum()) <= 1 and int((~ok_c).sum()) <= 1        # (only the exact zeros)
            assert bool(((dz - R["dz"]).abs()[ok_r] <= 1e-12 * R["scale_dz"][ok_r]).all())
            assert bool(((dE - R["dE"]).abs()[ok_c] <= 1e-12 * R["scale_dE"][ok_c]).all())
            assert bool((R["dE"][R["count"] == 0] == 0).all())
            em = ref.emulate_bwd(z, E, idx, go, gl, beta)
            ref.assert_within(em, R, ("dz", "ge", "dE"), f"f32 backward {mode} N{N} K{K} C{C}", key="vq_cpu")
            for n in ("dz", "ge", "dE"):
                assert bool(torch.isfinite(R["bound_" + n]).all())
            if mode == "random" and N >= 129:
                bad = dict(em)
                bad["dz"] = em["dz"] * (1 + 4e-6)
                assert ref.ratios(bad, R, ("dz",))["dz"][0] > 0


def test_gather_reference():
    for C in ref.CS:
        E = torch.randn(40, C, generator=ref._gen(C))
        idx = torch.randint(0, 40, (77,), generator=ref._gen(1))
        R = ref.ref_gather(idx, E)
        got = torch.nn.functional.normalize(E[idx], dim=1)
        ref.assert_within({"gather": got}, R, ("gather",), f"gather C{C}", key="vq_cpu")


def test_abi_refusals():
    from amk import lib

    L = lib.load()
    null, p, off = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    err = lambda: L.amk_last_error().decode()  # noqa: E731

    def fwd(z=p, cb=p, N=3, K=8, C=32, ns=1, en=p, out=p, zq=p, zn=p, idx=p):
        return L.amk_vq_lookup_fwd(z, cb, N, K, C, ns, en, p, p, p, idx, out, zq, zn, p, null)

    def bwd(fn, z=p, N=3, K=8, C=128, dz=p, last=p, go=p):
        return fn(z, p, p, p, p, go, p, 0.25, N, K, C, dz, last, null)

    def gat(idx=p, cb=p, N=3, K=8, C=32, out=p):
        return L.amk_vq_gather(idx, cb, N, K, C, out, null, null)

    assert fwd(z=null) == -1 and "null" in err()
    assert fwd(idx=null) == -1 and fwd(en=null) == -1
    for kw in (dict(N=0), dict(K=0), dict(ns=0), dict(N=-5), dict(K=-1)):
        assert fwd(**kw) == -1 and "non-positive" in err(), kw
    for C in (0, 16, 48, 96, 512):
        assert fwd(C=C) == -2 and "not supported" in err(), C
        assert gat(C=C) == -2 and bwd(L.amk_vq_lookup_bwd, C=C) == -2 and bwd(L.amk_vq_lookup_bwd_rows, C=C) == -2
    for name in ("z", "cb", "en", "out", "zq", "zn"):
        assert fwd(**{name: off}) == -1 and "16-byte" in err(), name
    assert fwd(K=2 ** 22, C=256) == -2 and "too large" in err()
    for fn in (L.amk_vq_lookup_bwd, L.amk_vq_lookup_bwd_rows):
        assert bwd(fn, z=null) == -1 and bwd(fn, last=null) == -1 and "null" in err()
        assert bwd(fn, N=0) == -1 and bwd(fn, K=0) == -1 and "non-positive" in err()
        assert bwd(fn, z=off) == -1 and bwd(fn, dz=off) == -1 and bwd(fn, go=off) == -1 and "16-byte" in err()
    assert gat(idx=null) == -1 and gat(out=null) == -1 and gat(N=0) == -1 and gat(K=0) == -1
    assert L.amk_vq_padded_codes(40, 4) == 128 and L.amk_vq_padded_codes(5, 2) == 64 and L.amk_vq_padded_codes(0, 1) == 0
    for K, ns in ((1, 1), (500, 4), (768, 24), (1024, 32), (544, 17)):
        assert L.amk_vq_padded_codes(K, ns) == ref.padded_codes(K, ns)
    for N in (1, 16, 17, 257):
        assert L.amk_vq_num_partials(N) == ref.num_partials(N)
