"""tests/sample_ref.py without a GPU: the numpy Philox4x32-10 against the published known-answer vectors; the word ->
uniform map strictly inside (0, 1) over all 2^24 inputs of an f32 emulation (and the 24-bit map it replaced reaching
u = 1 exactly once); the recorded (seed, offset) of the Gumbel test re-derived; every cap of the module asserted from the
reference alone (rows excluded from the guided threshold check, rows inside the prediction licence, rows inside the
in-kernel-noise licence); an f32 op chain on the CPU inside the licence and the score bound; planted defects outside;
the C ABI's refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

import sample_ref as ref


def test_philox_known_answers():
    # Random123's kat_vectors for philox4x32-10
    w = ref.philox4x32_10(0, 0, np.array([0], dtype=np.uint64))[0]
    assert [int(x) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFFFFFFFFFF
    w = ref.philox4x32_10(ones, ones, np.array([ones], dtype=np.uint64))[0]
    assert [int(x) for x in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    w = ref.philox4x32_10(0x299F31D0A4093822, 0x0370734413198A2E, np.array([0x85A308D3243F6A88], dtype=np.uint64))[0]
    assert [int(x) for x in w] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # element (row, j) of a call: counter low word row V / 4 + j / 4, lane j % 4
    full = ref.words(5, 9, 3, 64)
    assert np.array_equal(full[2, 20:24], ref.philox4x32_10(5, 9, np.array([2 * 16 + 5], dtype=np.uint64))[0])
    assert len(np.unique(full)) == full.size


def test_uniform_map_is_strictly_inside_the_unit_interval():
    top = np.arange(2 ** 24, dtype=np.uint32)              # every value of w >> 8
    u = ref.uniform_f32(top >> np.uint32(1), 23)           # the kernel: (float)(w >> 9) + 0.5f, times 2^-23, in f32
    assert u.dtype == np.float32 and float(u.min()) == 2.0 ** -24 and float(u.max()) == 1 - 2.0 ** -24
    assert np.array_equal(u.astype(np.float64), ref.uniform_of(top << np.uint32(8)))      # exact: no rounding at all
    g = -np.log(-np.log(u.astype(np.float64)))
    assert bool(np.isfinite(g).all()) and -3 < float(g.min()) and float(g.max()) < 17
    old = ref.uniform_f32(top, 24)                         # the 24-bit map: 16777215.5 is not an f32
    assert int((old == 1).sum()) == 1 and int((old == 0).sum()) == 0 and float(old[-1]) == 1.0


def test_gumbel_hit_constants():
    assert ref.find_gumbel_hit(ref.GUMBEL_HIT_SEED) == ref.GUMBEL_HIT
    off, row, j = ref.GUMBEL_HIT
    w = ref.words(ref.GUMBEL_HIT_SEED, off, ref.GUMBEL_HIT_ROWS, ref.GUMBEL_HIT_V)
    assert int(w[row, j]) >> 8 == 0xFFFFFF and int(((w >> np.uint32(8)) == 0xFFFFFF).sum()) == 1
    g = ref.gumbel_of(w)
    assert bool(np.isfinite(g).all()) and abs(float(g[row, j]) - (-math.log(2.0 ** -24))) < 1e-6
    # with a logit 40 below the others the hit position cannot win under the fixed map
    y = g[row].copy()
    y[j] -= 40
    assert int(y.argmax()) != j and float(np.sort(y)[-1] - y[j]) > 10


def test_in_kernel_noise_licence_is_never_needed():
    rows = within = 0
    preds = []
    for R, V in ref.NOISE_SHAPES:
        for seed, off in ref.NOISE_KEYS:
            g = ref.gumbel_of(ref.words(seed, off, R, V))
            srt = np.sort(g, axis=1)
            idx = np.argsort(g, axis=1)
            gap = srt[:, -1] - srt[:, -2]
            within += int((gap <= ref.dg(srt[:, -1]) + ref.dg(srt[:, -2])).sum())
            rows += R
            preds += [(R, V, seed, off, r, int(idx[r, -1])) for r in range(R)]
    assert within <= ref.MAX_LICENSED * rows and within == 0
    # the stream differs between rows, between the four lanes of a word and between offsets
    for R, V in ref.NOISE_SHAPES:
        w0, w1 = ref.words(1234, 0, R, V), ref.words(1234, 7, R, V)
        assert not np.array_equal(w0, w1) and len(np.unique(w0)) > 0.99 * w0.size
        assert all(not np.array_equal(w0[0, e::4], w0[0, (e + 1) % 4::4]) for e in range(4))
        assert R == 1 or not np.array_equal(w0[0], w0[1])
    assert len({p[-1] % 4 for p in preds}) > 1


@pytest.mark.parametrize("V", ref.VS)
def test_guided_threshold_rows_excluded(V):
    rows = excluded = 0
    for fam in ref.GUIDED_FAMILIES:
        for keep in ref.keeps(V):
            logits, null = ref.make_logits(fam, 5, V, 7 + keep), ref.make_logits(fam, 5, V, 8 + keep)
            s, ds = ref.scaled(logits, null, ref.CFG_SCALE)
            ok = ref.threshold_rows(s, ds, keep, "last")[4]
            rows += 5
            excluded += int((~ok).sum())
    print(f"V{V}: {excluded} of {rows} guided rows excluded")
    assert excluded <= ref.MAX_EXCLUDED * rows


@pytest.mark.parametrize("V", ref.VS)
def test_threshold_construction(V):
    """The planted noise decides: the fp64 reference picks the planted element, and the twin row the row's maximum; an
    exactly-k rule (torch.topk's) and a rule that orders -0.0 below +0.0 pick something else on the families with ties."""
    strict_differs = zero_differs = 0
    for fam in ref.FAMILIES:
        for keep in ref.keeps(V):
            logits = ref.make_logits(fam, 5, V, 7 + keep)
            s, ds = ref.scaled(logits, None, 1.0)
            for pick in ("first", "last"):
                g1, at, g2, want2, ok = ref.threshold_rows(s, ds, keep, pick)
                assert bool(ok.all())
                for g, want in ((g1, at), (g2, want2)):
                    P = ref.ref_pred(s, ds, g, keep)
                    use = want >= 0
                    assert bool(P["exact"][use].all()) and torch.equal(P["argmax"][use], want[use]), (fam, keep, pick)
                # exactly k kept (ties at the threshold cut by index): the last of the equal values falls out
                kept_k = torch.zeros_like(s, dtype=torch.bool).scatter_(1, torch.topk(s, keep, dim=1).indices, True)
                strict_differs += int((~kept_k[torch.arange(5), at]).sum())
                # -0.0 ordered below +0.0: a -0.0 at a threshold of +0.0 falls out
                bits = logits.view(torch.int32)
                thr_pos = (torch.where((s == ref.kth_largest(s, keep)) & (bits >= 0), 1, 0).sum(1) > 0)
                zero_differs += int(((bits[torch.arange(5), at] < 0) & (logits[torch.arange(5), at] == 0) & thr_pos).sum())
    if V >= 64:
        assert strict_differs > 0 and zero_differs > 0, (strict_differs, zero_differs)


@pytest.mark.parametrize("V", ref.VS)
@pytest.mark.parametrize("guided", [False, True])
def test_prediction_licence_share_and_f32_chain(V, guided):
    rows = short = 0
    for case in ref.noise_cases(V, guided):
        fam, keep, R, tau, _, _, _ = case
        logits, null, g, _ = ref.noise_problem(V, guided, case)
        s, ds = ref.scaled(logits, null, ref.CFG_SCALE)
        P = ref.ref_pred(s, ds, g, keep)
        if tau > 0:
            rows += R
            short += int((~P["exact"]).sum())
        pred, score = ref.emulate(logits, null, ref.CFG_SCALE, g, keep, tau)
        ref.check_pred(P, pred, tau, f"f32 chain {case}")
        S = ref.ref_score(s, ds, pred)
        assert bool(torch.isfinite(S["bound_score"]).all())
        ref.assert_within({"score": score}, S, ("score",), f"f32 chain {case}", key="sample_cpu")
        if fam == "gaussian" and V >= 64:
            q = ref.ratios({"score": score * (1 + 3e-5)}, S, ("score",))
            assert q["score"][0] > 0
    print(f"V{V} guided{int(guided)}: {short} of {rows} rows inside the prediction licence")
    assert short <= ref.MAX_LICENSED * rows


def test_small_probabilities_carry_a_relative_bound():
    for V in (64, 1028, 8192):
        logits, g, at = ref.make_small_prob(5, V, V)
        s, ds = ref.scaled(logits, None, 1.0)
        P = ref.ref_pred(s, ds, g, V)
        assert bool(P["exact"].all()) and torch.equal(P["argmax"], at)
        pred, score = ref.emulate(logits, None, 1.0, g, V, 1.0)
        assert torch.equal(pred, at)
        S = ref.ref_score(s, ds, pred)
        assert bool((S["score"] < 1e-20).all() and (S["score"] > 1e-37).all())
        assert bool((S["bound_score"] <= 3e-5 * S["score"]).all())
        ref.assert_within({"score": score}, S, ("score",), f"small probabilities V{V}", key="sample_cpu")


def test_abi_refusals():
    from amk import lib

    L = lib.load()
    null, p, off = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    err = lambda: L.amk_last_error().decode()  # noqa: E731

    def call(logits=p, nl=null, g=null, R=3, V=64, keep=7, ids=p, scores=p):
        return L.amk_sample_step(logits, nl, 3.0, g, 1, 2, 1.0, R, V, keep, null, -1.0, ids, scores, null)

    assert call(logits=null) == -1 and "null" in err()
    assert call(ids=null) == -1 and call(scores=null) == -1
    for kw in (dict(R=0), dict(V=0), dict(keep=0), dict(keep=65), dict(keep=-1), dict(R=-2)):
        assert call(**kw) == -1 and "bad sizes" in err(), kw
    for V in (6, 1001, 36868, 40000):
        assert call(V=V, keep=1) == -2 and "multiple of 4" in err(), V
    for kw in (dict(logits=off), dict(nl=off), dict(g=off)):
        assert call(**kw) == -1 and "16-byte" in err(), kw
    assert call(R=2 ** 31) == -2
