"""csrc/sample.hip held to tests/sample_ref.py through the raw C ABI: the radix-select threshold pinned exactly by planted
noise (the element at the threshold must be chosen, the one just below it never) on eight logit families -- negative
logits, values that differ in the last byte only, +-1e30, subnormals, -inf, bf16 ties at the threshold, signed zeros --
at V = 4 .. 36864 and keep = 1 .. V; predictions under random noise inside the licence and the chosen probability inside
a relative per-row bound, with and without guidance and masks, tau = 1, 1/18 and 0; probabilities below 1e-20; the
in-kernel Philox stream against the numpy Philox of the reference (argmax of the Gumbel noise on equal logits); the word
that the 24-bit uniform map sent to g = +inf; rows independent of their number and position, bitwise."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import sample_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL = -12345


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    worst = {k: v for k, v in ref.WORST.items() if k.startswith("sample.")}
    print("worst |got - ref| / bound:", {k: round(v, 4) for k, v in sorted(worst.items())})
    path = os.environ.get("AMK_SAMPLE_BOUND_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(worst, f, indent=1, sort_keys=True)


def _P(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _step(device, logits, keep, null=None, g=None, seed=0, offset=0, tau=1.0, mask=None, unmasked=-1.0, scale=ref.CFG_SCALE):
    """amk_sample_step -> (ids, scores) on the CPU; ids start at SENTINEL, scores at NaN, both between guard elements."""
    from amk import lib

    L = lib.load()
    R, V = logits.shape
    dev = lambda t: None if t is None else t.contiguous().to(device)  # noqa: E731
    ld, nd, gd = dev(logits), dev(null), dev(g)
    md = None if mask is None else mask.to(torch.uint8).to(device)
    ids = torch.full((R + 2,), SENTINEL, device=device, dtype=torch.int64)
    sc = torch.full((R + 2,), float("nan"), device=device)
    rc = L.amk_sample_step(_P(ld), _P(nd), scale, _P(gd), seed, offset, tau, R, V, keep, _P(md), unmasked,
                           ctypes.c_void_p(ids.data_ptr() + 8), ctypes.c_void_p(sc.data_ptr() + 4), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    lib.check(rc, "amk_sample_step")
    torch.cuda.synchronize()
    ids, sc = ids.cpu(), sc.cpu()
    assert int(ids[0]) == SENTINEL and int(ids[-1]) == SENTINEL and bool(torch.isnan(sc[[0, -1]]).all()), "wrote outside its rows"
    return ids[1:-1], sc[1:-1]


@pytest.mark.parametrize("V", ref.VS)
def test_threshold_is_exact(device, V):
    for guided in (False, True):
        for fam in (ref.GUIDED_FAMILIES if guided else ref.FAMILIES):
            for keep in ref.keeps(V):
                logits = ref.make_logits(fam, 5, V, 7 + keep)
                null = ref.make_logits(fam, 5, V, 8 + keep) if guided else None
                s, ds = ref.scaled(logits, null, ref.CFG_SCALE)
                for pick in ("first", "last"):
                    g1, at, g2, want2, ok = ref.threshold_rows(s, ds, keep, pick)
                    two = lambda t: None if t is None else torch.cat([t, t])  # noqa: E731
                    ids, _ = _step(device, two(logits), keep, null=two(null), g=torch.cat([g1, g2]))
                    what = f"{fam} V{V} keep{keep} {pick} guided{int(guided)}"
                    assert torch.equal(ids[:5][ok], at[ok]), f"{what}: the element at the threshold was not kept: {ids[:5]} != {at}"
                    use = ok & (want2 >= 0)
                    assert torch.equal(ids[5:][use], want2[use]), f"{what}: an element below the threshold was kept: {ids[5:]} != {want2}"


@pytest.mark.parametrize("V", ref.VS)
@pytest.mark.parametrize("guided", [False, True])
def test_prediction_and_score(device, V, guided):
    differ = 0
    for case in ref.noise_cases(V, guided):
        fam, keep, R, tau, masked, unmasked, _ = case
        logits, null, g, mask = ref.noise_problem(V, guided, case)
        ids, sc = _step(device, logits, keep, null=null, g=g, tau=tau, mask=mask, unmasked=unmasked)
        # a second call without a mask: every row's prediction
        pred, sc_all = _step(device, logits, keep, null=null, g=g, tau=tau)
        s, ds = ref.scaled(logits, null, ref.CFG_SCALE)
        what = f"sample {case} guided{int(guided)}"
        differ += ref.check_pred(ref.ref_pred(s, ds, g, keep), pred, tau, what)
        S = ref.ref_score(s, ds, pred)
        ref.assert_within({"score": sc_all}, S, ("score",), what, key="sample")
        assert bool(torch.isfinite(sc_all).all())
        if mask is None:
            assert torch.equal(ids, pred) and torch.equal(sc, sc_all), f"{what}: two calls differ"
        else:
            assert torch.equal(ids[mask], pred[mask]) and bool((ids[~mask] == SENTINEL).all()), f"{what}: ids outside the mask"
            want = torch.where(mask | (unmasked < 0), sc_all, torch.tensor(unmasked))
            assert torch.equal(sc, want), f"{what}: scores under the mask"
    print(f"V{V} guided{int(guided)}: {differ} rows differ from the fp64 argmax inside the licence")


@pytest.mark.parametrize("V", [64, 1028, 8192])
def test_small_probabilities(device, V):
    logits, g, at = ref.make_small_prob(5, V, V)
    ids, sc = _step(device, logits, V, g=g)
    assert torch.equal(ids, at)
    s, ds = ref.scaled(logits, None, 1.0)
    S = ref.ref_score(s, ds, ids)
    assert bool((S["score"] < 1e-20).all())
    ref.assert_within({"score": sc}, S, ("score",), f"small probabilities V{V}", key="sample_small")


@pytest.mark.parametrize("R,V", ref.NOISE_SHAPES)
def test_in_kernel_noise_is_the_reference_stream(device, R, V):
    seen = {}
    for seed, off in ref.NOISE_KEYS:
        g = ref.gumbel_of(ref.words(seed, off, R, V))
        ids, sc = _step(device, torch.zeros(R, V), V, seed=seed, offset=off)
        n = np.arange(R)
        p = ids.numpy()
        assert bool(((p >= 0) & (p < V)).all())
        best = g.argmax(1)
        short = g[n, p] + ref.dg(g[n, p]) < g[n, best] - ref.dg(g[n, best])
        assert not short.any(), f"seed {seed} offset {off}: rows {np.nonzero(short)[0]} do not follow the reference stream"
        assert np.array_equal(p, best), "no row of these cases is inside the licence (asserted on the CPU)"
        assert bool((sc == 1.0 / V).all())
        seen[(seed, off)] = p
    # the stream differs between offsets and seeds, and between rows.  What holds rows and the four lanes of a word to
    # their own draws is the equality with the reference's argmax above (a stream repeated across rows or lanes has another
    # argmax; the CPU test asserts that the reference's words differ there): the checks below only restate it.
    keys = list(seen)
    assert all(not np.array_equal(seen[a], seen[b]) for i, a in enumerate(keys) for b in keys[i + 1:])
    if R > 1:
        assert all(len(set(v.tolist())) > 1 for v in seen.values())


def test_every_word_gives_finite_noise(device):
    """The word whose top 24 bits are set: under a 24-bit uniform map u rounds to 1 and g = +inf, so its position wins
    whatever its logit.  Its logit is 40 below every other; it must not be chosen, and the scores are finite."""
    off, row, j = ref.GUMBEL_HIT
    R, V = ref.GUMBEL_HIT_ROWS, ref.GUMBEL_HIT_V
    logits = torch.zeros(R, V)
    logits[row, j] = -40.0
    ids, sc = _step(device, logits, V, seed=ref.GUMBEL_HIT_SEED, offset=off)
    assert bool(torch.isfinite(sc).all()), sc
    assert int(ids[row]) != j, "the word with its top 24 bits set won against a logit 40 above it: g = +inf"
    g = ref.gumbel_of(ref.words(ref.GUMBEL_HIT_SEED, off, R, V)) + logits.double().numpy()
    assert np.array_equal(ids.numpy(), g.argmax(1))


@pytest.mark.parametrize("V", [64, 1028, 36864])
def test_rows_are_independent(device, V):
    R = 5
    logits, null, g = ref.make_logits("bf16_ties", R, V, 3), ref.make_logits("gaussian", R, V, 4), ref.make_gumbel(R, V, 5)
    keep = math.ceil(0.1 * V)
    for nl in (None, null):
        ids, sc = _step(device, logits, keep, null=nl, g=g)
        ids2, sc2 = _step(device, logits, keep, null=nl, g=g)
        assert torch.equal(ids, ids2) and torch.equal(sc, sc2), "two calls with the same noise differ"
        perm = torch.tensor([3, 0, 4, 2, 1])
        idp, scp = _step(device, logits[perm], keep, null=None if nl is None else nl[perm], g=g[perm])
        assert torch.equal(ids[perm], idp) and torch.equal(sc[perm], scp), "a row depends on its position"
        for r in (0, 4):
            i1, s1 = _step(device, logits[r:r + 1], keep, null=None if nl is None else nl[r:r + 1], g=g[r:r + 1])
            assert torch.equal(ids[r:r + 1], i1) and torch.equal(sc[r:r + 1], s1), "a row depends on the number of rows"
