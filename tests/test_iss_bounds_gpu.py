"""The HIP kernels of the Reals iterated sums, of CosWISS and of the fast path-length lookup
against the derived elementwise bound of tests/iss_bounds.py: ``|gpu - hp| <= c n_ops u A`` with hp
and A from the long-double oracle on the CPU - seven (Reals) and five (CosWISS) orders of magnitude
below the row-wise 1e-6 bars of test_hip_parity.py, and at every element, not against the row's
largest.

One case per kernel family of the walk, each asserting through ``Plan.last_launch()`` /
``jit_loaded()`` that the family ran; 64 series, every length of ``iss_bounds.LENGTHS`` the family
accepts (the packed limit, one chunk, a multi-chunk carry), the words of the CPU check plus the
family's own, no weighting / Indices(scale=2) / L1(scale=3), total and non-total, a zero-mean and
a positive input.  A weighted case hands the DEVICE'S OWN lookup (read back) to the oracle: the
lookup's rounding is tested on its own (test_fast_pathlen_lookup) and is no part of this bound.

The largest err / bound per family is printed at the end (``ISS-RATIO``)."""
import numpy as np
import pytest

import iss_bounds as ib
from test_hip_parity import _require_hiprtc, make_weighting

pytestmark = pytest.mark.gpu
N_SERIES = 64


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    yield fruits_amd
    ib.print_ratios()


@pytest.fixture(scope="module")
def hiprtc(fr):
    """The run-time compiler, asked once before any work of the tests that need it (skips them
    where hipRTC is not installed): a program that then fails to compile or load is a failure."""
    strs = ib.FAMILY_WORDS["static_jit"][1]
    plan = fr.ISS([fr.words.SimpleWord(s) for s in strs], mode=fr.ISSMode.EXTENDED)._plan(0, len(strs))
    assert plan.static_schedule(1) is not None
    _require_hiprtc(plan)


def _knobs(monkeypatch, **knobs):
    monkeypatch.setenv("FRUITS_HIP_DEBUG", ",".join(f"{k}={v}" for k, v in knobs.items()))


# family -> (environment, lengths it accepts, weightings it accepts)
#   interpreter: a short plan (<= 32 nodes) without a static program; packed=0 keeps it on short series
#   lean:        more than 32 nodes (launch_choice.h: lean_shape); two input dimensions and one alpha
#                stage four rows, so the chunk carries fit its LDS at every length
#   packed:      T <= 256, and T <= 384 for words of at most four letters (packed_supported)
#   static_aot:  of_weight(2, 3), unweighted, one aligned chunk of 513 ... 1024 elements below 768 series
#   static_jit:  another word set of the same shapes, compiled at run time (hipRTC)
ALL_W = tuple(ib.WEIGHTINGS)
FAMILIES = {
    "interpreter": dict(env={"FRUITS_HIP_JIT": "0"}, knobs=dict(packed=0), lengths=ib.LENGTHS, weightings=ALL_W),
    "lean": dict(env={"FRUITS_HIP_JIT": "0"}, knobs=dict(packed=0), lengths=ib.LENGTHS, weightings=ALL_W),
    "packed": dict(env={}, knobs={}, lengths=(1, 2, 63, 300), weightings=ALL_W),
    "static_aot": dict(env={"FRUITS_HIP_STATIC": "1"}, knobs={}, lengths=(514, 1000, 1024), weightings=("none",)),
    "static_jit": dict(env={"FRUITS_HIP_JIT": "1"}, knobs={}, lengths=(514, 1000, 1024), weightings=("none",)),
}
REALS_CASES = [(f, T, w) for f, c in FAMILIES.items() for T in c["lengths"] for w in c["weightings"]]


@pytest.mark.parametrize("family,T,weighting", REALS_CASES, ids=lambda v: str(v))
def test_reals_family_within_bound(fr, request, monkeypatch, tmp_path, family, T, weighting):
    import torch
    from fruits_amd import _native as nat
    cfg = FAMILIES[family]
    for k, v in cfg["env"].items():
        monkeypatch.setenv(k, v)
    if cfg["knobs"]:
        _knobs(monkeypatch, **cfg["knobs"])
    if family == "static_jit":
        request.getfixturevalue("hiprtc")
        monkeypatch.setenv("FRUITS_HIP_JIT_CACHE", str(tmp_path / "jit"))
    D, strs = ib.FAMILY_WORDS[family]
    spec = ib.WEIGHTINGS[weighting]
    total = bool(spec and spec.get("total", False))
    for dist in ("normal", "uniform"):
        iss = fr.ISS([fr.words.SimpleWord(s) for s in strs], mode=fr.ISSMode.EXTENDED,
                     weighting=make_weighting(fr, spec))
        plan = iss._plan(0, len(strs))
        X = ib.reals_input(dist, N_SERIES, D, T)
        iss._attach_cache(X)
        Xd = nat.to_device(X)
        lk = iss.lookup_device(Xd)
        if family == "static_jit":
            assert plan.static_schedule(1) is not None and plan.static_program_index(1) == 0
            plan.prepare(N_SERIES, T)
            assert plan.jit_loaded() >= 1
        out = plan.run(Xd, lk)
        torch.cuda.synchronize()
        ran = plan.last_launch()
        assert ran["family"] == family, (family, T, weighting, ran)
        got = nat.to_host(out)
        hp, A, n = ib.reals_reference(X, strs, "EXTENDED", None, None if lk is None else nat.to_host(lk), total)
        what = f"{family} T={T} {weighting} {dist}"
        if dist == "uniform":
            assert ib.positive_precondition(hp, A) <= 1.0, what
        ib.check_bound(got, hp, A, n, what, family)


@pytest.mark.parametrize("weighting", list(ib.WEIGHTINGS))
@pytest.mark.parametrize("T", ib.LENGTHS)
def test_pieces_within_bound(fr, hiprtc, monkeypatch, T, weighting):
    """A plan in pieces (walk_fused.h fwalk_pieces: chains by the record loop, bodies as straight-line
    code, one kernel per piece type - test_large_plan_in_pieces).  It exists as a fused pipeline only,
    so the rows are read through END sieves: the row values at the ends, around a third and a half of
    the series.  The lean family's plan cut into pieces of at most 8 nodes.  The pipeline is run the
    way ``Fruit.transform`` runs it - ``pipe.run(Xd, iss.lookup_device(Xd))`` - with the lookup
    kept: the oracle gets the device's own, the N rows of L1 too."""
    from fruits_amd import _native as nat
    from fruits_amd.cache import SharedSeedCache
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    _knobs(monkeypatch, pieces=1, piece_min=30, piece_nodes=8, packed=0)
    D, strs = ib.FAMILY_WORDS["lean"]
    spec = ib.WEIGHTINGS[weighting]
    total = bool(spec and spec.get("total", False))
    cuts = sorted({c for c in (1, 2, 3, T // 3, T // 2, T - 1, T) if 1 <= c <= T})
    fruit = fr.Fruit("pieces")
    iss = fr.ISS([fr.words.SimpleWord(s) for s in strs], mode=fr.ISSMode.EXTENDED,
                 weighting=make_weighting(fr, spec))
    fruit.add(iss)
    fruit.add(fr.sieving.END(cut=cuts))
    slc = fruit.get_slice()
    slc.fit_sample_size = 1.0
    np.random.seed(4)
    fruit.fit(ib.reals_input("normal", N_SERIES, D, T))
    pipe = slc._fused(T)
    assert pipe is not None
    cover = pipe.plan.pieces(8)
    assert cover is not None and len(cover["types"]) >= 2
    pipe.prepare(N_SERIES)
    assert pipe.pieces_loaded() == len(cover["types"])
    iss = slc._iss[0]
    for dist in ("normal", "uniform"):
        X = ib.reals_input(dist, N_SERIES, D, T)
        cache = SharedSeedCache(X)
        Xd = cache.input_device(X)
        slc._attach(cache)                       # (the weighting reads the raw input from the cache)
        lk = iss.lookup_device(Xd)
        feats = nat.to_host(pipe.run(Xd, lk))
        assert pipe.last_launch()["family"] == "fused_pieces", pipe.last_launch()
        hp, A, n = ib.reals_reference(X, strs, "EXTENDED", None, None if lk is None else nat.to_host(lk), total)
        at = np.array(cuts) - 1
        K = hp.shape[0]
        assert feats.shape == (N_SERIES, K * len(cuts))
        got = feats.reshape(N_SERIES, K, len(cuts)).transpose(1, 0, 2)
        ib.check_bound(got, hp[:, :, at], A[:, :, at], n, f"pieces T={T} {weighting} {dist}", "fused_pieces")


COS_CASES = [(p, e, T) for T in ib.COS_LENGTHS for e in ib.COS_EXPONENTS
             for p in ((0, 1) if T <= 384 else (0,))]


@pytest.mark.parametrize("packed,exponent,T", COS_CASES, ids=lambda v: str(v))
def test_coswiss_within_bound(fr, monkeypatch, packed, exponent, T):
    """The cooperative (packed=0; all of T > 384) and the wave-per-unit kernel (packed=1, T <= 384),
    term-expanded exponents 1 ... 4 and a factorised one (6), total and non-total weighting.
    Which of the two kernels ran is NOT asserted: a CosWISS launch leaves no record
    (``last_launch`` is the trie walk's).  The host takes the wave-per-unit kernel for
    ``T <= 384`` unless the knob says 0, whatever the words (capi_walk.cpp), so the family a
    ratio is recorded under is the knob's."""
    _knobs(monkeypatch, packed=packed)
    words = ib.coswiss_words(T, exponent)
    family = "coswiss_packed" if packed else "coswiss_cooperative"
    for total in (False, True):
        cw = fr.CosWISS([fr.words.SimpleWord(s) for s in words], ib.COS_FREQS, exponent=exponent,
                        total_weighting=total)
        for dist in ("positive", "zero_mean"):
            X = ib.coswiss_input(dist, 6, T)
            got = cw.fit_transform(X)
            hp, A, n = ib.coswiss_reference(X, words, ib.COS_FREQS, exponent, total)
            what = f"{family} exponent={exponent} T={T} total={total} {dist}"
            if dist == "positive" and exponent >= 2:
                ib.positive_precondition(hp, A)
            ib.check_bound(got, hp, A, n, what, family)


@pytest.mark.parametrize("T", [1, 2, 511, 512, 513, 1024, 1025, 4097])
def test_fast_pathlen_lookup(fr, T):
    """``pathlen_lookup_kernel`` with FR_LOOKUP_FAST - the scan in tiles of 512 that every Reals
    L1 / L2 plan takes its lookup from - against the long-double cumulative sum of the same
    float64 summands: the raw sums (non-negative summands) within 2 T u hp, the normalised forms
    within (2 T + 6) u scale (the division by last + 1e-5, the subtraction and division of the
    min-max step, the scaling).  ``exact=True`` is np.cumsum bit for bit (T = 4097 crosses its
    4096-element LDS segment)."""
    from fruits_amd import _native as nat
    HP = ib.HP
    X = np.random.default_rng(T).standard_normal((5, 2, T)).cumsum(axis=2) / 4.0
    Xd = nat.to_device(X)
    inc = np.zeros((5, T))
    inc[:, 1:] = X[:, 0, 1:] - X[:, 0, :-1]
    scale = 3.0
    for norm in (1, 2):
        terms = np.abs(inc) if norm == 1 else inc * inc
        hp = np.cumsum(terms.astype(HP), axis=1)
        raw = nat.to_host(nat.pathlen_lookup(Xd, norm, 2, scale, exact=False))
        err = np.abs(raw.astype(HP) - hp)
        assert np.all(err <= HP(2 * T * ib.U) * hp), (norm, T, float(np.max(err / np.where(hp > 0, hp, 1))))
        ib.RATIOS["lookup_raw"] = max(ib.RATIOS.get("lookup_raw", 0.0),
                                      float(np.max(err / np.where(hp > 0, HP(2 * T * ib.U) * hp, 1))))
        np.testing.assert_array_equal(nat.to_host(nat.pathlen_lookup(Xd, norm, 2, scale, exact=True)),
                                      np.cumsum(terms, axis=1))
        for relative in (0, 1):
            r = hp / (hp[:, -1:] + HP(1e-5)) if relative else hp
            mn, mx = r.min(axis=1, keepdims=True), r.max(axis=1, keepdims=True)
            ref = np.where(mn != mx, (r - mn) / np.where(mn != mx, mx - mn, 1), 0) * HP(scale)
            dev = nat.to_host(nat.pathlen_lookup(Xd, norm, relative, scale, exact=False))
            err = np.abs(dev.astype(HP) - ref)
            b = HP((2 * T + 6) * ib.U * scale)
            assert np.all(err <= b), (norm, relative, T, float(err.max() / b))
            ib.RATIOS["lookup_normalised"] = max(ib.RATIOS.get("lookup_normalised", 0.0), float(err.max() / b))
