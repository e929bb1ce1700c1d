"""The derived rounding bound of tests/iss_bounds.py on the CPU: what the reference itself
produced (the goldens; compiled with fastmath, float64) and both float64 oracles lie within
``c n_ops u A`` of the long-double oracle; the magnitude run dominates the value; and the bound
is tight enough to see a relative perturbation of 1e-9."""
import numpy as np
import pytest

import iss_bounds as ib
from conftest import load_golden
from oracle import c_oracle as corc
from oracle import ref_numpy as orc

G = load_golden()
REALS_GOLDEN = [c for c in G.cases("iss") if c.get("semiring", "Reals") == "Reals"]
COS_GOLDEN = G.manifest.get("coswiss", [])
N_HOST = 8          # (the arithmetic is per series: 64 series as on the GPU would add nothing here)


def test_extended_precision_is_there():
    """np.longdouble carries a 64-bit significand here; the bounds mean nothing without."""
    orc.require_extended_precision()
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_defaults_are_the_float64_oracle():
    """``dtype`` / ``magnitude`` default to the reference's arithmetic: float64 results."""
    X = ib.reals_input("normal", 3, 3, 40)
    lk = orc.lookup_l1(X, scale=3.0)
    a = orc.iss_transform(X, ib.WORDS, "EXTENDED", None, lk, True)
    b = orc.iss_transform(X, ib.WORDS, "EXTENDED", None, lk, True, dtype=np.float64, magnitude=False)
    assert a.dtype == np.float64 and np.array_equal(a, b)
    hp = orc.iss_transform(X, ib.WORDS, "EXTENDED", None, lk, True, dtype=np.longdouble)
    # (extended precision for real: values that no float64 holds, next to the float64 result)
    assert hp.dtype == np.longdouble and (hp != hp.astype(np.float64)).any()
    assert np.max(np.abs(hp - a)) < 1e-9
    c = orc.coswiss_transform(X, ib.WORDS[:2], [0.5], 2, True)
    d = orc.coswiss_transform(X, ib.WORDS[:2], [0.5], 2, True, dtype=np.float64, magnitude=False)
    assert c.dtype == np.float64 and np.array_equal(c, d)


def _golden_reals(case):
    X = G.x_of(case)
    if "series" in case:
        X = np.ascontiguousarray(X[case["series"]])
    lookup, total = orc._weight_lookup(case.get("weighting"), X, X)
    hp, A, n = ib.reals_reference(X, case["words"], case["mode"], case.get("alphas"), lookup, total)
    return X, hp, A, n


@pytest.mark.parametrize("case", REALS_GOLDEN, ids=lambda c: c["name"])
def test_reals_golden_within_bound(case):
    """(a) + (c): the reference's own float64 output against the long-double oracle."""
    _, hp, A, n = _golden_reals(case)
    assert np.all(A >= np.abs(hp))
    ib.check_bound(G[case["out"]], hp, A, n, case["name"])


@pytest.mark.parametrize("case", COS_GOLDEN, ids=lambda c: c["name"])
def test_coswiss_golden_within_bound(case):
    kw = case["kw"]
    hp, A, n = ib.coswiss_reference(G[case["x"]], case["words"], case["freqs"], kw.get("exponent", 2),
                                    kw.get("total_weighting", False))
    assert np.all(A >= np.abs(hp))
    ib.check_bound(G[case["out"]], hp, A, n, case["name"])


@pytest.mark.parametrize("T", ib.LENGTHS)
@pytest.mark.parametrize("family", list(ib.FAMILY_WORDS))
def test_reals_oracles_within_bound(family, T):
    """(b), (c), (d) on inputs drawn like the GPU cases' - their distributions, dimensions, lengths,
    words and weightings, 8 series of another draw -: the numpy and the C oracle within the bound,
    A >= |hp|, and the numpy oracle times (1 + 1e-9) outside it on the positive input."""
    D, words = ib.FAMILY_WORDS[family]
    for wname, spec in ib.WEIGHTINGS.items():
        for dist in ("normal", "uniform"):
            X = ib.reals_input(dist, N_HOST, D, T)
            lookup, total = orc._weight_lookup(spec, X, X)
            hp, A, n = ib.reals_reference(X, words, "EXTENDED", None, lookup, total)
            what = f"{family} T={T} {wname} {dist}"
            assert np.all(A >= np.abs(hp)), what
            ref = orc.iss_transform(X, words, "EXTENDED", None, lookup, total)
            ib.check_bound(ref, hp, A, n, what + " numpy")
            ib.check_bound(corc.iss_transform(X, words, "EXTENDED", None, lookup, total), hp, A, n,
                           what + " C")
            if dist == "uniform":
                assert ib.positive_precondition(hp, A) <= 1.0, what     # (all factors positive)
                assert ib.violates(ref * (1 + 1e-9), hp, A, n), what


@pytest.mark.parametrize("T", ib.COS_LENGTHS)
@pytest.mark.parametrize("exponent", ib.COS_EXPONENTS)
def test_coswiss_oracle_within_bound(exponent, T):
    words = ib.coswiss_words(T, exponent)
    for total in (False, True):
        for dist in ("positive", "zero_mean"):
            X = ib.coswiss_input(dist, 6, T)
            hp, A, n = ib.coswiss_reference(X, words, ib.COS_FREQS, exponent, total)
            what = f"coswiss exponent={exponent} T={T} total={total} {dist}"
            assert np.all(A >= np.abs(hp)), what
            ref = orc.coswiss_transform(X, words, ib.COS_FREQS, exponent, total)
            ib.check_bound(ref, hp, A, n, what)
            if dist == "positive" and exponent >= 2:
                # (exponent 1 cancels - cos(a - b) changes sign -: no such case)
                ib.positive_precondition(hp, A)
                assert ib.violates(ref * (1 + 1e-9), hp, A, n), what


def test_probe_positions():
    """Sorted, inside [0, T), the ends of the series and every boundary below T among them."""
    for T in (1, 2, 63, 300, 1025, 3000):
        p = ib.probe_positions(T)
        assert p == sorted(set(p)) and p[0] == 0 and p[-1] == T - 1 and all(0 <= v < T for v in p)
        want = {0, T - 1, T // 2, T // 3} | {v for v in (63, 64, 127, 128, 129, 255, 256, 257, 383, 384,
                                                          511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
                                             if v < T}
        assert (want | ({T - 2} if T >= 2 else set())) <= set(p)
    assert ib.probe_positions(1) == [0] and ib.probe_positions(2) == [0, 1]
    assert ib.segments(300, [100, -1]) == [(0, 100), (100, 300)]
    assert ib.segments(2, [0, -1]) == [(0, 0), (0, 2)]


FEATURE_WEIGHTINGS = ("none", "indices", "indices_total")


@pytest.mark.parametrize("T", [1, 2, 63, 300, 1025])
@pytest.mark.parametrize("weighting", FEATURE_WEIGHTINGS)
def test_feature_bounds_hold_the_oracle(weighting, T):
    """The feature bounds of ``ib.feature_reference`` - END at the probe cuts; MAX, MIN, MPI(inc=0)
    and MPI(inc=1) over [0, T//3) and [T//3, T) with open bands -: the float64 numpy oracle's
    features lie inside them against the long-double ones, and on the positive input (A == hp:
    ``positive_precondition`` holds of the oracle alone) the features of the rows times (1 + 1e-9)
    lie outside.  The one case without a sensitivity half is MPI(inc=1) at T = 1: its only
    feature is the padded increment, the constant 0, bound 0."""
    spec = ib.WEIGHTINGS[weighting]
    probes = [p + 1 for p in ib.probe_positions(T)]
    for dist in ("normal", "uniform"):
        X = ib.reals_input(dist, N_HOST, 3, T)
        lookup, total = orc._weight_lookup(spec, X, X)
        hp, A, n = ib.reals_reference(X, ib.WORDS, "EXTENDED", None, lookup, total)
        rows = orc.iss_transform(X, ib.WORDS, "EXTENDED", None, lookup, total)
        band = ib.open_band(A)
        assert band[0] < -float(np.abs(rows).max()) * 1.5 and float(np.abs(rows).max()) * 1.5 < band[1]
        if dist == "uniform":
            assert ib.positive_precondition(hp, A) <= 1.0
        for kind in ib.FEATURE_KINDS:
            cut = probes if kind == "END" else [T // 3, -1]
            what = f"{kind} T={T} {weighting} {dist}"
            ref, bnd = ib.feature_reference(kind, hp, A, n, cut)
            assert ref.shape == (hp.shape[0], N_HOST, len(cut)) and (bnd >= 0).all(), what
            ib.check_features(ib.oracle_features(kind, rows, cut, band), ref, bnd, what)
            if dist == "uniform" and not (kind == "MPI1" and T == 1):
                off = ib.oracle_features(kind, rows * (1 + 1e-9), cut, band)
                assert (ib.feature_ratio(off, ref, bnd) > 1.0).any(), what
                with pytest.raises(AssertionError):
                    ib.check_features(off, ref, bnd, what)


def test_check_features_wants_equality_where_the_bound_is_zero():
    """An empty segment ([0, T//3) at T = 2) and the leading zeros of a row: bound 0, values equal."""
    X = ib.reals_input("uniform", 2, 3, 2)
    hp, A, n = ib.reals_reference(X, ib.WORDS)
    for kind in ib.FEATURE_KINDS[1:]:
        ref, bnd = ib.feature_reference(kind, hp, A, n, [0, -1])
        assert (ref[..., 0] == 0).all() and (bnd[..., 0] == 0).all()
        got = ref.astype(np.float64)
        ib.check_features(got, ref, bnd, kind)
        got[0, 0, 0] = 1e-300
        with pytest.raises(AssertionError):
            ib.check_features(got, ref, bnd, kind)


def test_check_bound_sees_what_the_old_bars_passed():
    """The faults the row-wise 1e-6 bar let through: an exp table rounded through float, a wrong
    early element of a row that grows by 1e4, a carry dropped at a chunk boundary."""
    T = 1100
    X = ib.reals_input("uniform", 4, 3, T)
    lookup, total = orc._weight_lookup({"kind": "Indices", "scale": 2.0, "total": True}, X, X)
    hp, A, n = ib.reals_reference(X, ib.WORDS, "EXTENDED", None, lookup, total)
    ref = orc.iss_transform(X, ib.WORDS, "EXTENDED", None, lookup, total)
    ib.check_bound(ref, hp, A, n, "clean")
    through_float = orc.iss_transform(X, ib.WORDS, "EXTENDED", None,
                                      np.log(np.exp(lookup).astype(np.float32).astype(np.float64)), total)
    scale = np.abs(ref).max(axis=2, keepdims=True)
    assert np.max(np.abs(through_float - ref) / scale) <= 1e-6         # the old bar passes it
    with pytest.raises(AssertionError):
        ib.check_bound(through_float, hp, A, n, "exp table through float")
    early = ref.copy()
    early[0, :, 3] *= 1 + 1e-8
    with pytest.raises(AssertionError):
        ib.check_bound(early, hp, A, n, "early element")
    dropped = ref.copy()
    dropped[0, :, 1024:] -= ref[0, :, 1023:1024] * 1e-10            # a low-order part of the carry
    with pytest.raises(AssertionError):
        ib.check_bound(dropped, hp, A, n, "dropped carry")
    # the leading zeros of a word of L letters are exact
    zeros = ref.copy()
    zeros[2, :, 0] = 1e-300
    assert A[2, 0, 0] == 0
    with pytest.raises(AssertionError):
        ib.check_bound(zeros, hp, A, n, "leading zero")
