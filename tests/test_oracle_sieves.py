"""The oracle's MAX / MIN / XPI / LPI (oracle/ref_numpy.py) pinned against the outputs of the
reference itself (tests/golden/golden_sieves.json, make_golden_sieves.py) and against rows whose
answers are known by hand."""
import copy
import json
import os

import numpy as np
import pytest

from oracle import ref_numpy as orc

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_sieves.json")) as _f:
    MANIFEST = json.load(_f)
ARRAYS = np.load(os.path.join(HERE, "golden", "golden_sieves.npz"))


def _quantiles(case):
    return np.array([np.inf if v == "inf" else (-np.inf if v == "-inf" else v)
                     for v in case["quantiles"]])


def _masked_extreme(kind, A, cuts, q):
    """MAX / MIN per (segment, band) by masking with -inf / +inf instead of selecting: an
    empty band (no finite survivor) gives 0.0."""
    N, Q = A.shape[0], len(q) - 1
    out = np.zeros((N, (cuts.shape[1] - 1) * Q))
    fill = -np.inf if kind == "MAX" else np.inf
    for n in range(N):
        for j in range(cuts.shape[1] - 1):
            seg = A[n, cuts[n, j]:cuts[n, j + 1]]
            for k in range(Q):
                m = (q[k] < seg) & (seg <= q[k + 1])
                v = np.where(m, seg, fill)
                out[n, j * Q + k] = (v.max() if kind == "MAX" else v.min()) if m.any() else 0.0
    return out


@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_golden_sieve(case):
    kw = dict(case["kw"])
    sv = orc.SieveOracle(case["kind"], **kw)
    A = ARRAYS[case["x"]]
    sv.fit(A)
    out = sv.transform(A)
    assert out.shape == (A.shape[0], case["nfeatures"])
    if "out" in case:
        np.testing.assert_allclose(sv.quantiles, _quantiles(case), rtol=1e-12, atol=0)
        ref = ARRAYS[case["out"]]
        if case["kind"] in ("XPI", "LPI"):
            np.testing.assert_array_equal(out, ref)       # positions and run lengths: exact
        else:
            np.testing.assert_allclose(out, ref, rtol=1e-12, atol=0)
        return
    # the reference raises (np.max / np.min of an empty band of a non-empty segment): here
    # 0.0 there, and the in-band extreme wherever the band is not empty
    assert case["reference_raises"] == "ValueError" and case["kind"] in ("MAX", "MIN")
    cuts = orc.transformed_cuts(A.shape[0], A.shape[1], sv.cut, A[:, None, :], sv.norm)
    want = _masked_extreme(case["kind"], A, cuts, sv.quantiles)
    np.testing.assert_array_equal(out, want)
    assert (out == 0.0).any()


def _fit_all(spec):
    # make_golden_sieves.py fits every fruit on the whole input (fit_sample_size = 1.0)
    spec = copy.deepcopy(spec)
    for sl in spec["slices"]:
        sl["fit_sample_size"] = 1.0
    return spec


@pytest.mark.parametrize("case", MANIFEST["fruit"], ids=lambda c: c["name"])
def test_golden_fruit(case):
    X = ARRAYS[case["x"]]
    spec = _fit_all(case["spec"])
    fitted = orc.fruit_fit(spec, X)
    out = orc.fruit_transform(spec, fitted, X)
    assert out.shape[1] == case["nfeatures"]
    # (the criterion of test_oracle.py::test_fruit)
    np.testing.assert_allclose(out, ARRAYS[case["out"]], rtol=1e-12, atol=1e-12)


def test_kinds_and_defaults():
    for kind in ("NPI", "MPI", "XPI", "LPI"):
        sv = orc.SieveOracle(kind, inc=3)
        assert sv.q == (0.0, 1.0) and sv.inc == 3
    for kind in ("MAX", "MIN", "END"):
        sv = orc.SieveOracle(kind, inc=3)
        assert sv.q == (-1.0, 1.0) and sv.inc == 0
    A = np.array([[1.0, -2.0, 3.0, 0.5]])
    np.testing.assert_array_equal(orc.SieveOracle("MAX").transform(A), [[3.0]])
    np.testing.assert_array_equal(orc.SieveOracle("MIN").transform(A), [[-2.0]])
    # the increments are 0, -3, 5, -2.5: in (0, inf] one, in (-inf, inf] all four
    np.testing.assert_array_equal(orc.SieveOracle("XPI", q=(-1.0, 1.0)).transform(A), [[1.5]])
    np.testing.assert_array_equal(orc.SieveOracle("LPI", q=(-1.0, 1.0)).transform(A), [[4.0]])
    np.testing.assert_array_equal(orc.SieveOracle("LPI").transform(A), [[1.0]])
    np.testing.assert_array_equal(orc.SieveOracle("XPI").transform(A), [[2.0]])
    for bad in ("XYZ", "max", ""):
        with pytest.raises(ValueError):
            orc.SieveOracle(bad)


def _run(kind, row, q, cut=-1, inc=0):
    sv = orc.SieveOracle(kind, cut=cut, q=q, inc=inc)
    return sv.transform(np.asarray(row, dtype=np.float64)[None, :])[0]


def test_hand_made_rows():
    q = (-1.0, 0.0, 1.0)          # bands (-inf, 0] and (0, inf]
    #       0    1    2    3    4    5    6    7
    row = [2.0, 3.0, -1.0, 4.0, 5.0, 6.0, -2.0, 7.0]
    # positive: runs [0, 2), [3, 6), [7, 8) - longest 3; a run at the start and one at the end
    np.testing.assert_array_equal(_run("LPI", row, q), [1.0, 3.0])
    np.testing.assert_array_equal(_run("XPI", row, q), [(2 + 6) / 2, (0 + 1 + 3 + 4 + 5 + 7) / 6])
    np.testing.assert_array_equal(_run("MAX", row, q), [-1.0, 7.0])
    np.testing.assert_array_equal(_run("MIN", row, q), [-2.0, 2.0])
    # cut [4, -1]: segments [0, 4) and [4, 8); XPI counts from the segment start
    np.testing.assert_array_equal(_run("XPI", row, q, cut=[4, -1]), [2.0, 4 / 3, 2.0, 4 / 3])
    np.testing.assert_array_equal(_run("LPI", row, q, cut=[4, -1]), [1.0, 2.0, 1.0, 2.0])
    # a run that ends exactly at the segment end, and one that fills the whole segment
    np.testing.assert_array_equal(_run("LPI", [-1.0, 1.0, 1.0, 1.0], q), [1.0, 3.0])
    whole = [1.0, 2.0, 3.0]
    np.testing.assert_array_equal(_run("LPI", whole, q), [0.0, 3.0])
    np.testing.assert_array_equal(_run("XPI", whole, q), [0.0, 1.0])
    np.testing.assert_array_equal(_run("MAX", whole, q), [0.0, 3.0])
    np.testing.assert_array_equal(_run("MIN", whole, q), [0.0, 1.0])
    # an empty segment (cut [2, 2]): 0.0 for every kind and band
    for kind in ("MAX", "MIN", "XPI", "LPI", "NPI", "MPI"):
        out = _run(kind, whole, q, cut=[2, 2, -1])
        np.testing.assert_array_equal(out[2:4], [0.0, 0.0], err_msg=kind)
    # a cut beyond the series' end is clamped to it ([10, 10]: empty)
    for kind in ("MAX", "MIN", "XPI", "LPI"):
        np.testing.assert_array_equal(_run(kind, whole, q, cut=[10, 10])[2:], [0.0, 0.0], err_msg=kind)


def test_thresholds_and_nan():
    # q_lo < v <= q_hi: an element equal to q_hi is in the band, one equal to q_lo is not
    q = (-1.0, 0.0, 1.0)
    row = [0.0, -3.0, 0.0, 2.0]
    np.testing.assert_array_equal(_run("MAX", row, q), [0.0, 2.0])
    np.testing.assert_array_equal(_run("MIN", row, q), [-3.0, 2.0])
    np.testing.assert_array_equal(_run("XPI", row, q), [1.0, 3.0])
    np.testing.assert_array_equal(_run("LPI", row, q), [3.0, 1.0])
    # the same with fitted thresholds that ARE data points
    sv = orc.SieveOracle("LPI", q=(0.5, 1.0), inc=0)
    A = np.array([[1.0, 2.0, 3.0, 4.0, 5.0]])
    sv.fit(A)
    assert sv.quantiles[0] == 3.0
    np.testing.assert_array_equal(sv.transform(A), [[2.0]])          # 4, 5 (3 is not in)
    sv = orc.SieveOracle("MIN", q=(0.5, 1.0))
    sv.fit(A)
    np.testing.assert_array_equal(sv.transform(A), [[4.0]])
    # NaN is in no band, not even (-inf, inf]; it breaks a run
    row = [1.0, np.nan, 2.0, 3.0, np.nan]
    full = (-1.0, 1.0)
    np.testing.assert_array_equal(_run("MAX", row, full), [3.0])
    np.testing.assert_array_equal(_run("MIN", row, full), [1.0])
    np.testing.assert_array_equal(_run("XPI", row, full), [(0 + 2 + 3) / 3])
    np.testing.assert_array_equal(_run("LPI", row, full), [2.0])
    np.testing.assert_array_equal(_run("MAX", [np.nan, np.nan], full), [0.0])
    # +inf is in (q, inf], -inf in no band
    np.testing.assert_array_equal(_run("MAX", [1.0, np.inf, -np.inf], full), [np.inf])
    np.testing.assert_array_equal(_run("MIN", [1.0, np.inf, -np.inf], full), [1.0])


def test_candidate_values():
    """exposure(): the candidates of an entry with exposed elements are the feature after
    moving every subset of the exposed elements across the threshold."""
    q = (-1.0, 0.0, 1.0)
    # elements 2 and 5 sit on the threshold 0 (1e-17 off it); element 0 is never exposed
    row = np.array([[0.0, 2.0, 1e-17, 3.0, -1.0, -1e-17, 4.0]])
    want = {
        # band (0, inf]: in {1, 2, 3, 6}; flipping 2 (out) and / or 5 (in)
        "MAX": [4.0, 4.0, 4.0, 4.0],
        "MIN": [1e-17, 2.0, -1e-17, -1e-17],
        "XPI": [3.0, (1 + 3 + 6) / 3, (1 + 2 + 3 + 5 + 6) / 5, (1 + 3 + 5 + 6) / 4],
        "LPI": [3.0, 1.0, 3.0, 2.0],
        "MPI": [(2 + 1e-17 + 3 + 4) / 4, 3.0, (2 + 1e-17 + 3 - 1e-17 + 4) / 5, (2 + 3 - 1e-17 + 4) / 4],
    }
    for kind, cands in want.items():
        sv = orc.SieveOracle(kind, q=q, inc=0)
        got = {}
        expo = sv.exposure(row, rel=1e-10, candidates=got)
        assert expo.tolist() == [[2, 2]], kind
        assert sorted(got) == [(0, 0), (0, 1)], kind
        np.testing.assert_allclose(got[(0, 1)], cands, rtol=1e-15, atol=0, err_msg=kind)
        # the unflipped candidate is the feature itself
        assert got[(0, 1)][0] == sv.transform(row)[0, 1], kind
    # a count needs no candidates (it moves by at most the number of exposed elements)
    none = {}
    orc.SieveOracle("NPI", q=q, inc=0).exposure(row, candidates=none)
    assert none == {}
    # the older keyword still fills the same dict
    means = {}
    orc.SieveOracle("MPI", q=q, inc=0).exposure(row, means=means)
    assert sorted(means) == [(0, 0), (0, 1)]
    # more than four exposed elements: no candidates (a plateau)
    many = {}
    sv = orc.SieveOracle("MAX", q=q, inc=0)
    sv.exposure(np.array([[1.0] + [0.0] * 5]), candidates=many)
    assert many == {}
    # MAX / MIN of the segment sieves: exposure of the band thresholds only, none for (-inf, inf]
    assert orc.SieveOracle("MAX").exposure(row).tolist() == [[0]]
    # ... and END is never exposed
    assert orc.SieveOracle("END").exposure(row).tolist() == [[0]]
