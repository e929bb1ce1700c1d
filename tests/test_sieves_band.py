"""MAX / MIN / XPI / LPI (fruits/sieving/segment.py:107-200, increment.py:166-239): the class
surface against the reference's (tests/golden/golden_sieves.json, make_golden_sieves.py), the
standalone kernel (fr_sieve) against the reference's outputs, and the fused epilogue of MAX / MIN
/ XPI against the standalone path bit for bit."""
import json
import os

import numpy as np
import pytest

from fruits_amd.sieving import LPI, MAX, MIN, XPI, END, MPI, NPI
from oracle import ref_numpy as orc

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_sieves.json")) as _f:
    MANIFEST = json.load(_f)
ARRAYS = np.load(os.path.join(HERE, "golden", "golden_sieves.npz"))
KINDS = {"MAX": MAX, "MIN": MIN, "XPI": XPI, "LPI": LPI}


def make_sieve(case):
    kw = dict(case["kw"])
    if "q" in kw:
        kw["q"] = tuple(kw["q"])
    return KINDS[case["kind"]](**kw)


def np_band(kind, X, cuts, q, inc=0):
    """numpy restatement of the four sieves on (N, T) rows with (N, C+1) sorted cut rows and
    sorted thresholds q (an empty band or segment: 0)."""
    A = X.copy()
    for _ in range(max(inc, 0)):
        A = np.concatenate([np.zeros((A.shape[0], 1)), np.diff(A, axis=1)], axis=1)
    for _ in range(max(-inc, 0)):
        A = np.cumsum(A, axis=1)
    N, Q = A.shape[0], len(q) - 1
    out = np.zeros((N, (cuts.shape[1] - 1) * Q))
    for n in range(N):
        for j in range(cuts.shape[1] - 1):
            seg = A[n, cuts[n, j]:cuts[n, j + 1]]
            for k in range(Q):
                m = (q[k] < seg) & (seg <= q[k + 1])
                if not m.any():
                    continue
                if kind == "MAX":
                    v = seg[m].max()
                elif kind == "MIN":
                    v = seg[m].min()
                elif kind == "XPI":
                    v = np.flatnonzero(m).mean()
                else:
                    best = cur = 0
                    for b in m:
                        cur = cur + 1 if b else 0
                        best = max(best, cur)
                    v = float(best)
                out[n, j * Q + k] = v
    return out


# ---------------------------------------------------------------- class surface (no device)
@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_surface(case):
    sv = make_sieve(case)
    assert [sv.label(i) for i in range(sv.nfeatures())] == case["labels"]
    assert str(sv) == case["str"]
    assert sv.summary() == case["summary"]
    assert sv.nfeatures() == case["nfeatures"]
    assert sv.requires_fitting == case["requires_fitting"]
    dup = sv.copy()
    assert type(dup) is type(sv) and str(dup) == case["copy_str"]


def test_labels_literal():
    assert MAX().label(0) == "MAX!-1![-1.0, 1.0]"
    assert MIN(cut=[3, 0.5]).label(1) == "MIN!0.5![-1.0, 1.0]"
    assert XPI().label(0) == "XPI[inc=1]!-1![0.0, 1.0]"
    assert LPI(inc=2, q=(0.5, 1.0)).label(0) == "LPI[inc=2]!-1![0.5, 1.0]"
    assert MAX()._inc == 0 and XPI()._inc == 1


def test_quantile_requests():
    # np.quantile(method="linear") placement, the same for the new kinds as for NPI / MPI
    for cls in (MAX, MIN, XPI, LPI):
        sv = cls(q=(0.25, 0.5, 1.0))
        assert sv._quantile_requests(11) == NPI(q=(0.25, 0.5, 1.0))._quantile_requests(11)
        assert sv._quantile_requests(11)[0] == (0, 2, 3, 0.5)


def _slice(sieves, argmax=False):
    import fruits_amd as fr
    fruit = fr.Fruit("s")
    semiring = fr.semiring.Arctic(argmax=True) if argmax else fr.semiring.Reals()
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED, semiring=semiring))
    fruit.add(*sieves)
    return fruit.get_slice()


def test_fusable(monkeypatch):
    monkeypatch.delenv("FRUITS_AMD_FUSED", raising=False)
    assert _slice([MAX(), MIN(q=(-1.0, 0.5, 1.0)), XPI(inc=-2), END()])._fusable()
    assert _slice([MAX(cut=[0.5, -1]), NPI(), MPI()])._fusable()
    assert not _slice([MAX(), LPI()])._fusable()
    assert not _slice([XPI(inc=9)])._fusable()
    # the Arctic argmax kernel forms NPI / MPI / END only
    assert _slice([NPI(), END()], argmax=True)._fusable()
    assert not _slice([MAX()], argmax=True)._fusable()
    assert not _slice([XPI(inc=1)], argmax=True)._fusable()


def test_numpy_restatement_matches_reference():
    # (the restatement the GPU tests use for the cases where the reference raises)
    for case in MANIFEST["sieve"]:
        if "out" not in case or any(isinstance(c, float) for c in np.atleast_1d(case["kw"].get("cut", -1))):
            continue
        sv = make_sieve(case)
        X = ARRAYS[case["x"]]
        q = np.array([np.inf if v == "inf" else (-np.inf if v == "-inf" else v)
                      for v in case["quantiles"]])
        cuts = np.repeat(sv._int_cut_row(X.shape[1])[None, :], X.shape[0], axis=0)
        got = np_band(case["kind"], X, cuts, q, getattr(sv, "_inc", 0) if case["kind"] in ("XPI", "LPI") else 0)
        np.testing.assert_allclose(got, ARRAYS[case["out"]], rtol=1e-12, atol=0, err_msg=case["name"])


# ---------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


@pytest.mark.gpu
@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_golden_sieve(fr, case):
    sv = make_sieve(case)
    X = ARRAYS[case["x"]]
    out = sv.fit_transform(X)
    if "out" in case:
        np.testing.assert_array_equal(out, ARRAYS[case["out"]])
        return
    # the reference raises (an empty band of a non-empty segment): 0.0 here, the rest as numpy
    assert case["reference_raises"] == "ValueError" and case["kind"] in ("MAX", "MIN")
    cuts = np.repeat(sv._int_cut_row(X.shape[1])[None, :], X.shape[0], axis=0)
    want = np_band(case["kind"], X, cuts, sv._quantiles)
    np.testing.assert_array_equal(out, want)
    assert (out == 0.0).any()


def _build(fr, spec):
    fruit = fr.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fruit.cut()
        for p in sl.get("preps", []):
            fruit.add(getattr(fr.preparation, p["kind"]))
        for i in sl["iss"]:
            ws = [fr.words.SimpleWord(s) for s in i["words"]]
            if i.get("kind") == "CosWISS":
                fruit.add(fr.CosWISS(freqs=i["freqs"], words=ws, exponent=i.get("exponent", 2)))
                continue
            fruit.add(fr.ISS(ws, mode=getattr(fr.ISSMode, i["mode"]),
                             semiring=getattr(fr.semiring, i.get("semiring", "Reals"))()))
        for s in sl["sieves"]:
            kw = {k: (tuple(v) if k == "q" else v) for k, v in s.items() if k != "kind"}
            fruit.add(getattr(fr.sieving, s["kind"])(**kw))
        fruit.get_slice().fit_sample_size = 1.0
    return fruit


@pytest.mark.gpu
@pytest.mark.parametrize("case", MANIFEST["fruit"], ids=lambda c: c["name"])
def test_golden_fruit(fr, case):
    X = ARRAYS[case["x"]]
    fruit = _build(fr, case["spec"])
    fruit.fit(X)
    out = fruit.transform(X)
    ref = ARRAYS[case["out"]]
    assert [fruit.label(i) for i in range(fruit.nfeatures())] == case["labels"]
    assert fruit.summary() == case["summary"]
    assert out.shape == ref.shape
    labels = case["labels"]
    # counting features (NPI, LPI) and positions (XPI): exact outside threshold ties - a value
    # within 1e-10 of a fitted threshold may fall on either side after a re-associated scan
    for c, lb in enumerate(labels):
        if lb.startswith(("NPI", "LPI", "XPI")):
            d = out[:, c] != ref[:, c]
            assert d.mean() <= 0.1, (lb, int(d.sum()))
        else:
            np.testing.assert_allclose(out[:, c], ref[:, c], rtol=1e-6, atol=1e-9, err_msg=lb)
    # ... and entry by entry: where the oracle (fitted like the reference, on the whole input)
    # sees no element within 1e-10 of a threshold, an NPI / LPI / XPI entry equals the
    # reference's, a count differs by no more than the number of exposed elements
    spec = {**case["spec"], "slices": [{**sl, "fit_sample_size": 1.0} for sl in case["spec"]["slices"]]}
    _, expo = orc.fruit_transform_exposure(spec, orc.fruit_fit(spec, X), X, rel=1e-10)
    kinds = np.array([lb.rsplit(" | ", 1)[-1][:3] for lb in labels])
    for c, kind in enumerate(kinds):
        e = expo[:, c]
        if kind in ("NPI", "LPI", "XPI"):
            d = out[:, c] != ref[:, c]
            assert not (d & (e == 0)).any(), (labels[c], out[:, c], ref[:, c], e)
            if kind == "NPI":
                assert np.all(np.abs(out[:, c] - ref[:, c]) <= e), (labels[c], e)


# ---------------------------------------------------------------- fused == standalone, bit for bit
# The fused walk and the materialising walk may round an iterated sum differently in its last
# bit (a re-associated scan).  On small-integer inputs every iterated sum of these plans is an
# exact integer in any association, so both paths see the same values and the sieves must agree
# bit for bit - thresholds, ties and all.
def int_input(seed, shape):
    return np.random.default_rng(seed).integers(-2, 3, shape).astype(np.float64)


def _fused_pair(fr, monkeypatch, X, make, T=None):
    """(fused features, unfused features, fitted fused slice) of two fruits made by ``make``."""
    outs = []
    fused_slice = None
    for fused in ("1", "0"):
        monkeypatch.setenv("FRUITS_AMD_FUSED", fused)
        fruit = make()
        fruit.fit(X)
        outs.append(fruit.transform(X))
        if fused == "1":
            fused_slice = fruit.get_slice()
            assert fused_slice._fused(X.shape[2]) is not None
    monkeypatch.delenv("FRUITS_AMD_FUSED")
    return outs[0], outs[1], fused_slice


def _mmx_fruit(fr, words, sieves=None):
    def make():
        fruit = fr.Fruit("mmx")
        fruit.add(fr.preparation.INC)
        fruit.add(fr.ISS(words, mode=fr.ISSMode.EXTENDED))
        fruit.add(*(sieves() if sieves else
                    [MAX(), MIN(q=(-1.0, 0.5, 1.0), cut=[100, -1]), XPI(q=(0.5, 1.0)),
                     XPI(inc=2, cut=[7, -1]), MAX(q=(0.25, 0.75, 1.0)), END()]))
        fruit.get_slice().fit_sample_size = 1.0
        return fruit
    return make


@pytest.mark.gpu
@pytest.mark.parametrize("shape,weight", [((64, 3, 1024), 2), ((6, 3, 5000), 2), ((8, 2, 700), 4)],
                         ids=["one_chunk", "multi_chunk", "window_flushes"])
def test_fused_equals_unfused(fr, monkeypatch, shape, weight):
    X = int_input(sum(shape), shape)
    make = _mmx_fruit(fr, fr.words.of_weight(weight, dim=shape[1]))
    a, b, _ = _fused_pair(fr, monkeypatch, X, make)
    np.testing.assert_array_equal(a, b)
    fruit = make()
    fruit.fit(X)
    np.testing.assert_array_equal(fruit.transform(X), a)      # two runs: the same bits


@pytest.mark.gpu
def test_fused_window_flushes_across_chunks(fr, monkeypatch):
    """One group per series (FRUITS_HIP_DEBUG groups=1) and 82 words: the features of a unit do
    not fit the LDS window, which then leaves for the feature row once per chunk and more - on
    a series of three chunks onto what earlier chunks left there (feat_flush with add: MAX / MIN
    keys by maximum, sums and counts by addition).  Fused == standalone, bit for bit."""
    monkeypatch.setenv("FRUITS_HIP_DEBUG", "groups=1")
    X = int_input(16, (4, 2, 2100))
    make = _mmx_fruit(fr, fr.words.of_weight(4, dim=2))
    a, b, _ = _fused_pair(fr, monkeypatch, X, make)
    np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_fused_float_cuts(fr, monkeypatch):
    X = int_input(3, (16, 2, 300))
    make = _mmx_fruit(fr, fr.words.of_weight(3, dim=2), lambda: [
        MAX(cut=[0.3, 0.7, -1]), MIN(cut=[0.5, -1], coquantile_norm="L1"),
        XPI(cut=[0.25, 0.5], q=(0.25, 0.75, 1.0)), MIN(cut=[0.3, 0.7, -1])])
    a, b, _ = _fused_pair(fr, monkeypatch, X, make)
    np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_fused_coswiss_and_arctic(fr, monkeypatch):
    X = int_input(4, (10, 2, 200))
    words = [fr.words.SimpleWord(s) for s in ("[1]", "[2]", "[1][2]", "[11][2]")]

    def cos():
        fruit = fr.Fruit("c")
        fruit.add(fr.CosWISS(freqs=[0.5, 2.0], words=words))
        fruit.add(MIN(), XPI(inc=0), MAX(q=(0.5, 1.0)))
        fruit.get_slice().fit_sample_size = 1.0
        return fruit

    def arctic():
        fruit = fr.Fruit("a")
        fruit.add(fr.ISS(words, mode=fr.ISSMode.EXTENDED, semiring=fr.semiring.Arctic()))
        fruit.add(MAX(cut=[0.5, -1]), XPI(q=(0.25, 0.75, 1.0)), MIN(cut=[50, -1]))
        fruit.get_slice().fit_sample_size = 1.0
        return fruit
    a, b, _ = _fused_pair(fr, monkeypatch, X, arctic)     # max-plus of integers: exact
    np.testing.assert_array_equal(a, b)
    # CosWISS: cosine weights - the two walks round differently; a value on a fitted threshold
    # may fall on either side
    a, b, _ = _fused_pair(fr, monkeypatch, X, cos)
    close = np.isclose(a, b, rtol=1e-12, atol=1e-12)
    assert close.mean() >= 0.95, close.mean()
    np.testing.assert_allclose(a[:, 0::3], b[:, 0::3], rtol=1e-12, atol=1e-12)   # MIN, no thresholds


@pytest.mark.gpu
def test_fused_plan_in_pieces(fr, monkeypatch):
    # of_weight(4, 3): a plan beyond the straight-line limit, run in pieces when compiled
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "all")
    X = int_input(5, (8, 3, 256))
    make = _mmx_fruit(fr, fr.words.of_weight(4, dim=3))
    a, b, slc = _fused_pair(fr, monkeypatch, X, make)
    np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_fused_jit_off_against_prepared(fr, monkeypatch):
    X = int_input(6, (32, 3, 512))
    make = _mmx_fruit(fr, fr.words.of_weight(2, dim=3))
    monkeypatch.setenv("FRUITS_HIP_JIT", "0")
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    f0 = make()
    f0.fit(X)
    a = f0.transform(X)
    monkeypatch.setenv("FRUITS_HIP_JIT", "1")
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "all")
    f1 = make()
    f1.fit(X)
    b = f1.transform(X)
    assert f1.get_slice()._fused(X.shape[2]) is not None
    np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------- standalone kernel edge cases
@pytest.mark.gpu
def test_lpi_edges(fr):
    from fruits_amd import _native as nat
    t = nat.torch()
    rng = np.random.default_rng(7)
    cases = [np.ones((3, 1)), np.array([[1.0, 2.0], [-1.0, 3.0], [2.0, -1.0]])]
    # runs across a thread tile (T = 4096: tiles of 16) and a wave boundary (1024 per wave),
    # a run that fills the whole segment
    X = np.where(rng.random((4, 4096)) < 0.9, 1.0, -1.0)
    X[0, :] = 1.0
    X[1, :] = -1.0
    X[1, 1000:1050] = 1.0                     # crosses element 1024 (waves 0 | 1)
    X[2, 10:40] = 1.0                         # crosses tiles of 16
    cases.append(X)
    for A in cases:
        N, T = A.shape
        for inc in (0, 1):
            for cut_row in ([0, T], [0, T // 2, T]):
                cuts = np.repeat(np.array(cut_row)[None, :], N, axis=0)
                q = np.array([0.0, np.inf])
                out = t.zeros((N, len(cut_row) - 1), dtype=t.float64, device="cuda")
                nat.sieve(nat.FR_SIEVE_LPI, nat.to_device(A), inc, nat.to_device(cuts, dtype=np.int64),
                          nat.to_device(q), out, 0)
                np.testing.assert_array_equal(nat.to_host(out), np_band("LPI", A, cuts, q, inc))
    assert LPI(inc=0).fit_transform(cases[2])[0, 0] == 4096.0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["MAX", "MIN", "XPI", "LPI"])
def test_raw_abi_per_series_cuts(fr, kind):
    from fruits_amd import _native as nat
    t = nat.torch()
    rng = np.random.default_rng(8)
    N, T = 9, 777
    A = rng.standard_normal((N, T))
    cuts = np.sort(np.concatenate([np.zeros((N, 1), int), rng.integers(0, T + 1, (N, 3)),
                                   np.full((N, 1), T)], axis=1), axis=1)
    cuts[0, 2] = cuts[0, 1]                    # an empty segment
    q = np.array([-np.inf, -0.5, 0.5, np.inf])
    out = t.zeros((N, 4 * 3), dtype=t.float64, device="cuda")
    code = getattr(nat, f"FR_SIEVE_{kind}")
    nat.sieve(code, nat.to_device(A), 0, nat.to_device(cuts, dtype=np.int64), nat.to_device(q), out, 0)
    np.testing.assert_array_equal(nat.to_host(out), np_band(kind, A, cuts, q))


@pytest.mark.gpu
def test_argmax_falls_back(fr):
    X = np.random.default_rng(9).standard_normal((6, 1, 90))
    fruit = fr.Fruit("am")
    fruit.add(fr.ISS([fr.words.SimpleWord("[1]"), fr.words.SimpleWord("[1][1]")],
                     mode=fr.ISSMode.EXTENDED, semiring=fr.semiring.Arctic(argmax=True)))
    fruit.add(MAX(cut=[40, -1]))
    fruit.fit(X)
    slc = fruit.get_slice()
    assert not slc._fusable() and slc._fused(X.shape[2]) is None
    out = fruit.transform(X)
    rows = slc.get_iss()[0].fit_transform(X)               # (K, N, T): values and positions
    cuts = np.repeat(np.array([[0, 40, 90]]), X.shape[0], axis=0)
    want = np.concatenate([np_band("MAX", r, cuts, np.array([-np.inf, np.inf])) for r in rows], axis=1)
    np.testing.assert_array_equal(out, want)


@pytest.mark.gpu
def test_transform_sharded(fr):
    from fruits_amd import parallel as par
    X = int_input(10, (12, 3, 300))
    fruit = fr.Fruit("sh")
    fruit.add(fr.preparation.INC, fr.ISS(fr.words.of_weight(3, dim=3), mode=fr.ISSMode.EXTENDED))
    fruit.add(MAX(), XPI(q=(0.5, 1.0)), MIN(cut=[0.5, -1]))
    fruit.get_slice().fit_sample_size = 1.0
    fruit.fit(X)
    full = fruit.transform(X)
    np.testing.assert_array_equal(par.transform_sharded(fruit, X, rank=0, world=1), full)


# ---------------------------------------------------------------- exact extreme values
# Small integers (and +-0) times 2^e: every cumulative sum, running maximum and difference of
# these rows is exact in any association - the GPU sees the oracle's values bit for bit, so the
# four sieves must agree with it exactly, thresholds, ties and all - from subnormals (2^-1074)
# over ordinary values to values near overflow (2^900 and sums of thousands of them).
EXPONENTS = [-1074, 0, 900]
EXTREME_T = {300: [100, 150, 150, -1],                 # packed (wave-per-series) kernels
             1100: [1000, 1050, 1050, -1],             # straddles 1024
             2200: [1020, 1030, 2040, 2060, -1]}       # straddles 1024 and 2048


def extreme_rows(T, e, seed, nan=False, inf=False):
    """(8, 1, T): all-negative, all-positive, mixed small integers with many zeros of both
    signs, a row of +-0 only, and walks that cross 0 - scaled by 2^e.  ``nan`` / ``inf``: a NaN
    / a +inf inside the second segment of two rows."""
    rng = np.random.default_rng(abs(seed))
    K = np.zeros((8, T))
    K[0] = -rng.integers(1, 4, T)                       # cumsum all negative: MAX of negatives
    K[1] = rng.integers(1, 4, T)                        # cumsum all positive: MIN of positives
    K[2] = rng.integers(-2, 3, T)
    K[3] = 0.0
    K[4] = rng.choice([-1.0, 1.0], T)                   # a walk that touches 0 often
    K[5] = rng.integers(-3, 4, T)
    K[6] = -rng.integers(0, 3, T)
    K[7] = rng.integers(0, 3, T)
    K[K == 0] *= np.where(rng.random((K == 0).sum()) < 0.5, -1.0, 1.0)  # +0 and -0
    X = np.ldexp(K, e)
    if nan:
        X[2, T - 60] = np.nan
        X[5, T // 2 + 3] = np.nan
    if inf:
        X[1, T - 40] = np.inf
        X[4, T // 2 + 5] = np.inf
    return X[:, None, :]


def _extreme_spec(T, semiring, lpi, only_max=False):
    cut = EXTREME_T[T]
    q3, full, pos = [-1.0, 0.0, 1.0], [-1.0, 1.0], [0.0, 1.0]
    if only_max:
        sieves = [{"kind": "MAX", "cut": cut, "q": q3}, {"kind": "MAX", "cut": cut, "q": full}]
    elif lpi:
        sieves = [{"kind": "LPI", "cut": cut, "q": q3, "inc": 0},
                  {"kind": "LPI", "cut": cut, "q": q3, "inc": 1},
                  {"kind": "LPI", "cut": cut, "q": pos, "inc": 2}, {"kind": "MAX", "cut": cut, "q": q3}]
    else:
        sieves = [{"kind": "MAX", "cut": cut, "q": q3}, {"kind": "MAX", "cut": cut, "q": full},
                  {"kind": "MIN", "cut": cut, "q": q3}, {"kind": "MIN", "cut": cut, "q": pos},
                  {"kind": "XPI", "cut": cut, "q": q3, "inc": 0},
                  {"kind": "XPI", "cut": cut, "q": q3, "inc": 1},
                  {"kind": "XPI", "cut": cut, "q": full, "inc": 2},
                  {"kind": "XPI", "cut": cut, "q": pos, "inc": -1}]
    return {"slices": [{"iss": [{"words": ["[1]"], "mode": "SINGLE", "semiring": semiring}],
                        "sieves": sieves}]}


@pytest.mark.gpu
@pytest.mark.parametrize("T", sorted(EXTREME_T))
@pytest.mark.parametrize("fused", ["1", "0"])
def test_extreme_values_exact(fr, monkeypatch, T, fused):
    monkeypatch.setenv("FRUITS_AMD_FUSED", fused)
    for e in EXPONENTS:
        cases = [(extreme_rows(T, e, T + e), ("Reals", "Arctic"), False),
                 (extreme_rows(T, e, T + e + 1, nan=True), ("Reals",), False),
                 (extreme_rows(T, e, T + e + 2, inf=True), ("Reals", "Arctic"), True)]
        for X, semirings, only_max in cases:
            for semiring in semirings:
                for lpi in ((False,) if only_max else (False, True)):
                    spec = _extreme_spec(T, semiring, lpi, only_max)
                    fruit = _build(fr, spec)
                    fruit.fit(X)
                    runs = [fruit.transform(X)]
                    if fused == "1" and not lpi:
                        # the generic fused walk above, then the pipeline's own compiled kernel
                        # (walk_fused.h: kinds, orders and cuts as immediates)
                        pipe = fruit.get_slice()._fused(T)
                        assert pipe is not None
                        pipe.prepare(X.shape[0])
                        # (series of up to 384 run on the packed wave-per-series kernels, which
                        # have no compiled variant)
                        assert pipe.jit_loaded() > 0 or T <= 384
                        runs.append(fruit.transform(X))
                    want = orc.fruit_transform(spec, orc.fruit_fit(spec, X), X)
                    for got in runs:
                        # (the sign of a zero is not compared: numpy's own MAX of +-0 depends on
                        # the order of the elements)
                        np.testing.assert_array_equal(
                            got, want, err_msg=f"e={e} {semiring} lpi={lpi} nan/inf={only_max}")
                        if only_max:
                            assert (got == np.finfo(np.float64).max).any()     # +inf -> nan_to_num


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["MAX", "MIN", "XPI", "LPI"])
def test_extreme_values_raw_abi(fr, kind):
    """The rows of test_extreme_values_exact (their cumulative sums) through fr_sieve with a cut
    row per series, NaN and +inf included, against the oracle's backends."""
    from fruits_amd import _native as nat
    t = nat.torch()
    q = np.array([-np.inf, 0.0, np.inf])
    for T in sorted(EXTREME_T):
        rng = np.random.default_rng(T)
        for e in EXPONENTS:
            A = np.cumsum(extreme_rows(T, e, T + e, nan=True, inf=kind == "MAX")[:, 0, :], axis=1)
            N = A.shape[0]
            inner = np.sort(rng.integers(0, T + 1, (N, 3)), axis=1)
            inner[:, 1] = np.clip(inner[:, 1], 1000, T) if T > 1024 else inner[:, 1]
            cuts = np.concatenate([np.zeros((N, 1), int), inner, np.full((N, 1), T)], axis=1)
            cuts = np.sort(cuts, axis=1)
            cuts[3, 2] = cuts[3, 1]                    # an empty segment
            for inc in ((0,) if kind in ("MAX", "MIN") else (0, 1, 2)):
                out = t.zeros((N, 4 * 2), dtype=t.float64, device="cuda")
                nat.sieve(getattr(nat, f"FR_SIEVE_{kind}"), nat.to_device(A), inc,
                          nat.to_device(cuts, dtype=np.int64), nat.to_device(q), out, 0)
                want = orc.BACKENDS[kind](orc.pre_transform(A, inc), cuts, q)
                np.testing.assert_array_equal(nat.to_host(out), want, err_msg=f"T={T} e={e} inc={inc}")


# ---------------------------------------------------------------- graph capture, word sharding
@pytest.mark.gpu
def test_fused_band_slice_replays_from_a_hip_graph(fr):
    """A fused MAX / MIN / XPI slice captured into a HIP graph (one stream, no branches) and
    replayed twice into the SAME feature tensor: band_key_finalize_kernel decodes the MAX / MIN
    columns in place, so a column the walk did not rewrite would be decoded twice - both
    replays must reproduce the eager features bit for bit."""
    import torch
    from fruits_amd import _native as nat
    rng = np.random.default_rng(14)
    for T in (100, 1500):
        X = rng.standard_normal((32, 2, T)).cumsum(axis=2) / np.sqrt(T)
        Xd = nat.to_device(X)
        iss = fr.ISS(fr.words.of_weight(3, 2), mode=fr.ISSMode.EXTENDED,
                     weighting=fr.iss.weighting.Indices())
        fruit = fr.Fruit()
        fruit.add(iss.copy(), MAX(q=(-1.0, 0.0, 1.0), cut=[T // 3, -1]), MIN(q=(0.5, 1.0)),
                  XPI(q=(0.25, 0.75, 1.0)), MIN(cut=[T // 2, T // 2, -1]), END)
        fruit.fit(X)
        slc = fruit.get_slice()
        pipe = slc._fused(T)
        assert pipe is not None
        lk = iss.lookup_device(Xd)
        feats = torch.empty((32, pipe.n_features), dtype=torch.float64, device=Xd.device)
        pwork = torch.empty(int(nat.lib().fr_pipeline_workspace_bytes(pipe._h, 32, 1)) + 1,
                            dtype=torch.uint8, device=Xd.device)
        slc._attach(fr.cache.SharedSeedCache(X))
        feager = pipe.run(Xd, lk, work=pwork).clone()
        torch.cuda.synchronize()
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                pipe.run(Xd, lk, feats=feats, work=pwork)
        for replay in range(2):
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(feats, feager), (T, replay)
        # ... and holds decoded values: those of the transform (MAX / MIN / END; the transform
        # may run another build of the walk, whose sums can differ in the last bit)
        labels = [fruit.label(i) for i in range(fruit.nfeatures())]
        vals = np.array([lb.rsplit(" | ", 1)[-1][:3] in ("MAX", "MIN", "END") for lb in labels])
        np.testing.assert_allclose(feager.cpu().numpy()[:, vals], fruit.transform(X)[:, vals],
                                   rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_word_sharded_band_kinds_reassemble(fr, world):
    """The word-sharded pipeline (fruits_amd.parallel) rank after rank on one GPU: a fused MAX /
    MIN / XPI slice (one launch per rank) and an LPI slice (materialising) reassemble to the
    unsharded transform bit for bit."""
    from fruits_amd import parallel as par
    from fruits_amd.cache import SharedSeedCache
    X = np.random.default_rng(15).standard_normal((12, 2, 1100)).cumsum(axis=2) / 30.0
    fruit = fr.Fruit("band-sharded")
    fruit.add(fr.preparation.INC, fr.ISS(fr.words.of_weight(3, dim=2), mode=fr.ISSMode.EXTENDED))
    fruit.add(MAX(q=(-1.0, 0.5, 1.0)), MIN(cut=[300, 300, 1050, -1]), XPI(q=(0.25, 0.75, 1.0), inc=2))
    fruit.get_slice().fit_sample_size = 1.0
    fruit.cut()
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED,
                     semiring=fr.semiring.Arctic()))
    fruit.add(LPI(q=(0.5, 1.0)), MAX(cut=[0.5, -1]), LPI(inc=0, q=(-1.0, 0.0, 1.0)))
    fruit.get_slice().fit_sample_size = 1.0
    np.random.seed(0)
    fruit.fit(X)
    ref = fruit.transform(X)
    col0 = 0
    for slc in fruit:
        iss = slc.get_iss()[0]
        strings = [str(w) for w in iss.words]
        depths = [iss._depth(i) for i in range(len(strings))]
        per_sum = sum(s.nfeatures() for s in slc.get_sieves())
        parts = par.shard_words(strings, depths, world)
        maps = par.column_map(parts, depths, per_sum)
        out = np.zeros((X.shape[0], slc.nfeatures()))
        lpi = any(type(s) is LPI for s in slc.get_sieves())
        for r in range(world):
            cache = SharedSeedCache(X)
            if parts[r] and not lpi:
                assert slc._fused(X.shape[2], indices=parts[r]) is not None
            block = par._device_block(slc, iss, cache.input_device(X), cache, parts[r], depths,
                                      per_sum).cpu().numpy()
            assert block.shape[1] == len(maps[r])
            out[:, maps[r]] = block
        np.testing.assert_array_equal(np.nan_to_num(out), ref[:, col0:col0 + slc.nfeatures()])
        col0 += slc.nfeatures()
    assert col0 == ref.shape[1]
