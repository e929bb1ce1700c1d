"""CUR / AVG / STD (fruits/sieving/segment.py:228-358) and the sieve wrappers INC / INT
(fruits/sieving/wrapper.py): the class surface against the reference's
(tests/golden/golden_curvature.json, make_golden_curvature.py), the standalone kernel (fr_sieve,
FR_SIEVE_CUR) against a numpy restatement, and the fused epilogue against the reference's whole
fruits and against the materialising path."""
import json
import os

import numpy as np
import pytest

from fruits_amd import sieving
from fruits_amd.sieving import AVG, CUR, END, INC, INT, LPI, MAX, MIN, MPI, NPI, STD, XPI

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_curvature.json")) as _f:
    MANIFEST = json.load(_f)
ARRAYS = np.load(os.path.join(HERE, "golden", "golden_curvature.npz"))


def make_sieve(spec):
    kw = {k: (tuple(v) if k == "q" else v) for k, v in spec["kw"].items()}
    cls = getattr(sieving, spec["kind"])
    if "sieve" in spec:
        return cls(make_sieve(spec["sieve"]), **kw)
    return cls(**kw)


def leaf_kind(spec):
    while "sieve" in spec:
        spec = spec["sieve"]
    return spec["kind"]


def np_cur(X, cuts, q, inc=2):
    """numpy restatement of FR_SIEVE_CUR on (N, T) rows with (N, C+1) sorted cut rows and sorted
    thresholds q: the sum of the squares of the in-band elements of the ``inc`` times differenced
    (zero-padded) row, per segment and band; 0 for an empty one."""
    D = X.copy()
    for _ in range(inc):
        D = np.concatenate([np.zeros((D.shape[0], 1)), D[:, 1:] - D[:, :-1]], axis=1)
    N, Q = D.shape[0], len(q) - 1
    out = np.zeros((N, (cuts.shape[1] - 1) * Q))
    for n in range(N):
        for j in range(cuts.shape[1] - 1):
            seg = D[n, cuts[n, j]:cuts[n, j + 1]]
            for k in range(Q):
                out[n, j * Q + k] = np.sum(seg[(q[k] < seg) & (seg <= q[k + 1])] ** 2)
    return out


def _quantiles(case):
    return np.array([np.inf if v == "inf" else (-np.inf if v == "-inf" else v)
                     for v in case["quantiles"]])


# ---------------------------------------------------------------- class surface (no device)
@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_surface(case):
    sv = make_sieve(case["spec"])
    assert [sv.label(i) for i in range(sv.nfeatures())] == case["labels"]
    assert str(sv) == case["str"]
    assert sv.summary() == case["summary"]
    assert sv.nfeatures() == case["nfeatures"]
    assert sv.requires_fitting == case["requires_fitting"]
    dup = sv.copy()
    assert type(dup) is type(sv) and str(dup) == case["copy_str"]
    if isinstance(sv, (INC, INT)):
        assert dup._sieve is not sv._sieve


def test_labels_literal():
    assert CUR().label(0) == "CUR!-1![-1.0, 1.0]"
    assert AVG(cut=[3, 0.5]).label(1) == "AVG!0.5![-1.0, 1.0]"
    assert STD(q=(0.5, 1.0)).label(0) == "STD!-1![0.5, 1.0]"
    assert INC(NPI()).label(0) == "INC of NPI[inc=1]!-1![0.0, 1.0]"
    assert INT(MAX(cut=[3, -1])).label(1) == "INT of MAX!-1![-1.0, 1.0]"
    assert INC(INT(NPI())).label(0) == "INC of INT of NPI[inc=1]!-1![0.0, 1.0]"
    assert str(INC(MAX(), depth=2, shift=3)) == "INC(MAX((-1,), (-1.0, 1.0)), 2, 3)"
    assert str(INT(CUR())) == "INT(CUR((-1,), (-1.0, 1.0)))"
    assert CUR().summary() == "CUR -> 1:\n   > -1"
    assert INC(CUR()).summary() == "INC>CUR -> 1:\n   > -1"
    assert INT(INC(STD(cut=[4, -1]))).summary() == "INT>INC>STD -> 2:\n   > 4\n   > -1"


def test_exports():
    assert sorted(sieving.wrapper.__all__) == ["INC", "INT"]
    assert {"CUR", "AVG", "STD"} <= set(sieving.segment.__all__)
    import fruits_amd
    assert fruits_amd.preparation.INC is not sieving.INC


def test_orders_of_fit_and_transform():
    # the kernel differences twice; fit takes its quantiles of the row itself (segment.py:66-75)
    for cls in (CUR, AVG, STD):
        assert cls()._inc == 2 and cls()._fit_inc == 0
        assert cls(q=(0.25, 1.0))._quantile_requests(11) == NPI(q=(0.25, 1.0))._quantile_requests(11)
    # ... and what the existing sieves do is what they did
    assert (MAX()._inc, MAX()._fit_inc) == (0, 0)
    assert (NPI(inc=3)._inc, NPI(inc=3)._fit_inc) == (3, 3)
    X = np.random.default_rng(0).standard_normal((4, 30))
    sv = CUR(q=(0.3, 1.0))
    sv._fit(X)
    np.testing.assert_array_equal(sv._quantiles, [np.quantile(X, 0.3), np.inf])


def test_reduced_orders():
    from fruits_amd import _native as nat

    def red(sv):
        form = sv._reduced()
        return None if form is None else form[1:]
    assert red(CUR()) == (nat.FR_SIEVE_CUR, 2, 0)
    assert red(INC(NPI())) == (nat.FR_SIEVE_NPI, 2, 2)
    assert red(INC(NPI(), depth=5)) == (nat.FR_SIEVE_NPI, 2, 2)      # any depth >= 1 is one
    assert red(INC(NPI(), depth=0)) == (nat.FR_SIEVE_NPI, 1, 1)
    assert red(INC(CUR())) == (nat.FR_SIEVE_CUR, 3, 1)
    assert red(INC(INC(MPI(inc=0)))) == (nat.FR_SIEVE_MPI, 2, 2)
    assert red(INT(MPI(inc=0))) == (nat.FR_SIEVE_MPI, -1, -1)
    assert red(INT(INT(MAX()))) == (nat.FR_SIEVE_MAX, -2, -2)
    assert red(INT(NPI(inc=-7))) == (nat.FR_SIEVE_NPI, -8, -8)
    for sv in (INT(NPI()), INT(CUR()), INC(INT(NPI(inc=0))), INC(NPI(inc=-1)),
               INC(NPI(), shift=3), INC(END()), INC(END(), depth=0), INT(LPI(inc=0)),
               INC(NPI(inc=8)), INT(NPI(inc=-8)), INC(MAX(cut=[0.5, -1]))):
        assert red(sv) is None, str(sv)
    inner = NPI(q=(0.5, 1.0))
    assert INC(inner)._reduced()[0] is inner


def _slice(sieves, argmax=False, semiring=None):
    import fruits_amd as fr
    fruit = fr.Fruit("s")
    semiring = semiring or (fr.semiring.Arctic(argmax=True) if argmax else fr.semiring.Reals())
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED, semiring=semiring))
    fruit.add(*sieves)
    return fruit.get_slice()


def test_fusable(monkeypatch):
    monkeypatch.delenv("FRUITS_AMD_FUSED", raising=False)
    assert _slice([CUR(), AVG(q=(0.5, 1.0)), STD(cut=[0.5, -1]), END()])._fusable()
    assert _slice([INC(NPI()), INC(MPI(), depth=0), INT(NPI(inc=0)), INC(CUR())])._fusable()
    assert _slice([INC(INC(XPI())), INT(INT(MPI(inc=-1)))])._fusable()
    # MAX / MIN at another order: fr_pipeline_create takes inc -8 to 8 for every band sieve
    assert _slice([INT(MAX()), INC(MIN(q=(-1.0, 0.0, 1.0)))])._fusable()
    # mixed signs, another shift, END and LPI inside a wrapper, a reduced order beyond 8
    for sv in (INT(NPI()), INT(CUR()), INC(INT(NPI(inc=0))), INC(NPI(), shift=2),
               INC(MAX(), depth=2, shift=3), INC(END()), INC(END(), depth=0), INC(LPI()),
               INT(LPI(inc=0)), INC(NPI(inc=8)), INT(NPI(inc=-8))):
        assert not _slice([NPI(), sv])._fusable(), str(sv)
    # the inner sieve's float cuts are coquantiles of the wrapped rows
    assert not _slice([INC(NPI(cut=[0.5, -1]))])._fusable()
    # the Arctic argmax kernel forms NPI / MPI / END only
    assert not _slice([CUR()], argmax=True)._fusable()
    assert not _slice([INC(NPI(inc=0))], argmax=True)._fusable()
    monkeypatch.setenv("FRUITS_AMD_FUSED", "0")
    assert not _slice([CUR()])._fusable()


def test_pipeline_specs_of_wrappers():
    from fruits_amd import _native as nat
    from fruits_amd.fruit import FruitSlice
    specs, cut_columns, n_slots = FruitSlice._pipeline_specs(
        [CUR(q=(0.5, 1.0)), INC(CUR(cut=[4, -1])), INT(MPI(inc=0)), STD(cut=[0.5, -1]), END()], 20)
    assert [(s[0], s[1], s[3]) for s in specs] == [
        (nat.FR_SIEVE_CUR, 2, 2), (nat.FR_SIEVE_CUR, 3, 2), (nat.FR_SIEVE_MPI, -1, 2),
        (nat.FR_SIEVE_CUR | nat.FR_SIEVE_SERIES_CUTS, 2, 2), (nat.FR_SIEVE_END, 0, 2)]
    np.testing.assert_array_equal(specs[1][2], [0, 4, 20])
    assert n_slots == 3 and len(cut_columns) == 1


def test_numpy_restatement_matches_reference():
    n = 0
    for case in MANIFEST["sieve"]:
        spec = case["spec"]
        if spec["kind"] not in ("CUR", "AVG", "STD"):
            continue
        if any(isinstance(c, float) for c in np.atleast_1d(spec["kw"].get("cut", -1))):
            continue
        sv = make_sieve(spec)
        X = ARRAYS[case["x"]]
        cuts = np.repeat(sv._int_cut_row(X.shape[1])[None, :], X.shape[0], axis=0)
        np.testing.assert_allclose(np_cur(X, cuts, _quantiles(case)), ARRAYS[case["out"]],
                                   rtol=1e-12, atol=0, err_msg=case["name"])
        n += 1
    assert n >= 60


def test_reference_avg_std_are_cur():
    # what the reference returns under the names AVG / STD is CUR's output, entry for entry
    by_name = {c["name"]: c for c in MANIFEST["sieve"]}
    n = 0
    for name, case in by_name.items():
        if case["spec"]["kind"] == "CUR":
            for other in ("avg", "std"):
                np.testing.assert_array_equal(ARRAYS[by_name[other + name[3:]]["out"]], ARRAYS[case["out"]])
                n += 1
    assert n == 2 * sum(c['spec']['kind'] == 'CUR' for c in MANIFEST['sieve']) > 0


# ---------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


_CUR_OUT = {}     # CUR's device output per (input, arguments): AVG / STD must equal it bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_golden_sieve(fr, case):
    """Every golden case through fit_transform (the materialising path of a sieve on its own).
    CUR / AVG / STD and the sum-valued wrapper cases at rtol 1e-12: the differences are the same
    correctly rounded subtractions as the reference's, and a sum of at most 64 non-negative squares
    in any order, with or without FMA, is within 64 * 2^-53 of the exact one.  Counts, MAX and END:
    exact."""
    spec = case["spec"]
    sv = make_sieve(spec)
    X = ARRAYS[case["x"]]
    out = sv.fit_transform(X)
    ref = ARRAYS[case["out"]]
    assert out.shape == ref.shape
    print(case["name"], "max rel", float(np.max(np.abs(out - ref) / np.maximum(np.abs(ref), 1e-300))))
    if leaf_kind(spec) in ("NPI", "LPI", "MAX", "END"):
        np.testing.assert_array_equal(out, ref)
    else:
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=0)
    if spec["kind"] in ("CUR", "AVG", "STD"):
        key = (case["x"], json.dumps(spec["kw"], sort_keys=True))
        if spec["kind"] != "CUR" and key not in _CUR_OUT:
            _CUR_OUT[key] = make_sieve({**spec, "kind": "CUR"}).fit_transform(X)
        np.testing.assert_array_equal(out, _CUR_OUT.setdefault(key, out))


@pytest.mark.gpu
@pytest.mark.parametrize("inc", [0, 2, 3])
@pytest.mark.parametrize("N", [1, 5])
def test_standalone_cur(fr, N, inc):
    """fr_sieve with FR_SIEVE_CUR against the numpy restatement: T = 1 and 2 are the sizes at which
    the zero padding of the second difference can go wrong, 63 / 64 / 65 the wave, 257 more than a
    workgroup's stride, 1025 several strides; a cut row with an empty segment (one broadcast row
    for N = 1, a row per series for N = 5).  The differences are the same subtractions on both
    sides, so the same elements are in a band; two sums of T non-negative squares in different
    orders are each within T * 2^-53 of the exact sum: rtol T * 2^-52."""
    from fruits_amd import _native as nat
    t = nat.torch()
    q = np.array([-np.inf, -0.5, 0.7, np.inf])
    for T in (1, 2, 3, 63, 64, 65, 257, 1025):
        X = np.random.default_rng(1000 * N + T).standard_normal((N, T)).cumsum(axis=1)
        cuts = np.array([sorted([0, (n + T // 2) % (T + 1), (n + T // 2) % (T + 1), T, (3 * n + T // 3) % (T + 1)])
                         for n in range(N)], dtype=np.int64)
        assert (np.diff(cuts, axis=1) == 0).any()      # (the repeated boundary: an empty segment)
        Ad = nat.to_device(X)
        for table in ((cuts, cuts[:1]) if N > 1 else (cuts,)):      # a row per series, one for all
            out = t.zeros((N, 4 * 3), dtype=t.float64, device=Ad.device)
            nat.sieve(nat.FR_SIEVE_CUR, Ad, inc, nat.to_device(table, dtype=np.int64), nat.to_device(q), out, 0)
            want = np_cur(X, np.repeat(table, N // table.shape[0], axis=0), q, inc)
            got = nat.to_host(out)
            print(f"N={N} inc={inc} T={T} max rel",
                  float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))))
            np.testing.assert_allclose(got, want, rtol=T * 2.0 ** -52, atol=0, err_msg=f"T={T}")


def _build(fr, spec):
    fruit = fr.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fruit.cut()
        for p in sl.get("preps", []):
            fruit.add(getattr(fr.preparation, p["kind"]))
        for i in sl["iss"]:
            ws = [fr.words.SimpleWord(s) for s in i["words"]]
            fruit.add(fr.ISS(ws, mode=getattr(fr.ISSMode, i["mode"]),
                             semiring=getattr(fr.semiring, i.get("semiring", "Reals"))()))
        for s in sl["sieves"]:
            fruit.add(make_sieve(s))
        fruit.get_slice().fit_sample_size = 1.0
    return fruit


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "materialised"])
@pytest.mark.parametrize("case", MANIFEST["fruit"], ids=lambda c: c["name"])
def test_golden_fruit(fr, monkeypatch, case, fused):
    """Both whole fruits against the reference's output, every entry: make_golden_curvature.py
    asserts that no element lies within 1e-9 of the row's magnitude of a fitted threshold, so no
    rounding-level difference moves one across a band."""
    monkeypatch.setenv("FRUITS_AMD_FUSED", fused)
    X = ARRAYS[case["x"]]
    fruit = _build(fr, case["spec"])
    fruit.fit(X)
    out = fruit.transform(X)
    if fused == "1":
        assert fruit.get_slice()._fused(X.shape[2]) is not None
    ref = ARRAYS[case["out"]]
    labels = case["labels"]
    assert [fruit.label(i) for i in range(fruit.nfeatures())] == labels
    assert fruit.summary() == case["summary"]
    assert out.shape == ref.shape
    counts = np.array(["NPI" in lb.rsplit(" | ", 1)[-1] for lb in labels])
    print(case["name"], fused, "counts differing", int((out[:, counts] != ref[:, counts]).sum()),
          "max err", float(np.max(np.abs(out - ref) / (1e-9 / 1e-6 + np.abs(ref)))))
    np.testing.assert_array_equal(out[:, counts], ref[:, counts])
    np.testing.assert_allclose(out, ref, rtol=1e-6, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [7, 64, 300, 1024, 1500, 3000])
def test_fused_against_materialised(fr, monkeypatch, T):
    """CUR in the fused epilogue against fr_iss_run + fr_sieve: the wave-per-series kernels
    (T = 7, 64), one chunk, several chunks and ragged tails; order 3 through INC(CUR()).  A
    threshold of 0 moves nothing measurable when an element flips (it contributes its square)."""
    X = np.random.default_rng(T).standard_normal((5, 2, T))
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("FRUITS_AMD_FUSED", fused)
        fruit = fr.Fruit("cur")
        fruit.add(fr.preparation.INC)
        fruit.add(fr.ISS(fr.words.of_weight(3, dim=2), mode=fr.ISSMode.EXTENDED))
        fruit.add(CUR(), CUR(cut=[T // 3 or 1, -1], q=(-1.0, 0.0, 1.0)), INC(CUR()))
        fruit.fit(X)
        outs.append(fruit.transform(X))
        if fused == "1":
            assert fruit.get_slice()._fused(T) is not None
    a, b = outs
    print(f"T={T} max err", float(np.max(np.abs(a - b) / (1e-9 / 1e-6 + np.abs(b)))))
    assert np.isfinite(b).all() and (b[:, 0] > 0).all()
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-9)


@pytest.mark.gpu
def test_own_kernel_bit_for_bit(fr, monkeypatch):
    """The run-time compiled kernel (the sieves as immediates) against the generic instance, bit
    for bit.  The four waves of a workgroup add their partial sums to the window in whatever order
    they arrive, so two launches of the SAME kernel agree bit for bit only where every partial sum
    is exact: small-integer input, whose iterated sums, differences and squares are integers far
    below 2^53 in any association."""
    T = 512
    X = np.random.default_rng(9).integers(-2, 3, (16, 2, T)).astype(np.float64)

    def make():
        fruit = fr.Fruit("own")
        fruit.add(fr.preparation.INC)
        fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED))
        fruit.add(CUR(), STD(cut=[100, -1], q=(-1.0, 0.0, 1.0)), INC(CUR()), INC(NPI()), END())
        return fruit
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    f0 = make()
    f0.fit(X)
    generic = f0.transform(X)
    assert f0.get_slice()._fused(T).jit_loaded() == 0
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "all")
    f1 = make()
    f1.fit(X)
    own = f1.transform(X)
    if f1.get_slice()._fused(T).jit_loaded() == 0:
        pytest.skip("hipRTC is not installed")
    assert np.abs(generic).max() > 0
    np.testing.assert_array_equal(own, generic)
