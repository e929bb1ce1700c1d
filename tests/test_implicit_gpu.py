"""PPV / CPV on the device: the standalone kernel (fr_sieve_implicit) against the numpy
restatement of tests/implicit_ref.py, exactly - the counts are integers and the one division is
correctly rounded on both sides - and the classes against the reference's recorded outputs."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

from fruits_amd.sieving import CPV, PPV

import implicit_ref as iref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_implicit.json")) as _f:
    MANIFEST = json.load(_f)
ARRAYS = np.load(os.path.join(HERE, "golden", "golden_implicit.npz"))
KINDS = {"PPV": PPV, "CPV": CPV}


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


# thresholds ON the data values (small integers in [-2, 2]): `>=` against `>` and `<` against
# `<=` show; the last two lists are unsorted (with `segments`: empty bands)
THRESHOLDS = [
    ([0.0], False), ([-2.0, -1.0, 0.0, 1.0, 2.0, 3.0], False), ([1.0, -1.0, 0.5], False),
    ([-2.0, 0.0, 2.0], True), ([-1.0, 0.0, 1.0, 2.0, np.inf], True), ([-np.inf, 0.0], True),
    ([1.0, -1.0, 0.0, 2.0], True), ([2.0, 0.0, 0.0, 1.0], True),
]


def _standalone(nat, kind, X, q, segments, col=0, width=None):
    t = nat.torch()
    Ad = nat.to_device(X)
    F = iref.nfeatures(q, segments)
    out = t.full((X.shape[0], width or F), -7.0, dtype=t.float64, device=Ad.device)
    nat.sieve_implicit(kind, Ad, nat.to_device(np.asarray(q, dtype=np.float64)), segments, out, col)
    return nat.to_host(out)


@pytest.mark.parametrize("T", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025])
def test_standalone_exact(fr, T):
    from fruits_amd import _native as nat
    rows = iref.edge_rows(T, np.random.default_rng(T))
    for N in (1, 5):
        X = np.ascontiguousarray(rows[:N] if N == 1 else rows[[0, 3, 5, 7, 8]])
        for name, kind in (("PPV", nat.FR_SIEVE_PPV), ("CPV", nat.FR_SIEVE_CPV)):
            for q, segments in THRESHOLDS:
                with np.errstate(invalid="ignore"):
                    want = iref.transform(name, X, q, segments)
                got = _standalone(nat, kind, X, q, segments)
                np.testing.assert_array_equal(got, want, err_msg=f"{name} T={T} N={N} q={q} {segments}")
    # every row kind at once, into the middle of a wider feature tensor (the columns around it
    # stay as they were)
    q, segments = THRESHOLDS[4]
    got = _standalone(nat, nat.FR_SIEVE_CPV, rows, q, segments, col=2, width=9)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(got[:, 2:6], iref.cpv(rows, np.asarray(q), True))
    assert (got[:, :2] == -7.0).all() and (got[:, 6:] == -7.0).all()


def test_standalone_strided_rows_and_many_thresholds(fr):
    from fruits_amd import _native as nat
    X = np.random.default_rng(5).integers(-2, 3, (7, 300)).astype(np.float64)
    Ad = nat.to_device(X)[:, 10:211]          # row stride 300, T = 201
    t = nat.torch()
    q = np.linspace(-2.5, 2.5, 256)
    out = t.zeros((7, 256), dtype=t.float64, device=Ad.device)
    nat.sieve_implicit(nat.FR_SIEVE_PPV, Ad, nat.to_device(q), False, out, 0)
    np.testing.assert_array_equal(nat.to_host(out), iref.ppv(X[:, 10:211], q))
    nat.sieve_implicit(nat.FR_SIEVE_CPV, Ad, nat.to_device(q), True, out, 0)
    np.testing.assert_array_equal(nat.to_host(out)[:, :255], iref.cpv(X[:, 10:211], q, True))
    with pytest.raises(ValueError, match="at most 256 features"):
        nat.sieve_implicit(nat.FR_SIEVE_PPV, Ad, nat.to_device(np.zeros(257)), False, out, 0)


@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_golden_sieve(fr, case):
    """fit (the host's numpy procedure, seeded) and transform (the kernel) of the class equal the
    reference's recorded features."""
    sv = KINDS[case["spec"]["kind"]](**case["spec"]["kw"])
    X = ARRAYS[case["x"]]
    np.random.seed(case["seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = sv.fit_transform(X)
    np.testing.assert_array_equal(out, ARRAYS[case["out"]])
    dup = sv.copy()
    with pytest.raises(RuntimeError, match="Missing call of"):
        dup.transform(X)


def test_raw_abi(fr):
    """One call of fr_sieve_implicit through fr_malloc and raw pointers (no torch tensors)."""
    from fruits_amd import _native as nat
    L = nat.lib()
    X = iref.edge_rows(130, np.random.default_rng(9))
    q = np.array([-1.0, 0.0, 2.0])
    N, T = X.shape
    out = np.full((N, 2), -1.0)
    dX, dQ, dO = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for ptr, arr in ((dX, X), (dQ, q), (dO, out)):
        assert L.fr_malloc(C.byref(ptr), C.c_int64(arr.nbytes)) == 0
        assert L.fr_memcpy_h2d(ptr, arr.ctypes.data_as(C.c_void_p), C.c_int64(arr.nbytes), None) == 0
    rc = L.fr_sieve_implicit(C.c_int32(nat.FR_SIEVE_CPV), dX, C.c_int64(N), C.c_int64(T), C.c_int64(T),
                             dQ, C.c_int32(3), C.c_int32(1), dO, C.c_int64(2), None)
    assert rc == 0, nat.last_error()
    assert L.fr_memcpy_d2h(out.ctypes.data_as(C.c_void_p), dO, C.c_int64(out.nbytes), None) == 0
    assert L.fr_stream_sync(None) == 0
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(out, iref.cpv(X, q, True))
    for ptr in (dX, dQ, dO):
        L.fr_free(ptr)


# ---------------------------------------------------------------- fused == standalone, bit for bit
# On small-integer inputs every iterated sum of these plans is an exact integer in any
# association (test_sieves_band.py): the fused walk and the materialising walk see the same
# values, and the epilogue must agree with fr_sieve_implicit bit for bit - the fitted quantiles
# of integer rows are data values, so the closed-below ties are all there.
def int_input(seed, shape):
    return np.random.default_rng(seed).integers(-2, 3, shape).astype(np.float64)


def _sieves(fr):
    S = fr.sieving
    return [PPV(0, True), PPV([0.2, 0.5, 0.9]), PPV([-1, 0, 3], True, segments=True), CPV(0.5),
            CPV([0, 2], True, segments=True), S.NPI(), S.END()]


def _fruit(fr, iss, sieves=None, inc=True):
    def make():
        fruit = fr.Fruit("implicit")
        if inc:
            fruit.add(fr.preparation.INC)
        fruit.add(iss())
        fruit.add(*(sieves() if sieves else _sieves(fr)))
        fruit.get_slice().fit_sample_size = 1.0
        return fruit
    return make


def _fused_pair(fr, monkeypatch, X, make):
    """(fused features, unfused features) of two fruits made by ``make``; the fused one did not
    fall back."""
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("FRUITS_AMD_FUSED", fused)
        fruit = make()
        np.random.seed(1)
        fruit.fit(X)
        slc = fruit.get_slice()
        assert (slc._fused(X.shape[2]) is not None) == (fused == "1")
        outs.append(fruit.transform(X))
        if fused == "1":
            family = slc._fused(X.shape[2]).last_launch()["family"]
            assert family is None or family.startswith("fused"), family     # (None: CosWISS)
            assert X.shape[2] > 256 or family in (None, "fused_packed"), family
    monkeypatch.delenv("FRUITS_AMD_FUSED")
    return outs[0], outs[1]


@pytest.mark.parametrize("shape,weight", [((64, 3, 1024), 2), ((6, 3, 5000), 2), ((8, 2, 200), 2),
                                          ((8, 2, 700), 4)],
                         ids=["one_chunk", "multi_chunk", "packed", "window_flushes"])
def test_fused_equals_standalone(fr, monkeypatch, shape, weight):
    X = int_input(sum(shape), shape)
    make = _fruit(fr, lambda: fr.ISS(fr.words.of_weight(weight, dim=shape[1]), mode=fr.ISSMode.EXTENDED))
    a, b = _fused_pair(fr, monkeypatch, X, make)
    np.testing.assert_array_equal(a, b)
    assert a[:, :8].max() <= 1.0 and a[:, :8].min() >= 0.0 and a[:, :8].sum() > 0    # (shares)
    fruit = make()
    np.random.seed(1)
    fruit.fit(X)
    np.testing.assert_array_equal(fruit.transform(X), a)      # two runs: the same bits


def test_fused_one_group_per_series(fr, monkeypatch):
    """FRUITS_HIP_DEBUG groups=1 on a series of three chunks: the window leaves once per chunk
    and more, the counts add up on the feature row; CPV's carry crosses every chunk boundary."""
    monkeypatch.setenv("FRUITS_HIP_DEBUG", "groups=1")
    X = int_input(17, (4, 2, 2100))
    make = _fruit(fr, lambda: fr.ISS(fr.words.of_weight(4, dim=2), mode=fr.ISSMode.EXTENDED))
    a, b = _fused_pair(fr, monkeypatch, X, make)
    np.testing.assert_array_equal(a, b)


def test_fused_jit_off_against_prepared(fr, monkeypatch):
    X = int_input(6, (32, 3, 512))
    make = _fruit(fr, lambda: fr.ISS(fr.words.of_weight(2, dim=3), mode=fr.ISSMode.EXTENDED))
    monkeypatch.setenv("FRUITS_HIP_JIT", "0")
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    f0 = make()
    np.random.seed(1)
    f0.fit(X)
    a = f0.transform(X)
    assert f0.get_slice()._fused(X.shape[2]) is not None
    monkeypatch.setenv("FRUITS_HIP_JIT", "1")
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "all")
    f1 = make()
    np.random.seed(1)
    f1.fit(X)
    b = f1.transform(X)
    assert f1.get_slice()._fused(X.shape[2]) is not None
    np.testing.assert_array_equal(a, b)
    monkeypatch.setenv("FRUITS_AMD_FUSED", "0")
    f2 = make()
    np.random.seed(1)
    f2.fit(X)
    np.testing.assert_array_equal(f2.transform(X), a)


def test_fused_plan_in_pieces(fr, monkeypatch):
    """of_weight(4, 3): a plan of more than 128 nodes, compiled and run in pieces - on series of
    two time chunks, so that CPV's carry crosses a chunk boundary inside the bodies of a piece."""
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "all")
    # (two feature ops and pieces of at most 32 nodes: seconds of compiler, not half a minute)
    monkeypatch.setenv("FRUITS_HIP_DEBUG", "piece_nodes=32")
    X = int_input(5, (4, 3, 1300))
    make = _fruit(fr, lambda: fr.ISS(fr.words.of_weight(4, dim=3), mode=fr.ISSMode.EXTENDED),
                  lambda: [PPV(0.5), CPV([0, 2], True, segments=True)])
    monkeypatch.setenv("FRUITS_AMD_FUSED", "1")
    fruit = make()
    np.random.seed(1)
    fruit.fit(X)
    a = fruit.transform(X)
    pipe = fruit.get_slice()._fused(X.shape[2])
    assert pipe is not None and pipe.plan.nodes > 128 and pipe.pieces_loaded() > 0
    assert pipe.last_launch()["family"] == "fused_pieces", pipe.last_launch()
    monkeypatch.setenv("FRUITS_AMD_FUSED", "0")
    plain = make()
    np.random.seed(1)
    plain.fit(X)
    np.testing.assert_array_equal(a, plain.transform(X))


def test_fused_arctic_and_coswiss(fr, monkeypatch):
    words = [fr.words.SimpleWord(s) for s in ("[1]", "[2]", "[1][2]", "[11][2]")]
    for shape in ((10, 2, 200), (5, 2, 2500)):          # wave per series; three time chunks
        X = int_input(4, shape)
        arctic = _fruit(fr, lambda: fr.ISS(words, mode=fr.ISSMode.EXTENDED, semiring=fr.semiring.Arctic()),
                        inc=False)
        a, b = _fused_pair(fr, monkeypatch, X, arctic)     # max-plus of integers: exact
        np.testing.assert_array_equal(a, b)
        # CosWISS: the cosine weights make the sums inexact, but the fused and the materialising
        # launch run the same unit (coswiss.h, coswiss_unit) on the same chunks - the same bits,
        # so constant and fitted thresholds alike must agree, ties and all
        cos = _fruit(fr, lambda: fr.CosWISS(freqs=[0.5, 2.0], words=words),
                     lambda: [PPV([0.37, -1.93], True), CPV([-0.61, 0.83, 7.7], True, segments=True),
                              PPV([0.2, 0.7]), CPV(0.5)], inc=False)
        a, b = _fused_pair(fr, monkeypatch, X, cos)
        np.testing.assert_array_equal(a, b)


def test_argmax_falls_back(fr):
    X = np.random.default_rng(9).standard_normal((6, 1, 90))
    fruit = fr.Fruit("am")
    fruit.add(fr.ISS([fr.words.SimpleWord("[1]"), fr.words.SimpleWord("[1][1]")],
                     mode=fr.ISSMode.EXTENDED, semiring=fr.semiring.Arctic(argmax=True)))
    fruit.add(PPV([0.5, 20.0], [False, True]), CPV(3.0, True))
    np.random.seed(2)
    fruit.fit(X)
    slc = fruit.get_slice()
    assert not slc._fusable() and slc._fused(X.shape[2]) is None
    out = fruit.transform(X)
    rows = slc.get_iss()[0].fit_transform(X)               # (K, N, T): values and positions
    want = []
    for r, fitted in zip(rows, slc._sieves_extended):
        want += [iref.ppv(r, np.asarray(fitted[0]._q)), iref.cpv(r, np.asarray(fitted[1]._q))]
    np.testing.assert_array_equal(out, np.concatenate(want, axis=1))
    assert out.shape == (6, len(rows) * 3) and out.max() > 0


# ---------------------------------------------------------------- golden fruits, real-valued
def _make_sieve(fr, spec):
    kw = {k: (tuple(v) if k == "q" else v) for k, v in spec["kw"].items()}
    return getattr(fr.sieving, spec["kind"])(**kw)


def _build(fr, spec):
    fruit = fr.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fruit.cut()
        for p in sl.get("preps", []):
            fruit.add(getattr(fr.preparation, p["kind"])(**p.get("kw", {})))
        for i in sl["iss"]:
            fruit.add(fr.ISS([fr.words.SimpleWord(s) for s in i["words"]],
                             mode=getattr(fr.ISSMode, i["mode"])))
        for s in sl["sieves"]:
            fruit.add(_make_sieve(fr, s))
        fruit.get_slice().fit_sample_size = 1.0
    return fruit


_ORACLE_SUMS = {}


def _oracle_sums(case):
    """The oracle's iterated sums of a golden fruit's slices (computed once per case)."""
    from oracle import ref_numpy as orc
    if case["name"] not in _ORACLE_SUMS:
        X = ARRAYS[case["x"]]
        sums = []
        for sl in case["spec"]["slices"]:
            preps = [{"kind": p["kind"], **p.get("kw", {})} for p in sl.get("preps", [])]
            sums.append(list(orc._iterate_iss(orc._apply_preps(X, preps), sl["iss"], X)))
        _ORACLE_SUMS[case["name"]] = sums
    return _ORACLE_SUMS[case["name"]]


def _exposure(case):
    """(N, F) numbers of elements the oracle sees within 1e-10 of a threshold of the reference's
    fitted PPV / CPV copies; -1 in the columns of other sieves."""
    cols = []
    N = ARRAYS[case["x"]].shape[0]
    for sl, sums, thr in zip(case["spec"]["slices"], _oracle_sums(case), case["thresholds"]):
        for itsum, row in zip(sums, thr):
            for s, key in zip(sl["sieves"], row):
                if key is None:
                    nf = _make_sieve(__import__("fruits_amd"), s).nfeatures()
                    cols.append(np.full((N, nf), -1, dtype=np.int64))
                else:
                    cols.append(iref.exposure(itsum, ARRAYS[key], bool(s["kw"].get("segments", False))))
    return np.concatenate(cols, axis=1)


@pytest.mark.parametrize("case", MANIFEST["fruit"], ids=lambda c: c["name"])
@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
def test_golden_fruit(fr, monkeypatch, case, fused):
    """The reference's tests/core/test_fruit.py fruit with its PPV sieves, fruits with CPV, and
    one whose sieves fit on half of the sample (the host path): labels and summary literally, the
    PPV / CPV entries equal where the oracle sees no element within 1e-10 of a threshold and off
    by at most e / T (2 e / n) where it sees e, at most 10 % of a column's entries exposed."""
    monkeypatch.setenv("FRUITS_AMD_FUSED", fused)
    X = ARRAYS[case["x"]]
    fruit = _build(fr, case["spec"])
    np.random.seed(case["seed"])
    fruit.fit(X)
    out = fruit.transform(X)
    ref = ARRAYS[case["out"]]
    labels = case["labels"]
    assert [fruit.label(i) for i in range(fruit.nfeatures())] == labels
    assert fruit.summary() == case["summary"]
    assert out.shape == ref.shape
    sampled = any(s["kw"].get("sample_size", 1.0) not in (1, 1.0)
                  for sl in case["spec"]["slices"] for s in sl["sieves"])
    if fused == "1":
        for slc in fruit:
            assert slc._fused(X.shape[2]) is not None
            assert (type(slc._sieves_extended).__name__ == "_FittedRows") == (not sampled)
    expo = _exposure(case)
    T = X.shape[2]
    n_even = T + T % 2
    for c, lb in enumerate(labels):
        kind = lb.rsplit(" | ", 1)[-1][:3]
        e = expo[:, c]
        if kind == "PPV":
            d = np.abs(out[:, c] - ref[:, c])
            print(lb, "exposed", int((e > 0).sum()), "max |d| T", float(d.max() * T))
            assert (e > 0).mean() <= 0.10, (lb, e)
            assert (d <= e / T * (1 + 1e-12)).all(), (lb, out[:, c], ref[:, c], e)
            assert (out[:, c] == ref[:, c])[e == 0].all(), (lb, out[:, c], ref[:, c])
        elif kind == "CPV":
            d = np.abs(out[:, c] - ref[:, c])
            print(lb, "exposed", int((e > 0).sum()), "max |d| n / 2", float(d.max() * n_even / 2))
            assert (e > 0).mean() <= 0.10, (lb, e)
            assert (d <= 2 * e / n_even * (1 + 1e-12)).all(), (lb, out[:, c], ref[:, c], e)
            assert (out[:, c] == ref[:, c])[e == 0].all(), (lb, out[:, c], ref[:, c])
        elif kind == "NPI":
            # (the project's bar for counts next to a fitted threshold, test_sieves_band.py)
            assert (out[:, c] != ref[:, c]).mean() <= 0.1, lb
        else:
            np.testing.assert_allclose(out[:, c], ref[:, c], rtol=1e-6, atol=1e-9, err_msg=lb)


# ---------------------------------------------------------------- the device-side fit
@pytest.mark.parametrize("case", MANIFEST["fruit"], ids=lambda c: c["name"])
def test_device_fit_draws_and_thresholds(fr, monkeypatch, case):
    """After a seeded Fruit.fit on the device numpy's global generator is where the host path
    (FRUITS_AMD_DEVICE_FIT=0) and the reference leave it - one slice and two, PPV mixed with NPI -
    and the thresholds are the host path's bit for bit (the bound of
    test_select_gpu.py::test_fit_with_time_split_equals_host_fit) and the reference's to 1e-13 of
    the magnitude of the rows (test_hip_parity.py, fit_parity)."""
    X = ARRAYS[case["x"]]
    fitted, states = [], []
    for flag in ("1", "0"):
        monkeypatch.setenv("FRUITS_AMD_DEVICE_FIT", flag)
        fruit = _build(fr, case["spec"])
        np.random.seed(case["seed"])
        fruit.fit(X)
        states.append(np.random.get_state())
        fitted.append(fruit)
    sampled = case["name"] == "ppv_sampled"
    for slc in fitted[0]:
        assert (type(slc._sieves_extended).__name__ == "_FittedRows") == (not sampled)
    for st in states:
        np.testing.assert_array_equal(st[1], ARRAYS[case["state_key"]])
        assert int(st[2]) == case["state_pos"]
    sums = _oracle_sums(case)
    for si, (dev, host) in enumerate(zip(fitted[0], fitted[1])):
        assert len(dev._sieves_extended) == len(host._sieves_extended) == len(sums[si])
        for i, (drow, hrow) in enumerate(zip(dev._sieves_extended, host._sieves_extended)):
            scale = np.abs(sums[si][i]).max()
            for j, (d, h) in enumerate(zip(drow, hrow)):
                if not hasattr(d, "_quantiles"):
                    continue
                np.testing.assert_array_equal(np.asarray(d._quantiles), np.asarray(h._quantiles))
                key = case["thresholds"][si][i][j]
                if key is not None:
                    gold = ARRAYS[key]
                    assert np.abs(np.asarray(d._q) - gold).max() <= 1e-13 * scale, (si, i, j, d._q, gold)
