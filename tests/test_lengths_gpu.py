"""Per-series lengths on the device: row n of ``fruit.transform(X, lengths=lengths)`` against the
per-series call ``fruit.transform(X[n:n+1, :, :lengths[n]])[0]`` of the same fitted fruit.

Inputs are small integers (``integers(-2, 3)``, as in test_implicit_gpu.py): every iterated sum
is then an exact integer in any association, so the comparison is ``assert_array_equal`` on
every column, whatever launch shape the padded batch and the truncated series take.  The tails
are filled with integers from 1000 to 2000, and a second run with other tails must give the same
bits.  Real-valued cases (STD, the weightings, the golden fixture) are held to the project's bar,
``rtol=1e-6, atol=1e-9``, and to exact equality where the column counts.

Short lengths: the per-series call of the parent commit handles series of 1, 2 and 3 elements
for every fruit of this file, so no length class of the issue is dropped.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


def int_input(seed, shape):
    return np.random.default_rng(seed).integers(-2, 3, shape).astype(np.float64)


def spread(classes, N):
    """N lengths in which every class appears."""
    assert len(classes) <= N
    return np.resize(np.asarray(classes, dtype=np.int64), N)


def with_tails(X, lengths, seed):
    """X with everything behind a series' length replaced by integers from 1000 to 2000."""
    Y = X.copy()
    rng = np.random.default_rng(seed)
    for n, L in enumerate(lengths):
        Y[n, :, L:] = rng.integers(1000, 2001, Y[n, :, L:].shape)
    return Y


def per_series(fruit, X, lengths):
    return np.stack([fruit.transform(np.ascontiguousarray(X[n:n + 1, :, :L]))[0]
                     for n, L in enumerate(lengths)])


def launch_sieves(fr):
    S = fr.sieving
    return [S.NPI(), S.NPI(inc=2), S.MPI(cut=[3, -1]), S.XPI(), S.MAX(), S.MIN(cut=[-3, -1]), S.CUR(),
            S.END(), S.PPV(0, True), S.CPV([0, 2], True, segments=True)]


def launch_fruit(fr, weight, D, extra=()):
    fruit = fr.Fruit("ragged")
    fruit.add(fr.preparation.INC)
    fruit.add(fr.ISS(fr.words.of_weight(weight, dim=D), mode=fr.ISSMode.EXTENDED))
    fruit.add(*launch_sieves(fr), *extra)
    return fruit


def check_ragged(fruit, X, lengths, fused=True):
    """The ragged call on two different tails equals the per-series calls, bit for bit; returns
    the ragged features."""
    T = X.shape[2]
    np.random.seed(3)
    fruit.fit(with_tails(X, lengths, 1), lengths=lengths)
    want = per_series(fruit, X, lengths)
    got = fruit.transform(with_tails(X, lengths, 1), lengths=lengths)
    slc = fruit.get_slice()
    pipe = slc._fused(T, ragged=True)
    assert (pipe is not None) == fused
    if fused:
        family = pipe.last_launch()["family"]
        assert family is not None and family.startswith("fused"), family
        assert pipe.jit_loaded() == 0          # (per-series cuts: the generic instances)
    again = fruit.transform(with_tails(X, lengths, 2), lengths=lengths)
    np.testing.assert_array_equal(got, again)
    labels = [fruit.label(i) for i in range(fruit.nfeatures())]
    for c, lb in enumerate(labels):
        np.testing.assert_array_equal(got[:, c], want[:, c], err_msg=f"{lb} lengths={lengths.tolist()}")
    return got


LAUNCH_SHAPES = {
    "wave_per_series": ((12, 2, 200), 2, [1, 2, 3, 5, 64, 65, 128, 129, 199, 200], None),
    "one_chunk": ((12, 3, 700), 2, [4, 255, 256, 257, 511, 512, 513, 699, 700], None),
    "several_chunks": ((12, 2, 2100), 2, [4, 1023, 1024, 1025, 2047, 2048, 2049, 2100], "groups=1"),
    "window_flushes": ((8, 2, 700), 4, [4, 255, 256, 257, 511, 512, 699, 700], None),
    "plan_over_128_nodes": ((4, 3, 1300), 4, [5, 1024, 1025, 1300], None),
}


@pytest.mark.parametrize("case", LAUNCH_SHAPES, ids=list(LAUNCH_SHAPES))
def test_launch_shapes(fr, monkeypatch, case):
    shape, weight, classes, debug = LAUNCH_SHAPES[case]
    if debug:
        monkeypatch.setenv("FRUITS_HIP_DEBUG", debug)
    X = int_input(sum(shape), shape)
    lengths = spread(classes, shape[0])
    fruit = launch_fruit(fr, weight, shape[1])
    got = check_ragged(fruit, X, lengths)
    pipe = fruit.get_slice()._fused(shape[2], ragged=True)
    if case == "plan_over_128_nodes":
        assert pipe.plan.nodes > 128
    if case == "wave_per_series":
        assert pipe.last_launch()["family"] == "fused_packed"
    # PPV's shares are shares of the series' own length
    ppv = [i for i in range(fruit.nfeatures()) if fruit.label(i).split("|")[-1].strip().startswith("PPV")]
    counts = got[:, ppv] * lengths[:, None]
    assert len(ppv) and (np.abs(counts - np.round(counts)) < 1e-9).all()


@pytest.mark.parametrize("semiring", ["Arctic", "Bayesian"])
@pytest.mark.parametrize("shape,classes", [((12, 2, 200), [1, 2, 3, 5, 64, 65, 128, 129, 199, 200]),
                                           ((9, 2, 700), [4, 255, 256, 257, 511, 512, 513, 699, 700])],
                         ids=["wave_per_series", "one_chunk"])
def test_semirings(fr, semiring, shape, classes):
    words = [fr.words.SimpleWord(s) for s in ("[1]", "[2]", "[1][2]", "[11][2]")]
    fruit = fr.Fruit(semiring)
    fruit.add(fr.ISS(words, mode=fr.ISSMode.EXTENDED, semiring=getattr(fr.semiring, semiring)()))
    fruit.add(*launch_sieves(fr))
    check_ragged(fruit, int_input(11, shape), spread(classes, shape[0]))


@pytest.mark.parametrize("how", ["lpi", "fused_off"])
def test_materialising_path(fr, monkeypatch, how):
    shape = (12, 2, 700)
    lengths = spread([1, 2, 3, 5, 64, 255, 256, 257, 512, 513, 699, 700], shape[0])
    if how == "fused_off":
        monkeypatch.setenv("FRUITS_AMD_FUSED", "0")
    fruit = launch_fruit(fr, 2, shape[1], extra=[fr.sieving.LPI()] if how == "lpi" else [])
    check_ragged(fruit, int_input(23, shape), lengths, fused=False)


# ---------------------------------------------------------------- STD
STD_LENGTHS = np.array([2, 3, 7, 8, 9, 127, 128, 129, 700])


def real_input(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape)


@pytest.mark.parametrize("var", [True, False])
def test_std_rows_are_the_truncated_call_bit_for_bit(fr, var):
    """The pairwise-summation block edges of numpy's sum: the statistics of series n are summed
    in numpy's order for ITS length, so the standardised rows are those of the per-series call."""
    from fruits_amd import _native as nat
    X = with_tails(real_input(31, (9, 2, 700)), STD_LENGTHS, 4)
    std = fr.preparation.STD(var=var)
    ld = nat.to_device(STD_LENGTHS.astype(np.int32), dtype=np.int32)
    got = nat.to_host(std._transform_device(nat.to_device(X), lengths_d=ld))
    for n, L in enumerate(STD_LENGTHS):
        want = std.transform(np.ascontiguousarray(X[n:n + 1, :, :L]))[0]
        np.testing.assert_array_equal(got[n, :, :L], want, err_msg=f"L={L}")
        assert (got[n, :, L:] == 0).all()
    # ... and the statistics pre-pass of the fused preparation: END of the word [d] is the sum of
    # a standardised row, MAX / MIN its extreme prefix sums
    fruit = fr.Fruit("std")
    fruit.add(std.copy())
    fruit.add(fr.ISS(fr.words.of_weight(1, dim=2)))
    fruit.add(fr.sieving.END, fr.sieving.MAX, fr.sieving.MIN, fr.sieving.NPI(q=(-1.0, 1.0)))
    fruit.fit(X, lengths=STD_LENGTHS)
    out = fruit.transform(X, lengths=STD_LENGTHS)
    assert fruit.get_slice()._fused(700, ragged=True).raw_dims == 2       # (fused preparation)
    want = per_series(fruit, X, STD_LENGTHS)
    for c in range(out.shape[1]):
        lb = fruit.label(c)
        if "NPI" in lb:
            np.testing.assert_array_equal(out[:, c], STD_LENGTHS.astype(float), err_msg=lb)
            np.testing.assert_array_equal(out[:, c], want[:, c], err_msg=lb)
        else:
            np.testing.assert_allclose(out[:, c], want[:, c], rtol=1e-6, atol=1e-9, err_msg=lb)


def unbounded(fr):
    S = fr.sieving
    return [S.END(), S.MAX(), S.MIN(), S.NPI(q=(-1.0, 1.0))]


def check_real(fruit, X, lengths):
    fruit.fit(X, lengths=lengths)
    out = fruit.transform(X, lengths=lengths)
    want = per_series(fruit, X, lengths)
    np.testing.assert_array_equal(fruit.transform(with_tails(X, lengths, 9), lengths=lengths), out)
    for c in range(out.shape[1]):
        lb = fruit.label(c)
        if "NPI" in lb:      # (every increment is inside (-inf, inf]: the segment length)
            np.testing.assert_array_equal(out[:, c], lengths.astype(float), err_msg=lb)
        np.testing.assert_allclose(out[:, c], want[:, c], rtol=1e-6, atol=1e-9, err_msg=lb)


@pytest.mark.parametrize("fused_prep", ["1", "0"])
def test_std_through_a_fruit(fr, monkeypatch, fused_prep):
    monkeypatch.setenv("FRUITS_AMD_FUSED_PREP", fused_prep)
    X = with_tails(real_input(32, (9, 2, 700)), STD_LENGTHS, 5)
    fruit = fr.Fruit("std")
    fruit.add(fr.preparation.NEW(fr.preparation.INC()), fr.preparation.STD)
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED))
    fruit.add(*unbounded(fr))
    check_real(fruit, X, STD_LENGTHS)


@pytest.mark.parametrize("weighting", ["Indices", "Plateaus"])
@pytest.mark.parametrize("semiring", ["Reals", "Arctic"])
def test_weighted(fr, weighting, semiring):
    W = fr.iss.weighting
    lengths = spread([4, 9, 64, 255, 256, 257, 512, 699, 700], 9)
    X = with_tails(real_input(33, (9, 2, 700)), lengths, 6)
    fruit = fr.Fruit(weighting)
    fruit.add(fr.preparation.INC)
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED,
                     semiring=getattr(fr.semiring, semiring)(),
                     weighting=W.Indices() if weighting == "Indices" else W.Plateaus(4)))
    fruit.add(*unbounded(fr))
    check_real(fruit, X, lengths)


# ---------------------------------------------------------------- fit
def fitted_fruit(fr, sample_size, extra=()):
    S = fr.sieving
    fruit = fr.Fruit("fit")
    fruit.add(fr.preparation.INC)
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED))
    fruit.add(S.NPI(q=(0.2, 0.7)), S.MPI(q=(0.1, 0.5, 0.9), inc=2), S.MAX(q=(0.3, 1.0)), S.CUR(q=(0.25, 0.75)),
              S.INC(S.NPI(q=(0.4, 1.0))), S.END(), *extra)
    fruit.get_slice().fit_sample_size = sample_size
    return fruit


def thresholds(fruit):
    """Every fitted threshold row of the slice, in (iterated sum, sieve) order."""
    rows = []
    for fitted in fruit.get_slice()._sieves_extended:
        for sv in fitted:
            leaf = sv._sieve if hasattr(sv, "_sieve") else sv
            if hasattr(leaf, "_q_c_input"):                  # PPV / CPV
                rows.append(np.asarray(leaf._q, dtype=np.float64))
            elif sv.requires_fitting:
                rows.append(np.asarray(leaf._quantiles, dtype=np.float64))
    return rows


def _state_pos_after(fit):
    np.random.seed(5)
    fit()
    return np.random.get_state()[2]


@pytest.mark.parametrize("sample", ["default", "one_length"])
def test_fit_truncates_a_sample_of_one_length(fr, sample):
    """The draws are the dense fit's; the sample - one series by default, or series that all have
    one length - is truncated to its length and fitted as the ordinary batch it is: the
    thresholds are those of a fresh fruit fitted on the truncated sample alone."""
    N, T = 10, 300
    X = real_input(41, (N, 2, T))
    extra = [fr.sieving.PPV([0.3, 0.6]), fr.sieving.CPV(0.5)]
    if sample == "default":
        lengths, size = spread([7, 64, 129, 300, 255], N), 1
        np.random.seed(5)
        n = np.random.randint(0, N)
        picked = np.arange(n, n + 1)
    else:
        lengths, size = np.full(N, 130), 1.0
        picked = np.arange(N)
    L = int(lengths[picked[0]])
    ragged, dense, alone = (fitted_fruit(fr, size, extra) for _ in range(3))
    pos = _state_pos_after(lambda: ragged.fit(with_tails(X, lengths, 8), lengths=lengths))
    assert pos == _state_pos_after(lambda: dense.fit(X))             # the same draws as without lengths
    _state_pos_after(lambda: alone.fit(np.ascontiguousarray(X[picked, :, :L])))
    a, b = thresholds(ragged), thresholds(alone)
    assert len(a) == len(b) > 0
    for qa, qb in zip(a, b):
        np.testing.assert_array_equal(qa, qb)
    if L != T:
        assert any(not np.array_equal(qa, qd) for qa, qd in zip(a, thresholds(dense)))


def test_fit_on_unequal_lengths_takes_quantiles_of_the_valid_parts(fr):
    """fit_sample_size = 1.0 on series of unequal lengths: every threshold is np.quantile over the
    concatenated valid parts of the pre-transformed rows.  Integer inputs: the iterated sums of
    the padded sample and of the truncated series are the same numbers."""
    N, T = 6, 300
    X = int_input(42, (N, 2, T))
    lengths = np.array([5, 64, 129, 300, 255, 17])
    fruit, dense = fitted_fruit(fr, 1.0), fitted_fruit(fr, 1.0)
    pos = _state_pos_after(lambda: fruit.fit(with_tails(X, lengths, 10), lengths=lengths))
    assert pos == _state_pos_after(lambda: dense.fit(X))
    slc = fruit.get_slice()
    iss = slc.get_iss()[0]
    inc = fr.preparation.INC()
    sums = [iss.transform(inc.transform(np.ascontiguousarray(X[n:n + 1, :, :L])))
            for n, L in enumerate(lengths)]                             # (K, 1, L_n) each
    assert len(slc._sieves_extended) == sums[0].shape[0]
    checked = 0
    for k, fitted in enumerate(slc._sieves_extended):
        for sv in fitted:
            if not sv.requires_fitting:
                continue
            wrapped = hasattr(sv, "_sieve")
            leaf = sv._sieve if wrapped else sv
            order = leaf._fit_inc + (1 if wrapped else 0)
            valid = np.concatenate([_increments(s[k, 0], order) for s in sums])
            want = np.sort([np.inf if q == 1.0 else (-np.inf if q == -1.0 else
                                                     (0.0 if q == 0 else np.quantile(valid, q)))
                            for q in leaf._q])
            np.testing.assert_array_equal(leaf._quantiles, want, err_msg=f"{sv} row {k}")
            checked += 1
    assert checked == 5 * len(slc._sieves_extended)
    # the fitted fruit transforms the ragged batch like the truncated series
    out = fruit.transform(with_tails(X, lengths, 11), lengths=lengths)
    np.testing.assert_array_equal(out, per_series(fruit, X, lengths))


def _increments(row, inc):
    """The inc-times differenced row, zero-padded at the front each time (fruits/cache.py:8-13)."""
    out = row
    for _ in range(inc):
        out = np.concatenate([[0.0], np.diff(out)])
    return out


def test_fit_on_unequal_lengths_refuses_ppv(fr):
    X = real_input(43, (6, 2, 100))
    lengths = np.array([5, 64, 100, 100, 55, 17])
    for sv in (fr.sieving.PPV(0.5), fr.sieving.CPV([0.2, 0.8])):
        fruit = fitted_fruit(fr, 1.0, [sv])
        with pytest.raises(NotImplementedError, match=type(sv).__name__):
            fruit.fit(X, lengths=lengths)


# ---------------------------------------------------------------- dense identity
def test_full_lengths_are_the_dense_call(fr):
    shape = (16, 3, 700)
    X = int_input(7, shape)
    fruit = launch_fruit(fr, 2, 3)
    np.random.seed(1)
    fruit.fit(X)
    dense = fruit.transform(X)
    slc = fruit.get_slice()
    pipe = slc._fused(700)
    assert pipe is not None
    full = fruit.transform(X, lengths=np.full(16, 700))
    np.testing.assert_array_equal(full, dense)
    assert list(slc._fused_cache) == [700] and slc._fused(700) is pipe
    ragged = fruit.transform(X, lengths=spread([700, 699], 16))
    assert slc._fused(700) is pipe and slc._fused(700, ragged=True) is not pipe
    np.testing.assert_array_equal(ragged[::2], dense[::2])             # (the series of 700)
    assert not np.array_equal(ragged[1::2], dense[1::2])
    np.testing.assert_array_equal(fruit.transform(X), dense)           # (the dense entry is untouched)
    refit = launch_fruit(fr, 2, 3)
    np.random.seed(1)
    refit.fit(X, lengths=np.full(16, 700))
    np.testing.assert_array_equal(refit.transform(X), dense)


def test_end_cut_beyond_a_short_series_raises(fr):
    X = int_input(8, (4, 2, 300))
    for sieves in ([fr.sieving.END(cut=10), fr.sieving.NPI()],
                   [fr.sieving.END(cut=10), fr.sieving.LPI()]):            # fused; materialising
        fruit = fr.Fruit("end")
        fruit.add(fr.ISS(fr.words.of_weight(1, dim=2)))
        fruit.add(*sieves)
        fruit.fit(X)
        with pytest.raises(IndexError, match="out of bounds"):
            fruit.transform(np.ascontiguousarray(X[1:2, :, :9]))
        with pytest.raises(IndexError, match="out of bounds"):
            fruit.transform(X, lengths=np.array([300, 9, 10, 11]))
        fruit.transform(X, lengths=np.array([300, 10, 10, 11]))


# ---------------------------------------------------------------- golden
def build_fruit(fr, spec):
    """The fruit a specification of tests/golden/make_golden_ragged.py describes."""
    fruit = fr.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fruit.cut()
        for p in sl.get("preps", []):
            cls = getattr(fr.preparation, p["kind"])
            fruit.add(cls(getattr(fr.preparation, p["inner"])()) if "inner" in p else cls(**p.get("kw", {})))
        for i in sl["iss"]:
            weighting = getattr(fr.iss.weighting, i["weighting"])() if "weighting" in i else None
            fruit.add(fr.ISS([fr.words.SimpleWord(s) for s in i["words"]],
                             mode=getattr(fr.ISSMode, i["mode"]),
                             semiring=getattr(fr.semiring, i.get("semiring", "Reals"))(),
                             weighting=weighting))
        for s in sl["sieves"]:
            kw = {k: (tuple(v) if k == "q" else v) for k, v in s["kw"].items()}
            fruit.add(getattr(fr.sieving, s["kind"])(**kw))
        fruit.get_slice().fit_sample_size = 1.0
    return fruit


with open(os.path.join(HERE, "golden", "golden_ragged.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.mark.parametrize("case", GOLDEN["fruit"], ids=lambda c: c["name"])
def test_golden(fr, case):
    """The reference, series by series on the truncated series after one seeded fit on the dense
    batch.  The fixture's generator kept every element of a counting sieve's row more than 1e-10
    from the thresholds, so the counting columns are exactly equal."""
    arrays = np.load(os.path.join(HERE, "golden", "golden_ragged.npz"))
    X, lengths, want = arrays["X"], arrays["lengths"], arrays[case["out"]]
    fruit = build_fruit(fr, case["spec"])
    np.random.seed(case["seed"])
    fruit.fit(X)
    out = fruit.transform(X, lengths=lengths)
    assert out.shape == want.shape
    for c, lb in enumerate(case["labels"]):
        assert fruit.label(c) == lb
        sieve = lb.split("|")[-1].strip()
        if sieve.startswith(tuple(GOLDEN["counting"])):
            np.testing.assert_array_equal(out[:, c], want[:, c], err_msg=lb)
        else:
            np.testing.assert_allclose(out[:, c], want[:, c], rtol=1e-6, atol=1e-9, err_msg=lb)


# ---------------------------------------------------------------- raw ABI
def test_raw_abi(fr):
    """One call of each new entry through fr_malloc and raw pointers (no torch tensors)."""
    import implicit_ref as iref
    from fruits_amd import _native as nat
    L = nat.lib()
    N, D, T = 5, 2, 130
    X = np.random.default_rng(9).integers(-2, 3, (N, D, T)).astype(np.float64)
    lengths = np.array([1, 7, 64, 129, 130], dtype=np.int32)
    q = np.array([-1.0, 0.0, 2.0])
    bufs = {}

    def dev(name, arr):
        ptr = C.c_void_p()
        assert L.fr_malloc(C.byref(ptr), C.c_int64(arr.nbytes)) == 0
        assert L.fr_memcpy_h2d(ptr, arr.ctypes.data_as(C.c_void_p), C.c_int64(arr.nbytes), None) == 0
        bufs[name] = ptr
        return ptr

    def host(ptr, arr):
        assert L.fr_memcpy_d2h(arr.ctypes.data_as(C.c_void_p), ptr, C.c_int64(arr.nbytes), None) == 0
        assert L.fr_stream_sync(None) == 0
        return arr

    try:
        dX, dL, dQ = dev("x", X), dev("l", lengths), dev("q", q)
        # fr_sieve_implicit_lengths on dimension 0 of every series (row stride D * T)
        out = np.full((N, 2), -1.0)
        dO = dev("o", out)
        L.fr_sieve_implicit_lengths.restype = C.c_int
        rc = L.fr_sieve_implicit_lengths(C.c_int32(nat.FR_SIEVE_CPV), dX, C.c_int64(N), C.c_int64(T),
                                         C.c_int64(D * T), dL, dQ, C.c_int32(3), C.c_int32(1), dO,
                                         C.c_int64(2), None)
        assert rc == 0, nat.last_error()
        host(dO, out)
        for n, Ln in enumerate(lengths):
            with np.errstate(invalid="ignore"):
                np.testing.assert_array_equal(out[n], iref.cpv(X[n, :1, :Ln], q, True)[0])
        # fr_standardize_lengths
        Z = np.full((N, D, T), -1.0)
        dZ = dev("z", Z)
        rc = L.fr_standardize_lengths(dX, C.c_int64(N), C.c_int64(D), C.c_int64(T), dL, C.c_int32(1),
                                      C.c_double(1e-5), dZ, None)
        assert rc == 0, nat.last_error()
        host(dZ, Z)
        for n, Ln in enumerate(lengths):
            rows = np.ascontiguousarray(X[n, :, :Ln])
            mean = rows.mean(axis=1, keepdims=True)
            want = (rows - mean) / (rows.std(axis=1, keepdims=True) + 1e-5)
            np.testing.assert_array_equal(Z[n, :, :Ln], want)
            assert (Z[n, :, Ln:] == 0).all()
        # fr_pipeline_set_lengths: a PPV with per-series cuts is divided by the series' length,
        # and refuses to run without one
        plan = nat.Plan([np.array([[1, 0]], dtype=np.int32)], [1])
        pipe = nat.Pipeline(plan, [(nat.FR_SIEVE_PPV | nat.FR_SIEVE_SERIES_CUTS, 0, np.array([0, 1]), 1)], T)
        pipe.set_quantiles(np.array([[0.0]]))
        table = np.stack([np.zeros(N, dtype=np.int32), lengths], axis=1).copy()
        dT = dev("t", table)
        feats = np.full((N, 1), -1.0)
        dF = dev("f", feats)
        wb = int(L.fr_pipeline_workspace_bytes(pipe._h, N, 0))
        dW = C.c_void_p()
        assert L.fr_malloc(C.byref(dW), C.c_int64(max(wb, 8))) == 0
        bufs["w"] = dW
        assert L.fr_pipeline_set_series_cuts(pipe._h, dT, C.c_int64(N), C.c_int32(2)) == 0
        run = lambda: L.fr_pipeline_run(pipe._h, dX, C.c_int64(N), C.c_int64(D), C.c_int64(T), None,
                                        C.c_int64(0), dF, C.c_int64(1), dW, C.c_int64(wb), C.c_int32(0),
                                        None)
        assert run() == nat.FR_E_ARG and "fr_pipeline_set_lengths" in nat.last_error()
        assert L.fr_pipeline_set_lengths(pipe._h, dL, C.c_int64(N - 1)) == 0
        assert run() == nat.FR_E_ARG
        assert L.fr_pipeline_set_lengths(pipe._h, dL, C.c_int64(N)) == 0
        assert run() == 0, nat.last_error()
        host(dF, feats)
        for n, Ln in enumerate(lengths):
            assert feats[n, 0] == (np.cumsum(X[n, 0, :Ln]) >= 0).sum() / Ln
        del pipe
    finally:
        for ptr in bufs.values():
            L.fr_free(ptr)
