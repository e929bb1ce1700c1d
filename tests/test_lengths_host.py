"""Per-series lengths on the host: the validation of ``lengths=``, the gate (one
``_supports_lengths`` hook per seed class, asked before anything is launched), the per-series
resolution of integer cuts against a literal loop over ``_int_cut_row(L)``, and the
self-consistency of the fixture tests/golden/golden_ragged.{npz,json}.  No device."""
import json
import os

import numpy as np
import pytest

import fruits_amd as fr
from fruits_amd.lengths import check_lengths, lookup_rows, resolve_cuts, resolve_end_cuts

HERE = os.path.dirname(os.path.abspath(__file__))
P, S, W = fr.preparation, fr.sieving, fr.iss.weighting
N, D, T = 6, 2, 40
X = np.zeros((N, D, T))
OK = np.array([1, 2, 5, 17, 39, 40])


def _slice(*seeds):
    slc = fr.FruitSlice()
    slc.add(*seeds)
    return slc


def _words():
    return fr.words.of_weight(2, dim=2)


def _plain(*extra):
    return _slice(P.INC, fr.ISS(_words(), mode=fr.ISSMode.EXTENDED), S.NPI, S.END, *extra)


# ---------------------------------------------------------------- validation
def test_check_lengths_accepts_and_normalises():
    assert check_lengths(None, N, T) is None
    for dtype in (np.int64, np.int32, np.uint8, np.int16):
        got = check_lengths(OK.astype(dtype), N, T)
        assert got.dtype == np.int64 and (got == OK).all()
    assert (check_lengths(list(OK), N, T) == OK).all()


@pytest.mark.parametrize("bad", [np.ones(N - 1, dtype=int), np.ones((N, 1), dtype=int),
                                 np.ones((1, N), dtype=int), np.int64(3)],
                         ids=["short", "column", "row", "scalar"])
def test_bad_shape(bad):
    with pytest.raises(ValueError, match="shape"):
        check_lengths(bad, N, T)
    with pytest.raises(ValueError, match="shape"):
        _plain().fit(X, lengths=bad)


@pytest.mark.parametrize("bad", [[0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, T + 1], [-1, 1, 1, 1, 1, 1]],
                         ids=["zero", "beyond_T", "negative"])
def test_bad_range(bad):
    with pytest.raises(ValueError, match="1\\.\\."):
        check_lengths(np.asarray(bad), N, T)
    with pytest.raises(ValueError, match="1\\.\\."):
        _plain().fit(X, lengths=np.asarray(bad))


@pytest.mark.parametrize("bad", [OK.astype(np.float64), OK.astype(np.float32), OK > 3,
                                 OK.astype(object)], ids=["f64", "f32", "bool", "object"])
def test_bad_dtype(bad):
    with pytest.raises(TypeError, match="integers"):
        check_lengths(bad, N, T)
    with pytest.raises(TypeError, match="integers"):
        _plain().fit(X, lengths=bad)


def test_every_public_entry_takes_the_keyword_last():
    import inspect
    for fn in (fr.Fruit.fit, fr.Fruit.transform, fr.Fruit.fit_transform, fr.FruitSlice.fit,
               fr.FruitSlice.transform, fr.FruitSlice.transform_device, fr.FruitSlice.fit_transform):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "lengths" and params[-1].default is None, fn.__qualname__
    # (the positional order in front of it is the one it was)
    assert list(inspect.signature(fr.Fruit.transform).parameters)[:4] == ["self", "X", "callbacks", "cache"]
    assert list(inspect.signature(fr.Fruit.fit).parameters)[:3] == ["self", "X", "cache"]
    assert list(inspect.signature(fr.FruitSlice.fit).parameters)[:4] == ["self", "X", "cache", "deferred"]


def test_transform_validates_before_it_runs():
    slc = _plain()
    slc._fitted = True
    with pytest.raises(ValueError, match="shape"):
        slc.transform(X, lengths=OK[:3])
    with pytest.raises(TypeError, match="integers"):
        slc.transform_device(X, lengths=OK.astype(float))


# ---------------------------------------------------------------- the gate
def _unsupported():
    simple = fr.ISS(_words(), mode=fr.ISSMode.EXTENDED)
    one = [fr.words.SimpleWord("[1]")]
    generic = fr.words.Word("[ABS(1)]") if hasattr(fr.words, "Word") else None
    cases = [
        ("INC", _slice(P.INC(shift=0.1), simple, S.NPI)),
        ("INC", _slice(P.INC(shift=lambda n: 2), simple, S.NPI)),
        ("STD", _slice(P.STD(separately=False), simple, S.NPI)),
        ("NEW", _slice(P.NEW(P.INC(shift=0.5)), simple, S.NPI)),
        ("DIM", _slice(P.DIM(P.NRM(), 0), simple, S.NPI)),
        ("NEW", _slice(P.NEW(P.MAV(3)), simple, S.NPI)),
        ("ISS", _slice(fr.ISS(_words(), weighting=W.L1()), S.NPI)),
        ("ISS", _slice(fr.ISS(_words(), weighting=W.L2()), S.NPI)),
        ("ISS", _slice(fr.ISS(_words(), weighting=W.Custom(lambda Z: Z[:, 0, :])), S.NPI)),
        ("ISS", _slice(fr.ISS(one, mode=fr.ISSMode.EXTENDED, semiring=fr.semiring.Arctic(argmax=True)),
                       S.NPI)),
        ("CosWISS", _slice(fr.CosWISS(freqs=[0.5], words=one), S.NPI)),
        ("NPI", _slice(simple, S.NPI(cut=0.5))),
        ("END", _slice(simple, S.END(cut=[0.2, -1]))),
        ("MAX", _slice(simple, S.MAX(cut=[0.1, 0.9]))),
        ("INC", _slice(simple, S.INC(S.END()))),
        ("INC", _slice(simple, S.INC(S.NPI(), shift=2))),
        ("INT", _slice(simple, S.INT(S.NPI(inc=1)))),
        ("INT", _slice(simple, S.INT(S.PPV(0, True)))),
    ]
    for name in ("NRM", "LAG"):
        cases.append((name, _slice(getattr(P, name)(), simple, S.NPI)))
    if generic is not None:
        cases.append(("ISS", _slice(fr.ISS([generic]), S.NPI)))
    return cases


@pytest.mark.parametrize("name,slc", _unsupported(), ids=lambda v: v if isinstance(v, str) else "")
def test_unsupported_seed_raises_naming_itself(name, slc):
    with pytest.raises(NotImplementedError, match=name):
        slc.fit(X, lengths=OK)
    slc._fitted = True
    with pytest.raises(NotImplementedError, match=name):
        slc.transform(X, lengths=OK)
    # ... also for lengths that all equal T: the gate looks at the seeds, not at the values
    with pytest.raises(NotImplementedError, match=name):
        slc.transform(X, lengths=np.full(N, T))


def test_every_preparateur_and_sieve_class_answers():
    """Every exported seed class has the hook; the classes outside the supported set say no
    whatever their arguments."""
    for name in P.__all__ if hasattr(P, "__all__") else []:
        assert hasattr(getattr(P, name), "_supports_lengths"), name
    for name in ("NRM", "LAG"):
        assert getattr(P, name)()._supports_lengths() is False
    assert P.MAV(3)._supports_lengths() is False
    assert fr.CosWISS(freqs=[1.0], words=[fr.words.SimpleWord("[1]")])._supports_lengths() is False


def test_chained_iss_and_callbacks_raise():
    simple = fr.ISS(_words())
    chained = _slice(simple, fr.ISS([fr.words.SimpleWord("[1]")]), S.NPI)
    with pytest.raises(NotImplementedError, match="chained"):
        chained.fit(X, lengths=OK)
    slc = _plain()
    slc._fitted = True

    class Callback(fr.callback.AbstractCallback):
        pass

    with pytest.raises(NotImplementedError, match="callbacks"):
        slc.transform_device(X, [Callback()], lengths=OK)


def _supported():
    ext = fr.ISSMode.EXTENDED
    band = [S.NPI(), S.MPI(cut=[3, -1]), S.XPI(), S.LPI(), S.MAX(), S.MIN(cut=[-3, -1]), S.END(),
            S.CUR(), S.AVG(), S.STD(), S.PPV(0, True), S.CPV([0, 2], True, segments=True),
            S.INC(S.NPI()), S.INC(S.MAX(), depth=0), S.INT(S.NPI(inc=-1)), S.INT(S.MAX())]
    slices = []
    for preps in ([], [P.INC], [P.INC(shift=3, depth=2, zero_padding=False)], [P.STD],
                  [P.STD(var=False)], [P.NEW(P.INC()), P.STD], [P.DIM(P.INC(2), 0)], [P.NEW()],
                  [P.DIM(P.STD(), [0, 1])]):
        slices.append(_slice(*preps, fr.ISS(_words(), mode=ext), *band))
    for semiring in (fr.semiring.Reals(), fr.semiring.Arctic(), fr.semiring.Bayesian()):
        for weighting in (None, W.Indices(), W.Indices(total=True), W.Plateaus(4)):
            for mode in (fr.ISSMode.SINGLE, ext):
                slices.append(_slice(fr.ISS(_words(), mode=mode, semiring=semiring,
                                            weighting=weighting), *band))
    return slices


def test_every_supported_combination_passes_the_gate():
    for slc in _supported():
        got = slc._ragged_lengths(X, OK)
        assert got.dtype == np.int64 and (got == OK).all()
        assert slc._ragged_lengths(X, None) is None


# ---------------------------------------------------------------- cut resolution
LENGTHS = np.array([1, 2, 5, T])
CUTS = [(-1,), (3, -1), (-3, -1), (5, 2), (30,)]       # (30: beyond the short series)


@pytest.mark.parametrize("cut", CUTS, ids=str)
def test_cuts_resolve_like_a_series_of_that_length(cut):
    sv = S.NPI(cut=list(cut))
    got = resolve_cuts(cut, LENGTHS)
    assert got.dtype == np.int64 and got.shape == (len(LENGTHS), len(cut) + 1)
    for n, L in enumerate(LENGTHS):
        # the reference's row for a series of L elements (sorted with its 0), as a slice of L
        # elements takes it
        want = np.clip(sv._int_cut_row(int(L)), 0, L)
        np.testing.assert_array_equal(got[n], want, err_msg=f"L={L}")
        assert (np.diff(got[n]) >= 0).all() and got[n].min() >= 0 and got[n].max() <= L
    np.testing.assert_array_equal(sv._series_cut_rows(LENGTHS), got)
    # a batch of one length is the dense row
    np.testing.assert_array_equal(resolve_cuts(cut, np.full(3, T)),
                                  np.tile(np.clip(sv._int_cut_row(T), 0, T), (3, 1)))


@pytest.mark.parametrize("cut", CUTS, ids=str)
def test_end_cuts_read_what_the_truncated_series_reads(cut):
    """END reads ``X[:, c - 1]`` of the sorted row, a negative index wrapping by the series' OWN
    length; a series the reference raises IndexError for raises here."""
    sv = S.END(cut=list(cut))
    x = np.arange(1.0, T + 1)
    for L in LENGTHS:
        try:
            row = sv._int_cut_row(int(L))
        except IndexError:
            with pytest.raises(IndexError, match="out of bounds"):
                resolve_end_cuts(cut, np.array([T, L]))
            continue
        got = resolve_end_cuts(cut, np.array([L]))[0]
        want = x[:L][row[1:] - 1]                        # numpy's own wrap on the truncated series
        assert got[0] == 0 and got[1:].min() >= 1 and got[1:].max() <= L
        np.testing.assert_array_equal(x[got[1:] - 1], want, err_msg=f"L={L}")


def test_lookup_rows_one_row_per_length():
    for w in (W.Indices(), W.Indices(relative=False, scale=3), W.Plateaus(4), W.Plateaus(3, reverse=True)):
        L = np.array([7, 1, 40, 7, 2])
        got = lookup_rows(w._row, L, T)
        assert got.shape == (5, T)
        for n, length in enumerate(L):
            np.testing.assert_array_equal(got[n, :length], w._row(int(length)))
            assert (got[n, length:] == 0).all()


def test_new_entries_are_exported():
    from fruits_amd import _native as nat
    L = nat.lib()
    for name in ("fr_pipeline_set_lengths", "fr_sieve_implicit_lengths", "fr_standardize_lengths"):
        assert name in nat.EXPORTS and hasattr(L, name), name
    with open(os.path.join(os.path.dirname(HERE), "include", "fruits_hip.h")) as f:
        header = f.read()
    for name in ("fr_pipeline_set_lengths(", "fr_sieve_implicit_lengths(", "fr_standardize_lengths("):
        assert header.count("int " + name) == 1, name
    assert L.fr_version() >= 137


# ---------------------------------------------------------------- the fixture
def test_golden_ragged_is_self_consistent():
    with open(os.path.join(HERE, "golden", "golden_ragged.json")) as f:
        manifest = json.load(f)
    arrays = np.load(os.path.join(HERE, "golden", "golden_ragged.npz"))
    n, d, t = manifest["shape"]
    assert (n, d, t) == (8, 2, 600) and arrays["X"].shape == (n, d, t)
    lengths = arrays["lengths"]
    assert lengths.tolist() == manifest["lengths"] and lengths.shape == (n,)
    assert lengths.min() == 4 and lengths.max() == t and check_lengths(lengths, n, t) is not None
    np.testing.assert_array_equal(
        arrays["X"], np.random.default_rng(manifest["data_seed"]).standard_normal((n, d, t)))
    assert manifest["margin"] == 1e-10
    assert [c["name"] for c in manifest["fruit"]] == ["reals_indices", "arctic", "bayesian"]
    import test_lengths_gpu as gpu_side
    for case in manifest["fruit"]:
        out = arrays[case["out"]]
        fruit = gpu_side.build_fruit(fr, case["spec"])
        assert out.shape == (n, case["nfeatures"]) == (n, fruit.nfeatures())
        assert np.isfinite(out).all()
        assert [fruit.label(i) for i in range(fruit.nfeatures())] == case["labels"]
        fruit.get_slice()._ragged_lengths(arrays["X"], lengths)      # (passes the gate)
