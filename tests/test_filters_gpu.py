"""RDW / SPE / RPE / CTS / QTC / FUN and the filters DIL / WIN / DOT / PDD on the device against the
reference's goldens, through the classes and through the raw ``nat.prep_mask`` /
``nat.prep_pointwise``.

Bars.  Bit-exact, the sign of zero included: every mask class, CTS, QTC, SPE with a host table,
whatever DIM / NEW carry or wrap here, and RPE against this file's numpy restatement, which forms
the cosines and sines the way the product does.  RPE against the golden itself:
``|gpu - ref| <= 4 n 2^-53 (|c x0| + |s x1|)`` with n = 3 - two products, one sum, and one ulp for
a table entry that came out of another ``cos`` path (the reference takes the cosine of a scalar
per element, the product of one array); the form of test_preparation_gpu.py, doubled because both
sides round.  RDW and SPE(step_transform) take their ``pow`` / ``sin`` on the device: the project's
parity bar (README.md), 1e-6 of the row's largest magnitude, NaN in the same places.  The largest
observed ratio to a bar is printed per class (``pytest -s``).  The fruits take the bars of
test_preparation_gpu.py's fruit cases."""
import numpy as np
import pytest

from test_filters_host import ARRAYS, CASES, MANIFEST, innermost, leaf_spec, make, same_bits, transplant

pytestmark = pytest.mark.gpu
RATIOS = {}
U = 2.0 ** -53


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    yield fruits_amd
    for k, v in sorted(RATIOS.items()):
        print(f"PREP-RATIO {k}: largest |gpu - ref| / bound = {v:.3g}")


def _note(kind, ratio):
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), float(ratio))


def rounds(case):
    """RPE: 'rotate'; device pow / sin: 'libm'; everything else is exact."""
    leaf = leaf_spec(case["spec"])
    if leaf["kind"] == "RPE":
        return "rotate"
    if leaf["kind"] == "RDW" or (leaf["kind"] == "SPE" and leaf["kw"].get("step_transform")):
        return "libm"
    return None


def np_rotate(p, X):
    """The product's rotation restated: the same tables, every product rounded."""
    angles = p._angles(X.shape[2])
    c, s = np.cos(angles), np.sin(angles)
    out = np.stack([c * X[:, 0] - s * X[:, 1], s * X[:, 0] + c * X[:, 1]], axis=1)
    return out, c, s


def check(case, p, X, got):
    ref = ARRAYS[case["out"]]
    assert got.shape == ref.shape and got.dtype == np.float64, (got.shape, ref.shape)
    kind = rounds(case)
    if kind is None:
        same_bits(got, ref, case["name"])
    elif kind == "rotate":
        mine, c, s = np_rotate(p, X)
        same_bits(got, mine, case["name"])
        terms = np.abs(c * X[:, 0]) + np.abs(s * X[:, 1])
        bound = 4.0 * 3 * U * np.stack([terms, terms], axis=1)
        err = np.abs(got - ref)
        if (bound > 0).any():
            _note("RPE", (err[bound > 0] / bound[bound > 0]).max())
        assert (err <= bound).all(), (case["name"], float(err.max()))
    else:
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=case["name"])
        top = np.where(np.isnan(ref), 0.0, np.abs(ref)).max(axis=2, keepdims=True)
        bound = 1e-6 * top + np.zeros_like(ref)
        err = np.nan_to_num(np.abs(got - ref), nan=0.0)
        if (bound > 0).any():
            _note(leaf_spec(case["spec"])["kind"], (err[bound > 0] / bound[bound > 0]).max())
        assert (err <= bound).all(), (case["name"], float(err.max()))


def attach(fr, p, case):
    if "cache_x" in case:
        innermost(p)._cache = fr.cache.SharedSeedCache(ARRAYS[case["cache_x"]])


# ---------------------------------------------------------------- goldens through the classes
@pytest.mark.parametrize("case", [c for c in CASES if "out" in c], ids=lambda c: c["name"])
def test_golden_case(fr, case):
    p = transplant(case)
    X = ARRAYS[case["x"]]
    keep = X.copy()
    attach(fr, p, case)
    got = p._transform(X) if "cache_x" in case else p.transform(X)
    same_bits(X, keep)
    check(case, innermost(p), X[:, p._dim, :] if case["spec"]["kind"] == "DIM" else X, got)


def test_golden_raising_cases(fr):
    errors = {"ValueError": ValueError, "IndexError": IndexError}
    seen = 0
    for case in CASES:
        if "reference_raises" in case:
            p = make(case["spec"])
            attach(fr, p, case)
            X = ARRAYS[case["x"]]
            with pytest.raises(errors[case["reference_raises"]]):
                p._transform(X) if "cache_x" in case else p.fit_transform(X)
            seen += 1
    assert seen == 4


# ---------------------------------------------------------------- goldens through the raw ABI
@pytest.mark.parametrize("case", [c for c in CASES if "out" in c and "inner" not in c["spec"]],
                         ids=lambda c: c["name"])
def test_golden_raw_abi(fr, case):
    from fruits_amd import _native as nat
    from fruits_amd.cache import CacheType, SharedSeedCache
    p = transplant(case)
    X = ARRAYS[case["x"]]
    N, D, T = X.shape
    Xd = nat.to_device(X)
    kind, kw = case["spec"]["kind"], case["spec"]["kw"]
    f64 = lambda a: nat.to_device(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    cache = SharedSeedCache(ARRAYS[case.get("cache_x", case["x"])])
    if kind in ("DIL", "DOT", "PDD") or (kind == "CTS" and kw.get("pseudo_shift")):
        got = nat.prep_mask(Xd, nat.to_device(p._mask_words(T), dtype=np.int32))
    elif kind == "WIN":
        cs = cache.get_device(CacheType.COQUANTILE, f"{p._start}:L2")
        ce = cache.get_device(CacheType.COQUANTILE, f"{p._end}:L2")
        assert cs.dtype == nat.torch().int64
        got = nat.prep_mask(Xd, None, cs, ce)
    elif kind == "CTS":
        got = nat.prep_pointwise(nat.FR_PW_SHIFT, Xd, shift=p._steps(T))
    elif kind == "QTC":
        q = float(p._quantile)
        got = nat.prep_pointwise(nat.FR_PW_CLIP, Xd, q=q, v=q if p._bound is None else p._bound,
                                 flags=nat.FR_PW_FLAG_LOWER if p._lower else 0)
    elif kind == "RPE":
        _, c, s = np_rotate(p, X)
        got = nat.prep_pointwise(nat.FR_PW_ROTATE, Xd, f64(c), f64(s))
    elif kind == "RDW":
        got = nat.prep_pointwise(nat.FR_PW_POW, Xd, f64(p._weights))
    else:
        assert kind == "SPE"
        mode = nat.FR_PW_ADD if kw.get("operation") == "additive" else nat.FR_PW_MUL
        if kw.get("step_transform") is None:
            length = kw.get("max_length") or T
            wave = np.sin(np.arange(T) / length ** p._freq)
            got = nat.prep_pointwise(mode, Xd, f64(wave[None, :]))
        else:
            path = cache.get(CacheType.ISS, kw["step_transform"])
            with np.errstate(all="ignore"):
                last = path[:, -1:] if kw.get("max_length") is None else kw["max_length"]
                phase = path / last ** p._freq
            got = nat.prep_pointwise(mode, Xd, f64(phase), flags=nat.FR_PW_FLAG_SIN)
    same_bits(nat.to_host(Xd), X)
    check(case, p, X, nat.to_host(got))


def test_raw_mask_sources_and_slice_rules(fr):
    """Both sources at once, neither, and Python's slice rules for any counts."""
    from fruits_amd import _native as nat
    rng = np.random.default_rng(2)
    N, D, T = 9, 2, 77
    X = rng.standard_normal((N, D, T))
    X[:, :, ::5] = np.nan
    Xd = nat.to_device(X)
    same_bits(nat.to_host(nat.prep_mask(Xd)), X)
    cs = np.array([0, 1, 2, 40, 77, 78, 0, 30, 5], dtype=np.int64)
    ce = np.array([77, 1, 1, 41, 77, 90, 0, 10, 76], dtype=np.int64)
    keep = rng.integers(0, 2, T).astype(bool)
    words = np.packbits(np.pad(keep, (0, 96 - T)), bitorder="little").view(np.uint32).view(np.int32)
    i64 = lambda a: nat.to_device(a, dtype=np.int64)   # noqa: E731
    for mask in (None, keep):
        ref = np.zeros_like(X)
        for n in range(N):
            sl = slice(int(cs[n]) - 1, int(ce[n]))
            ref[n, :, sl] = X[n, :, sl]
        if mask is not None:
            ref = np.where(mask, ref, 0.0)
        md = None if mask is None else nat.to_device(words, dtype=np.int32)
        same_bits(nat.to_host(nat.prep_mask(Xd, md, i64(cs), i64(ce))), ref)
    same_bits(nat.to_host(Xd), X)


def test_raw_abi_argument_errors(fr):
    from fruits_amd import _native as nat
    t = nat.torch()
    Xd = nat.to_device(np.zeros((3, 2, 40)))
    i32 = lambda n: nat.to_device(np.zeros(n, np.int32), dtype=np.int32)   # noqa: E731
    i64 = lambda n: nat.to_device(np.zeros(n, np.int64), dtype=np.int64)   # noqa: E731
    f64 = lambda *s: nat.to_device(np.zeros(s))   # noqa: E731
    with pytest.raises(ValueError):      # one word where ceil(40 / 32) = 2 are read
        nat.prep_mask(Xd, i32(1))
    with pytest.raises(ValueError):
        nat.prep_mask(Xd, i32(3))
    with pytest.raises(ValueError):      # fewer windows than series
        nat.prep_mask(Xd, None, i64(2), i64(3))
    with pytest.raises(TypeError):
        nat.prep_mask(Xd, None, i64(3), None)
    with pytest.raises(TypeError):
        nat.prep_mask(Xd, None, i32(3), i32(3))
    with pytest.raises(ValueError):      # the input as the output
        nat.prep_mask(Xd, i32(2), out=Xd)
    with pytest.raises(ValueError):
        nat.prep_pointwise(nat.FR_PW_CLIP, Xd, out=Xd)
    with pytest.raises(ValueError):      # 3 series against 2 table rows
        nat.prep_pointwise(nat.FR_PW_MUL, Xd, f64(2, 40))
    with pytest.raises(ValueError):
        nat.prep_pointwise(nat.FR_PW_ADD, Xd, f64(1, 39))
    with pytest.raises(ValueError):      # D == 2 only
        nat.prep_pointwise(nat.FR_PW_ROTATE, nat.to_device(np.zeros((3, 3, 40))), f64(40), f64(40))
    with pytest.raises(ValueError):
        nat.prep_pointwise(nat.FR_PW_ROTATE, Xd, f64(40), f64(39))
    with pytest.raises(ValueError):
        nat.prep_pointwise(nat.FR_PW_POW, Xd, f64(3))
    with pytest.raises(ValueError):
        nat.prep_pointwise(nat.FR_PW_SHIFT, Xd, shift=-1)
    with pytest.raises(ValueError):
        nat.prep_pointwise(6, Xd)
    with pytest.raises(TypeError):
        nat.prep_pointwise(nat.FR_PW_POW, Xd, f64(2).to(t.float32))
    empty = nat.to_device(np.zeros((0, 2, 40)))
    assert tuple(nat.prep_mask(empty, i32(2)).shape) == (0, 2, 40)
    assert tuple(nat.prep_pointwise(nat.FR_PW_SHIFT, empty, shift=3).shape) == (0, 2, 40)


# ---------------------------------------------------------------- beyond the goldens
def test_many_rows_and_tiles(fr):
    """More workgroups than the goldens have: (64, 3, 2500), odd and even lengths."""
    rng = np.random.default_rng(9)
    P = fr.preparation
    for T in (2500, 2501):
        X = rng.integers(-4, 5, size=(64, 3, T)) / 2.0
        np.random.seed(T)
        p = P.DIL(0.05)
        p.fit(X)
        same_bits(p.transform(X), np.where(p._time_mask(T), X, 0.0))
        ref = np.concatenate([X[:, :, 1031:], np.repeat(X[:, :, -1:], 1031, axis=2)], axis=2)
        same_bits(P.CTS(1031).transform(X), ref)
        q = P.QTC(0.3, lower=True, bound=9.0)
        q.fit(X)
        same_bits(q.transform(X), np.where(X < q._quantile, 9.0, X))
        wave = np.sin(np.arange(T) / T ** 0.5)
        same_bits(P.SPE(0.5).transform(X), X * wave)
        # the window of every series from the cache's coquantiles, as the reference slices it
        path = np.cumsum(np.diff(X[:, 0, :], axis=1, prepend=X[:, 0, :1]) ** 2, axis=1)
        ref = np.zeros_like(X)
        for n in range(X.shape[0]):
            a = int((path[n] <= 0.2 * path[n, -1]).sum()) - 1
            b = int((path[n] <= 0.7 * path[n, -1]).sum())
            ref[n, :, a:b] = X[n, :, a:b]
        same_bits(P.WIN(0.2, 0.7).transform(X), ref)


def test_spe_user_function_and_fun(fr):
    P = fr.preparation
    X = np.random.default_rng(4).integers(-4, 5, size=(3, 2, 37)) / 2.0
    same_bits(P.SPE(0.5, function=np.cos).transform(X), X * np.cos(np.arange(37) / 37 ** 0.5))
    path = np.cumsum(np.abs(np.diff(X[:, 0, :], axis=1, prepend=X[:, 0, :1])), axis=1)
    got = P.SPE(0.5, "additive", function=np.tanh, step_transform="L1").transform(X)
    ref = X + np.tanh(path / path[:, -1:] ** 0.5)[:, None, :]
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
    with pytest.raises(ValueError):
        P.SPE(0.5, operation="subtractive").transform(X)
    same_bits(P.FUN(lambda a: a[:, ::-1, :5] * 2.0).transform(X), X[:, ::-1, :5] * 2.0)
    for bad in (lambda a: a.astype(np.float32), lambda a: a[0], lambda a: a.tolist()):
        with pytest.raises(TypeError):
            P.FUN(bad).transform(X)


def test_tables_follow_the_state(fr):
    """One upload per fit; state assigned after a transform is used."""
    P = fr.preparation
    X = np.random.default_rng(5).standard_normal((4, 2, 70))
    p = P.DOT(3)
    p.fit(X)
    first = p.transform(X)
    tables = dict(p._programs)
    assert len(tables) == 1
    p.transform(X)
    assert p._programs.keys() == tables.keys()
    assert all(p._programs[k][1] is v[1] for k, v in tables.items())
    p._n = 4
    same_bits(p.transform(X), np.where(p._time_mask(70), X, 0.0))
    assert all(p._programs[k][1] is not v[1] for k, v in tables.items())
    assert not np.array_equal(first, p.transform(X))
    w = P.RDW("uniform")
    np.random.seed(1)
    w.fit(X)
    w._weights = np.array([2.0, 1.0])
    np.testing.assert_allclose(w.transform(X), X ** np.array([2.0, 1.0])[None, :, None], rtol=1e-12)


# ---------------------------------------------------------------- whole fruits
def _build(fr, spec):
    fruit = fr.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fruit.cut()
        for p in sl.get("preps", []):
            fruit.add(make(p, fr.preparation))
        for i in sl["iss"]:
            fruit.add(fr.ISS([fr.words.SimpleWord(s) for s in i["words"]],
                             mode=getattr(fr.ISSMode, i["mode"])))
        for s in sl["sieves"]:
            fruit.add(getattr(fr.sieving, s["kind"])())
        fruit.get_slice().fit_sample_size = 1.0
    return fruit


@pytest.mark.parametrize("case", MANIFEST["fruit"], ids=lambda c: c["name"])
def test_golden_fruit(fr, case, monkeypatch):
    from fruits_amd import _native as nat
    from fruits_amd.cache import SharedSeedCache
    from oracle import ref_numpy as orc
    X = ARRAYS[case["x"]]
    prepared = ARRAYS[case["prepared"]]
    fruit = _build(fr, case["spec"])
    np.random.seed(case["seed"])
    fruit.fit(X)
    runs = []
    real_run = nat.Pipeline.run

    def counting_run(self, Xd, *a, **kw):
        runs.append((tuple(Xd.shape), self.raw_dims))
        return real_run(self, Xd, *a, **kw)
    monkeypatch.setattr(nat.Pipeline, "run", counting_run)
    out = fruit.transform(X)
    monkeypatch.undo()
    # one fused walk + sieve launch per slice, on the materialised prepared input
    assert runs == [(prepared.shape, 0)], runs
    ref = ARRAYS[case["out"]]
    labels = case["labels"]
    assert [fruit.label(i) for i in range(fruit.nfeatures())] == labels
    assert fruit.summary() == case["summary"]
    assert out.shape == ref.shape
    # the prepared input itself: masks are exact, the device sines of SPE to the parity bar
    got_prepared = nat.to_host(fruit.get_slice()._prepare_device(nat.to_device(X), SharedSeedCache(X)))
    if case["name"].startswith("spe"):
        bound = 1e-6 * np.abs(prepared).max(axis=2, keepdims=True)
        assert (np.abs(got_prepared - prepared) <= bound).all()
    else:
        same_bits(got_prepared, prepared, case["name"])
    # counting features: exact wherever the oracle, run on the reference's prepared input, sees
    # no element within 1e-10 of a threshold; the others to the project's 1e-6
    spec = {**case["spec"], "slices": [{**{k: v for k, v in sl.items() if k != "preps"},
                                        "fit_sample_size": 1.0} for sl in case["spec"]["slices"]]}
    _, expo = orc.fruit_transform_exposure(spec, orc.fruit_fit(spec, prepared), prepared, rel=1e-10)
    kinds = [lb.rsplit(" | ", 1)[-1][:3] for lb in labels]
    for c, kind in enumerate(kinds):
        if kind in ("NPI", "LPI", "XPI"):
            d = out[:, c] != ref[:, c]
            assert d.mean() <= 0.1, (labels[c], int(d.sum()))
            assert not (d & (expo[:, c] == 0)).any(), (labels[c], out[:, c], ref[:, c], expo[:, c])
            if kind == "NPI":
                assert np.all(np.abs(out[:, c] - ref[:, c]) <= expo[:, c]), labels[c]
        else:
            np.testing.assert_allclose(out[:, c], ref[:, c], rtol=1e-6, atol=1e-9, err_msg=labels[c])
