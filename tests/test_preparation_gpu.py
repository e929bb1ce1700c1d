"""NRM / MAV / LAG / FFN / RIN / JLD and DIM on the device against the reference's goldens and
the numpy restatement of test_preparation_host.py.

Bars: NRM, LAG and the DIM / NEW plumbing are bit-exact.  RIN, MAV, JLD: elementwise
``|gpu - ref| <= 4 n 2^-53 sum|terms|`` with n the number of summands of THAT element (per output
dimension: ndim[o] (w + 1) for RIN, w for MAV, 2 ndim[o] for JLD - a product and the bias per slot)
and sum|terms| formed by the restatement - the standard bound of a sum in any order, doubled because
both sides round; no measured number enters it.  FFN: 1e-6 of the row's largest magnitude
(two layers and a relu between; the reference sums through BLAS).  Chains of preparateurs
(random cases): 1e-9 of the output's largest magnitude - each stage is a short linear map (or
NRM's division by a range that the standard-normal inputs keep within 1e3 of the magnitudes), so
three stages amplify a 1e-15 relative difference by far less than 1e6.
The largest observed ratio to the bar is printed per class (``pytest -s``)."""
import numpy as np
import pytest

from test_preparation_host import (ARRAYS, CASES, MANIFEST, U, innermost, make, np_apply, np_mav,
                                   transplant)

pytestmark = pytest.mark.gpu
RATIOS = {}


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


def check(kind, got, ref, terms=None, n=None, what=""):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if kind in ("NRM", "LAG", "INC", "exact") or terms is None and kind != "FFN":
        np.testing.assert_array_equal(got, ref, err_msg=what)
        return
    if kind == "FFN":
        bound = 1e-6 * np.abs(ref).max(axis=2, keepdims=True) + np.zeros_like(ref)
    else:
        bound = 4.0 * n * U * terms
    err = np.abs(got - ref)
    nz = bound > 0
    if nz.any():
        _note(kind, (err[nz] / bound[nz]).max())
    assert (err <= bound).all(), (what, kind, float(err.max()), float((err - bound).max()))


def leaf_kind(p):
    return type(innermost(p)).__name__


# ---------------------------------------------------------------- goldens through the classes
@pytest.mark.parametrize("case", [c for c in CASES if "out" in c], ids=lambda c: c["name"])
def test_golden_case(fr, case):
    p = transplant(case)
    X = ARRAYS[case["x"]]
    keep = X.copy()
    got = p.transform(X)
    np.testing.assert_array_equal(X, keep)
    ref = ARRAYS[case["out"]]
    kind = leaf_kind(p)
    if type(p).__name__ not in ("DIM", "NEW"):
        _, terms, n = np_apply(p, X, detail=True)
        check(kind, got, ref, terms, n, case["name"])
        return
    # the carried-over dimensions are exact, the wrapped part keeps the wrapped class's bar
    Xin = X[:, p._dim, :] if type(p).__name__ == "DIM" else X
    inner_out, terms, n = np_apply(p._preparateur, Xin, detail=True)
    k = ref.shape[1] - inner_out.shape[1]
    np.testing.assert_array_equal(got[:, :k], ref[:, :k])
    if kind in ("NRM", "LAG", "INC"):
        np.testing.assert_array_equal(got[:, k:], ref[:, k:])
    else:
        assert terms is not None, case["name"]
        check(kind, got[:, k:], ref[:, k:], terms, n, case["name"])


def test_golden_raising_cases(fr):
    for case in CASES:
        if case.get("raises_at") == "transform":
            p = make(case["spec"])
            with pytest.raises(RuntimeError):
                p.fit_transform(ARRAYS[case["x"]])


# ---------------------------------------------------------------- goldens through the raw ABI
@pytest.mark.parametrize("case", [c for c in CASES if "out" in c and c["spec"]["kind"] in
                                  ("NRM", "LAG", "MAV", "RIN", "JLD", "FFN")],
                         ids=lambda c: c["name"])
def test_golden_raw_abi(fr, case):
    from fruits_amd import _native as nat
    p = transplant(case)
    X = ARRAYS[case["x"]]
    Xd = nat.to_device(X)
    kind = case["spec"]["kind"]
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)    # noqa: E731
    dev = lambda a, dt=np.float64: nat.to_device(np.ascontiguousarray(a, dtype=dt), dtype=dt)   # noqa: E731
    if kind == "NRM":
        got = nat.prep_normalize(Xd, p._scale_dim)
    elif kind == "LAG":
        got = nat.prep_leadlag(Xd)
    elif kind == "MAV":
        if p._w > X.shape[2]:
            with pytest.raises(ValueError):
                nat.prep_moving_average(Xd, p._w)
            return
        got = nat.prep_moving_average(Xd, p._w)
    elif kind == "RIN":
        nd, dd = i32(p._ndim_per_kernel), i32(p._dims_per_kernel)
        w = p._kernel.shape[1]
        if not p._adaptive_width and w >= X.shape[2]:
            with pytest.raises(ValueError):
                nat.prep_fir(Xd, dev(p._kernel), w, dev(nd, np.int32), dev(dd, np.int32), nd, dd)
            return
        got = nat.prep_fir(Xd, dev(p._kernel[:dd.size]), w, dev(nd, np.int32), dev(dd, np.int32),
                           nd, dd, p._adaptive_width)
    elif kind == "JLD":
        nd, dd = i32(p._ndim_per_kernel), i32(p._dims_per_kernel)
        got = nat.prep_project(Xd, dev(p._kernel), dev(p._bias_weights), dev(nd, np.int32),
                               dev(dd, np.int32), nd, dd)
    else:
        got = nat.prep_ffn(Xd, dev(p._weights1), dev(p._biases), dev(p._weights2), p._center,
                           p._relu_out)
    np.testing.assert_array_equal(nat.to_host(Xd), X)
    _, terms, n = np_apply(p, X, detail=True)
    check(kind, nat.to_host(got), ARRAYS[case["out"]], terms, n, case["name"])


def test_raw_abi_argument_errors(fr):
    from fruits_amd import _native as nat
    Xd = nat.to_device(np.zeros((2, 3, 8)))
    one = np.ones(3, np.int32)
    kd = nat.to_device(np.zeros((3, 2)))
    od, dd = nat.to_device(one, dtype=np.int32), nat.to_device(np.arange(3, dtype=np.int32), dtype=np.int32)
    with pytest.raises(IndexError):      # a dims entry outside [0, D)
        nat.prep_fir(Xd, kd, 2, od, dd, one, np.array([0, 1, 3], np.int32))
    with pytest.raises(IndexError):
        nat.prep_fir(Xd, kd, 2, od, dd, one, np.array([0, -1, 2], np.int32))
    with pytest.raises(ValueError):      # group sizes that do not add up
        nat.prep_fir(Xd, kd, 2, od, dd, np.array([1, 1, 2], np.int32), np.arange(3, dtype=np.int32))
    with pytest.raises(ValueError):      # w >= T
        nat.prep_fir(Xd, nat.to_device(np.zeros((3, 8))), 8, od, dd, one, np.arange(3, dtype=np.int32))
    with pytest.raises(ValueError):
        nat.prep_moving_average(Xd, 9)
    with pytest.raises(ValueError):
        nat.prep_moving_average(Xd, 0)
    with pytest.raises(IndexError):
        nat.prep_project(Xd, nat.to_device(np.zeros(3)), nat.to_device(np.zeros(3)), od, dd, one,
                         np.array([0, 1, 5], np.int32))
    wide = nat.to_device(np.zeros((1, 17, 4)))
    with pytest.raises(ValueError):      # FR_E_LIMIT: a hidden layer over more than 16 dimensions
        nat.prep_ffn(wide, nat.to_device(np.zeros((2, 17))), nat.to_device(np.zeros(2)),
                     nat.to_device(np.zeros((1, 2))), True, False)


# ---------------------------------------------------------------- shapes across the tiling
TS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4096)


def _fitted(p, shape, seed):
    np.random.seed(seed)
    p.fit(np.broadcast_to(0.0, shape))
    return p


def _shape_cases():
    """Every T with (N, D) = (7, 3); every D at T = 1025; every N at T = 65 (and N = 2048 at
    T = 1024 with one dimension)."""
    out = [(7, 3, T) for T in TS]
    out += [(7, D, 1025) for D in (1, 6, 16)]
    out += [(1, 3, 65), (2048, 3, 65), (2048, 1, 1024), (1, 16, 4096)]
    return out


@pytest.mark.parametrize("shape", _shape_cases(), ids=lambda s: "x".join(map(str, s)))
def test_shapes_across_the_tiling(fr, shape):
    N, D, T = shape
    X = np.random.default_rng(N * 7 + D * 3 + T).standard_normal(shape)
    keep = X.copy()
    for p in (fr.preparation.NRM(), fr.preparation.NRM(True), fr.preparation.LAG()):
        check("exact", p.fit_transform(X), np_apply(p, X), what=f"{p} {shape}")
    for w in sorted({w for w in (1, 7, 64, T - 1, T) if 1 <= w <= T}):
        p = _fitted(fr.preparation.MAV(w), shape, 1)
        ref, terms, n = np_mav(X, w)
        check("MAV", p.transform(X), ref, terms, n, f"MAV {w} {shape}")
    for w in sorted({w for w in (1, 7, 64, T - 1) if 1 <= w <= T - 1}):
        for kw in ({}, {"adaptive_width": True}, {"out_dim": max(1, D // 2)}):
            p = _fitted(fr.preparation.RIN(w, **kw), shape, w)
            ref, terms, n = np_apply(p, X, detail=True)
            check("RIN", p.transform(X), ref, terms, n, f"{p} {shape}")
    if T == 1:      # the width clamps to T - 1 = 0 taps (transform.py:491-493): the self terms alone
        with np.errstate(all="ignore"):
            p = _fitted(fr.preparation.RIN(1, out_dim=1), shape, 1)
        ref, terms, n = np_apply(p, X, detail=True)
        check("RIN", p.transform(X), ref, terms, n, f"{p} {shape}")
    for kw in ({"dim": 2}, {"dim": max(1, D // 2), "distribute": True, "bias": True}):
        p = _fitted(fr.preparation.JLD(**kw), shape, 3)
        ref, terms, n = np_apply(p, X, detail=True)
        check("JLD", p.transform(X), ref, terms, n, f"{p} {shape}")
    for kw in ({}, {"d_out": 3, "center": False, "relu_out": True}):
        p = _fitted(fr.preparation.FFN(**kw), shape, 4)
        check("FFN", p.transform(X), np_apply(p, X), what=f"{p} {shape}")
    np.testing.assert_array_equal(X, keep)


def test_wide_jld_reads_global_rows(fr):
    """More than 16 input dimensions: no LDS staging, the same sums."""
    shape = (5, 40, 300)
    X = np.random.default_rng(8).standard_normal(shape)
    p = _fitted(fr.preparation.JLD(3, bias=True), shape, 5)
    ref, terms, n = np_apply(p, X, detail=True)
    check("JLD", p.transform(X), ref, terms, n, "wide JLD")
    with pytest.raises(ValueError):
        _fitted(fr.preparation.FFN(), shape, 5).transform(X)


def test_long_kernel_beyond_one_tap_chunk(fr):
    """w larger than the taps one LDS window holds: handled in several windows."""
    shape = (3, 2, 3000)
    X = np.random.default_rng(9).standard_normal(shape)
    for w in (513, 1500, 2999):
        p = _fitted(fr.preparation.RIN(w), shape, w)
        ref, terms, n = np_apply(p, X, detail=True)
        check("RIN", p.transform(X), ref, terms, n, f"RIN {w}")
        q = _fitted(fr.preparation.MAV(w), shape, w)
        ref, terms, n = np_mav(X, w)
        check("MAV", q.transform(X), ref, terms, n, f"MAV {w}")


# ---------------------------------------------------------------- random chains
def _random_prep(fr, rng, D, depth=0):
    P = fr.preparation
    # (inside a wrapper the length must stay; a hidden layer takes at most 16 dimensions)
    kinds = (["NRM", "MAV", "RIN", "JLD"] + (["FFN"] if D <= 16 else [])
             + (["LAG", "DIM", "NEW"] if depth == 0 else []))
    k = kinds[rng.integers(len(kinds))]
    if k == "NRM":
        return P.NRM(bool(rng.integers(2)))
    if k == "MAV":
        return P.MAV(int(rng.integers(1, 9)))
    if k == "LAG":
        return P.LAG()
    if k == "FFN":
        return P.FFN(int(rng.integers(1, 4)), center=bool(rng.integers(2)), relu_out=bool(rng.integers(2)))
    if k == "RIN":
        return P.RIN(int(rng.integers(1, 9)), adaptive_width=bool(rng.integers(2)),
                     out_dim=int(rng.integers(1, D + 1)) if rng.integers(2) else -1,
                     force_sum_one=bool(rng.integers(2)))
    if k == "JLD":
        dist = bool(rng.integers(2))
        return P.JLD(int(rng.integers(1, D + 1 if dist else 5)), distribute=dist, bias=bool(rng.integers(2)))
    if k == "NEW":
        return P.NEW(_random_prep(fr, rng, D, 1))
    dims = sorted(rng.choice(D, size=int(rng.integers(1, D + 1)), replace=False).tolist())
    return P.DIM(_random_prep(fr, rng, len(dims), 1), dims[0] if len(dims) == 1 else tuple(dims))


@pytest.mark.parametrize("seed", range(40))
def test_random_chains(fr, seed):
    from fruits_amd import _native as nat
    rng = np.random.default_rng(1000 + seed)
    N, D, T = int(rng.integers(1, 20)), int(rng.integers(1, 7)), int(rng.integers(12, 700))
    X = rng.standard_normal((N, D, T))
    keep = X.copy()
    X0d = Xd = nat.to_device(X)
    ref = X
    np.random.seed(seed)
    chain = []
    for _ in range(int(rng.integers(1, 4))):
        p = _random_prep(fr, rng, ref.shape[1])
        p.fit(np.broadcast_to(0.0, ref.shape))
        chain.append(str(p))
        ref = np_apply(p, ref)
        Xd = p._transform_device(Xd)
    got = nat.to_host(Xd)
    assert got.shape == ref.shape, chain
    np.testing.assert_array_equal(nat.to_host(X0d), keep)      # the chain's own device input
    scale = max(np.abs(ref).max(), 1e-300)
    assert np.abs(got - ref).max() <= 1e-9 * scale, (chain, np.abs(got - ref).max(), scale)


# ---------------------------------------------------------------- whole fruits
def _build(fr, spec):
    fruit = fr.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fruit.cut()
        for p in sl.get("preps", []):
            fruit.add(make(p, fr.preparation))
        for i in sl["iss"]:
            ws = [fr.words.SimpleWord(s) for s in i["words"]]
            fruit.add(fr.ISS(ws, mode=getattr(fr.ISSMode, i["mode"]),
                             semiring=getattr(fr.semiring, i.get("semiring", "Reals"))()))
        for s in sl["sieves"]:
            kw = {k: (tuple(v) if k == "q" else v) for k, v in s.items() if k != "kind"}
            fruit.add(getattr(fr.sieving, s["kind"])(**kw))
        fruit.get_slice().fit_sample_size = 1.0
    return fruit


@pytest.mark.parametrize("case", MANIFEST["fruit"], ids=lambda c: c["name"])
def test_golden_fruit(fr, case, monkeypatch):
    from fruits_amd import _native as nat
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
    if "DIM" not in case["summary"] or MANIFEST["numpy"].split(".")[0] == np.__version__.split(".")[0]:
        assert fruit.summary() == case["summary"]
    assert out.shape == ref.shape
    # the prepared input itself, by the classes' own bars (FFN last: 1e-6 of the row)
    preps = fruit.get_slice()._preparateurs
    got_prepared = nat.to_host(fruit.get_slice()._prepare_device(nat.to_device(X), None))
    if all(type(p).__name__ in ("NRM", "LAG") for p in preps):
        np.testing.assert_array_equal(got_prepared, prepared)
    elif len(preps) == 1:
        _, terms, n = np_apply(preps[0], X, detail=True)
        check(type(preps[0]).__name__, got_prepared, prepared, terms, n, case["name"])
    else:
        check("FFN", got_prepared, prepared, what=case["name"])
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


def test_fit_hands_over_the_prepared_shape(fr):
    """Behind LAG / JLD the raw sample's D and T are wrong: the fits see the prepared shape."""
    X = np.random.default_rng(3).standard_normal((9, 3, 40))
    fruit = fr.Fruit("shapes")
    P = fr.preparation
    fruit.add(P.LAG(), P.JLD(2), P.RIN(3), P.DIM(P.FFN(2), (0, 1)))
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED))
    fruit.add(fr.sieving.NPI(), fr.sieving.END())
    np.random.seed(1)
    fruit.fit(X)
    sl = fruit.get_slice()
    assert sl._preparateurs[1]._kernel.shape == (12,)          # 6 lead-lag dimensions x 2
    assert sl._preparateurs[2]._kernel.shape == (2, 3)
    assert sl._preparateurs[3]._preparateur._weights1.shape == (4, 2)
    out = fruit.transform(X)
    ref = X
    for p in sl._preparateurs:
        ref = np_apply(p, ref)
    assert ref.shape == (9, 2, 79)
    assert out.shape == (9, fruit.nfeatures()) and np.isfinite(out).all()


def test_non_default_stream(fr, record_property):
    """Every preparateur on a non-blocking side stream while the producer of its input still runs
    (tests/stream_order.py): bit for bit the default-stream result, which is held to ``np_apply``."""
    import stream_order as so
    X = np.random.default_rng(4).standard_normal((33, 3, 700))
    wrong = np.random.default_rng(5).standard_normal(X.shape)
    P = fr.preparation
    preps = [P.NRM(), P.LAG(), _fitted(P.MAV(7), X.shape, 1), _fitted(P.RIN(5), X.shape, 2),
             _fitted(P.JLD(2), X.shape, 3), _fitted(P.FFN(2), X.shape, 4),
             _fitted(P.DIM(P.RIN(2), 1), X.shape, 5)]
    for p in preps:
        (got,), report = so.behind_producer(lambda b, p=p: p._transform_device(b), [X], [wrong], what=str(p))
        so.note(record_property, report)
        ref = np_apply(p, X)
        scale = np.abs(ref).max()
        assert np.abs(got - ref).max() <= 1e-9 * scale, str(p)


def _new_prep_fruit(fr):
    P = fr.preparation
    fruit = fr.Fruit("sharded")
    fruit.add(P.RIN(3, out_dim=2), P.NEW(P.JLD(1, bias=True)), P.FFN(2))
    fruit.add(fr.ISS(fr.words.of_weight(3, dim=2), mode=fr.ISSMode.EXTENDED))
    fruit.add(fr.sieving.NPI(), fr.sieving.MPI(), fr.sieving.END())
    fruit.get_slice().fit_sample_size = 1.0
    return fruit


def test_sharded_transform_and_pickled_fruit(fr):
    """parallel.py's _device_block takes the same materialised path, and a fruit that receives the
    pickled fit state (Fruit.fit_state, what fit_on_root broadcasts) computes the same features."""
    from fruits_amd import parallel as par
    X = np.random.default_rng(12).standard_normal((12, 3, 300))
    fruit = _new_prep_fruit(fr)
    np.random.seed(6)
    fruit.fit(X)
    full = fruit.transform(X)
    np.testing.assert_array_equal(par.transform_sharded(fruit, X, rank=0, world=1), full)
    other = _new_prep_fruit(fr)
    other.load_fit_state(fruit.fit_state())
    np.testing.assert_array_equal(other.transform(X), full)
    np.testing.assert_array_equal(par.transform_sharded(other, X, rank=0, world=1), full)


def test_state_assigned_after_a_transform_is_used(fr):
    X = np.random.default_rng(13).standard_normal((4, 3, 50))
    p = _fitted(fr.preparation.RIN(2), X.shape, 1)
    first = p.transform(X)
    p._kernel = p._kernel * 2.0
    second = p.transform(X)
    ref, terms, n = np_apply(p, X, detail=True)
    check("RIN", second, ref, terms, n, "reassigned kernel")
    assert not np.array_equal(first, second)
