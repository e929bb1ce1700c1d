"""The fused sieve epilogue keeps its bits: every kernel family that evaluates feature ops against
what the commit BEFORE the two copies of the epilogue became one computed.

``tests/golden/epilogue_before_one_copy.npz`` was written once, on an MI355X, by
``tools/epilogue_golden.py`` on a checkout of that commit (the second copy in walk_device.h served the
wave-per-series and the CosWISS kernels, ``fop`` of walk_fused.h the cooperative fused walk).  Per
case it holds the fitted thresholds and the (N, F) feature matrix; ``meta`` holds the cases'
shapes and seeds, ``summed_run_to_run`` the largest relative difference two runs of the recorder
showed in the band-sum columns of the cooperative cases.

A case (``CASES``; the recorder imports them from here) fits a fruit of one ISS or CosWISS under
the sieve set of ``sieve_set`` on a seeded real-valued input, asserts that the thresholds are the
recorded ones, runs ``Fruit.transform``, asserts the kernel family from ``last_launch()`` and
compares the features:

* wave per series / wave per unit (``fused_packed``, CosWISS at T <= 384): every column bit for
  bit - one wave owns the row;
* cooperative kernels: every column bit for bit except the band sums of real numbers (labels MPI,
  CUR, AVG, STD - ``SUMMED`` of test_lengths_batch_gpu.py), whose wave partials meet in LDS in
  arrival order: the project's bar rtol 1e-12, atol 1e-300 (test_hip_parity.py).  The exact
  columns are at least half of all columns (asserted).

A CosWISS launch leaves no launch record (test_fused_bounds_gpu.py): asserted is that the
pipeline ran no trie walk; the kernel is the ``packed`` knob's and the length's (wave per unit at
T <= 384 unless the knob says 0, capi_walk.cpp run_coswiss).

Sieve set: every kind ``FruitSlice._fusable`` admits.  Left out is only what the pipeline refuses:
differencing orders >= 3 and cumulations (INT) on a CosWISS of several time chunks; under
``lengths=`` the float cuts, since every integer cut is a per-series slot there already; and the
float cuts of the prepared case - a pipeline that names per-series cut slots has no run-time
compiled kernel (``jit_uniform``, csrc/capi_pipeline.cpp)."""
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epilogue_before_one_copy.npz")
N_SERIES = 6
SUMMED = ("MPI", "CUR", "AVG", "STD")      # band sums of real numbers: wave partials, arrival order
ISS_WORDS = ["[1][2]", "[11][2][1]"]       # EXTENDED: five rows, a node with a second scan when weighted
COS_WORDS = ["[2][1]", "[12][1][-2][1]"]
COS_FREQS = [0.15, 0.5]
RAGGED = [1, 2, 64, 65, 128, 129]          # and T


def sieve_set(fr, T, high=True, float_cuts=True):
    """``high``: with the differencing order 3 and the cumulation."""
    S = fr.sieving
    c = max(T // 3, 1)
    out = [S.NPI(inc=0, q=(0.25, 0.75)), S.NPI(inc=1), S.NPI(inc=2, q=(0.5, 1.0)),
           S.MPI(inc=1, q=(0.25, 1.0)), S.XPI(q=(0.5, 1.0)), S.XPI(inc=2, cut=[c, -1]),
           S.MAX(cut=[c, -1], q=(0.1, 0.9)), S.MIN(cut=[c, -1], q=(0.1, 0.9)),
           S.CUR(), S.AVG(q=(0.5, 1.0)), S.STD(cut=[c, -1]),
           S.END(),
           S.PPV(0.5), S.PPV([0.2, 0.8], segments=True), S.CPV(0.5), S.CPV([0.2, 0.8], segments=True)]
    if float_cuts:
        out += [S.END(cut=[0.5, -1]), S.NPI(cut=[0.3, -1], q=(0.5, 1.0))]
    if high:
        out += [S.NPI(inc=3), S.INT(S.NPI(inc=0, q=(0.25, 0.75)))]
    return out


def _case(name, kind, T, family, cooperative, debug="", **kw):
    return dict(name=name, kind=kind, T=T, family=family, cooperative=cooperative, debug=debug, **kw)


def _cases():
    out = []
    # wave per series, ISS (walk_packed.h): one, two and three pieces
    for T in (100, 200, 300):
        for what, kw in (("reals", {}), ("indices", {"weighting": {"kind": "Indices", "scale": 2.0}}),
                         ("arctic", {"semiring": "Arctic"})):
            out.append(_case(f"packed_{what}_T{T}", "iss", T, "fused_packed", False, **kw))
    out.append(_case("packed_lengths_T200", "iss", 200, "fused_packed", False, lengths=True))
    # CosWISS: wave per unit (E 2 / 4 / 2, P 1 / 1 / 3) and cooperative (a 512 chunk, a 1024 chunk,
    # three chunks with carries and the flush behind the last)
    for T in (100, 200, 300, 500, 1000, 2100):
        for exponent in (1, 2):
            for total in (False, True):
                out.append(_case(f"coswiss_T{T}_e{exponent}_{'total' if total else 'plain'}", "coswiss", T,
                                 None, T > 384, exponent=exponent, total=total, high=T <= 1024))
    # the cooperative fused walk
    out.append(_case("fused_T1000", "iss", 1000, "fused", True))
    out.append(_case("fused_T2100_highord", "iss", 2100, "fused", True))
    out.append(_case("fused_T200_unpacked", "iss", 200, "fused", True, debug="packed=0"))
    out.append(_case("fused_T1000_total", "iss", 1000, "fused", True,
                     weighting={"kind": "Indices", "scale": 2.0, "total": True}))
    out.append(_case("fused_T1000_prepared", "iss", 1000, "fused_jit", True, prepare=True, float_cuts=False))
    out.append(_case("fused_lengths_T700", "iss", 700, "fused", True, lengths=True))
    return out


CASES = _cases()


def case_input(case):
    """The seeded input of a case: N(0, 1) for an ISS, positive (U[0, 1) + 0.25, as
    iss_bounds.coswiss_input draws it) for a CosWISS; and the per-series lengths, or None."""
    T = case["T"]
    N = N_SERIES + 1 if case.get("lengths") else N_SERIES
    rng = np.random.default_rng([CASES.index(case), N, T])
    X = rng.random((N, 2, T)) + 0.25 if case["kind"] == "coswiss" else rng.standard_normal((N, 2, T))
    lengths = np.array(RAGGED + [T]) if case.get("lengths") else None
    return X, lengths


def fitted_thresholds(slc):
    """The rows of the pipeline's threshold table, read the way ``FruitSlice._fused`` fills it."""
    from fruits_amd import _native as nat
    from fruits_amd.fruit import _reduced
    out = []
    for row in slc._sieves_extended:
        for sv in row:
            sv, kind, _, _ = _reduced(sv)
            if kind == nat.FR_SIEVE_END:
                continue
            if not sv.requires_fitting:
                sv._get_unfitted_quantiles()
            out.append(np.asarray(sv._quantiles, dtype=np.float64).ravel())
    return np.concatenate(out)


def run_case(fr, case, setenv):
    """(thresholds, (N, F) features, feature labels) of a case; asserts the kernel family."""
    setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    setenv("FRUITS_HIP_DEBUG", case["debug"])
    T = case["T"]
    X, lengths = case_input(case)
    if case["kind"] == "coswiss":
        iss = fr.CosWISS([fr.words.SimpleWord(s) for s in COS_WORDS], COS_FREQS, exponent=case["exponent"],
                         total_weighting=case["total"])
    else:
        spec = case.get("weighting")
        weighting = None if spec is None else getattr(fr.iss.weighting, spec["kind"])(
            **{k: v for k, v in spec.items() if k != "kind"})
        iss = fr.ISS([fr.words.SimpleWord(s) for s in ISS_WORDS], mode=fr.ISSMode.EXTENDED,
                     semiring=getattr(fr.semiring, case.get("semiring", "Reals"))(), weighting=weighting)
    fruit = fr.Fruit(case["name"])
    fruit.add(iss)
    fruit.add(*sieve_set(fr, T, high=case.get("high", True), float_cuts=lengths is None and case.get("float_cuts", True)))
    slc = fruit.get_slice()
    slc.fit_sample_size = 1.0
    np.random.seed(4)
    fruit.fit(X)
    thresholds = fitted_thresholds(slc)
    pipe = slc._fused(T, ragged=lengths is not None)
    assert pipe is not None, case["name"]
    if case.get("prepare"):
        pipe.prepare(X.shape[0], plan_too=False)
        assert pipe.jit_loaded() >= 1, "the pipeline's own kernel did not compile or load"
    feats = fruit.transform(X) if lengths is None else fruit.transform(X, lengths=lengths)
    assert slc._fused(T, ragged=lengths is not None) is pipe
    ran = pipe.last_launch()
    assert ran["family"] == case["family"], (case["name"], ran)
    if case["kind"] == "coswiss":
        assert case["cooperative"] == (T > 384)       # (the packed knob is at its default)
    assert (pipe.jit_loaded() >= 1) == bool(case.get("prepare"))
    labels = [fruit.label(i) for i in range(fruit.nfeatures())]
    assert feats.shape == (X.shape[0], len(labels)) and np.isfinite(feats).all()
    return thresholds, feats, labels


def summed_columns(labels):
    """The band-sum columns: the kind is the first three letters of a label's last part."""
    return np.array([lb.rsplit(" | ", 1)[-1][:3] in SUMMED for lb in labels])


def largest_relative(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
    return float(np.nanmax(rel, initial=0.0))


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_golden_holds_these_cases(golden):
    meta = json.loads(str(golden["meta"]))
    assert [c["name"] for c in meta["cases"]] == [c["name"] for c in CASES]
    for c in CASES:
        assert c["name"] + "/features" in golden and c["name"] + "/thresholds" in golden


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_epilogue_keeps_its_bits(fr, golden, monkeypatch, case):
    t0 = time.perf_counter()
    if case.get("prepare"):
        from test_hip_parity import _require_hiprtc
        _require_hiprtc(fr.ISS([fr.words.SimpleWord(s) for s in ISS_WORDS], mode=fr.ISSMode.EXTENDED)
                        ._plan(0, len(ISS_WORDS)))
    thresholds, feats, labels = run_case(fr, case, monkeypatch.setenv)
    name = case["name"]
    np.testing.assert_array_equal(thresholds, golden[name + "/thresholds"], err_msg=name + ": thresholds")
    want = golden[name + "/features"]
    assert feats.shape == want.shape, name
    summed = summed_columns(labels) if case["cooperative"] else np.zeros(len(labels), dtype=bool)
    if case["cooperative"]:
        assert 2 * int((~summed).sum()) >= len(labels) and summed.any(), name
    moved = largest_relative(feats[:, summed], want[:, summed])
    print(f"epilogue {name}: F={len(labels)} exact={int((~summed).sum())} summed={int(summed.sum())} "
          f"largest relative difference {moved:.3g} (two runs of the recorder: "
          f"{float(golden['summed_run_to_run']):.3g}) seconds={time.perf_counter() - t0:.2f}")
    for c in np.flatnonzero(~summed):
        np.testing.assert_array_equal(feats[:, c], want[:, c], err_msg=f"{name}: {labels[c]}")
    np.testing.assert_allclose(feats[:, summed], want[:, summed], rtol=1e-12, atol=1e-300, err_msg=name)
