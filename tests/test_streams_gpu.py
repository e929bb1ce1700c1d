"""The stream contract: every device entry on a non-blocking side stream behind an unfinished
producer of its inputs (tests/stream_order.py has the protocol), tables replaced from the host
while a launch that reads them is still queued, and one object driven from two streams at once.

A launch, copy or table upload that went to another stream than the caller's runs while the
producer's delay still holds the side stream: it reads the WRONG values the buffers were filled
with (or the wrong input's intermediates the allocator hands out again) and the comparison fails.
The expected result is the same call on the default stream; one representative per section is also
tied to the oracle, with the assertion the existing test of that entry uses.

Shapes: N = 33, D = 3; T = 100 selects the wave-per-series kernels and the single-tile streaming
kernels, T = 1100 two time chunks with carries, two tiles and the multi-pass selection, T = 1024
the pre-compiled straight-line program of ``of_weight(2, 3)``.

``ENTRY_CASES`` / ``SYNCHRONISING`` name every entry of include/fruits_hip.h that takes a stream;
``test_every_stream_entry_is_named`` (no ``gpu`` mark) parses the header and holds that.  The GPU
tests spy on the ABI and assert that the entries they claim were called.
"""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import stream_order as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

N, D = 33, 3
TS = (100, 1100)
RTOL = 1e-6              # (the project's bar against the oracle, tests/test_hip_parity.py)

# Entries that synchronise by contract - they return host arrays - are checked on their result
# alone; everything else must return while its producer still runs.  Python name -> the
# stream-taking ABI entries it stands for.
SYNCHRONISING = {
    "Selection.result": (),                      # fr_select_ranks_end takes a handle, no stream
    "select_ranks": ("fr_select_ranks",),
    "to_host": (),
    "Fruit.transform": (),
    "Fruit.fit": (),
}
ENTRY_CASES = {}         # ABI entry -> names of the tests that run it behind a producer


def covers(*entries):
    def deco(fn):
        for e in entries:
            ENTRY_CASES.setdefault(e, []).append(fn.__name__)
        return fn
    return deco


def stream_entries():
    """The entries of include/fruits_hip.h with a ``void *stream`` parameter."""
    with open(os.path.join(ROOT, "include", "fruits_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for name, args in re.findall(r"\b(fr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", args):
            out.append(name)
    return out


def test_every_stream_entry_is_named():
    entries = stream_entries()
    assert len(entries) >= 30 and "fr_iss_run" in entries and len(set(entries)) == len(entries), entries
    assert set(SYNCHRONISING) == {"Selection.result", "select_ranks", "to_host", "Fruit.transform",
                                  "Fruit.fit"}
    sync = {e for v in SYNCHRONISING.values() for e in v}
    for e in entries:
        assert (e in ENTRY_CASES) != (e in sync), \
            f"{e} takes a stream: name it in exactly one of a case (covers) and SYNCHRONISING"
    assert not (set(ENTRY_CASES) | sync) - set(entries), (set(ENTRY_CASES) | sync) - set(entries)
    for e, tests in ENTRY_CASES.items():
        for name in tests:
            assert callable(globals().get(name)), (e, name)


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native
    _native.require_device()
    t0 = time.perf_counter()
    yield fruits_amd
    hosts = [r.host_ms for r in so.REPORTS]
    if hosts:
        print(f"\nSTREAMS {len(so.REPORTS)} runs behind a producer: host_ms median "
              f"{np.median(hosts):.3f} max {max(hosts):.3f}; delay_ms min "
              f"{min(r.delay_ms for r in so.REPORTS):.1f} max {max(r.delay_ms for r in so.REPORTS):.1f}; "
              f"attempts max {max(r.attempts for r in so.REPORTS)}; not pending "
              f"{sum(not r.pending for r in so.REPORTS)}; cycles/ms {so.cycles_per_ms():.0f}; "
              f"wall {time.perf_counter() - t0:.1f} s")


@pytest.fixture(scope="module")
def nat(fr):
    from fruits_amd import _native
    return _native


@pytest.fixture(scope="module")
def torch(fr):
    import torch as t
    return t


class Spy(set):
    def expect(self, *entries):
        missing = set(entries) - self
        assert not missing, f"the case did not run {sorted(missing)} (ran {sorted(self)})"


@pytest.fixture
def abi(nat, monkeypatch):
    """The stream-taking entries a test ran: the ABI functions of the loaded library wrapped."""
    L, seen = nat.lib(), Spy()
    for name in stream_entries():
        def spy(*a, _o=getattr(L, name), _n=name):
            seen.add(_n)
            return _o(*a)
        monkeypatch.setattr(L, name, spy)
    return seen


@pytest.fixture
def generic_kernels(monkeypatch):
    """The library's own instances: nothing compiled at run time (as the existing tests set it)."""
    monkeypatch.setenv("FRUITS_HIP_JIT", "0")
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")


def draw(T, seed, kind="normal", shape=None):
    """Finite random values: ``seed`` 1 the true input, 2 the wrong one, 3 and 4 further ones."""
    rng = np.random.default_rng([2027, seed, T])
    shape = (N, D, T) if shape is None else shape
    if kind == "uniform":                         # (Bayesian, CosWISS: positive)
        return 0.25 + 0.75 * rng.random(shape)
    if kind == "walk":
        return rng.standard_normal(shape).cumsum(axis=-1) / np.sqrt(shape[-1])
    return rng.standard_normal(shape)


def rowwise_close(got, ref, rtol=RTOL):
    flat_g, flat_r = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    scale = np.max(np.abs(flat_r), axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    err = np.max(np.abs(flat_g - flat_r) / scale)
    assert got.shape == ref.shape and err <= rtol, f"row-wise relative error {err:.3e} > {rtol}"


def run(call, T, what, record_property, kind="normal", shape=None, **kw):
    want, report = so.behind_producer(call, [draw(T, 1, kind, shape)], [draw(T, 2, kind, shape)],
                                      what=what, **kw)
    so.note(record_property, report)
    return want


# ------------------------------------------------------------------ forward, materialising
def _iss_cases():
    """name -> (ISS factory, kind of input, needs fit, entries it must run, Ts)."""
    def words(fr, *strings):
        return [fr.words.SimpleWord(s) for s in strings]

    def cos(fr, **kw):
        return fr.CosWISS(words(fr, "[1]", "[2][1]", "[1][2][3]"), [0.15, 0.5], exponent=2, **kw)
    W = lambda fr: fr.iss.weighting                     # noqa: E731
    S = lambda fr: fr.iss.semiring                      # noqa: E731
    ext = lambda fr: fr.ISSMode.EXTENDED                # noqa: E731
    w23 = lambda fr: fr.words.of_weight(2, dim=3)       # noqa: E731
    generic = ["[ABS(1)DIM(2)][ABS(1)]", "[DIM(1)][][DIM(2)]", "[DIM(2)]"]
    return {
        "reals_static": (lambda fr: fr.ISS(w23(fr), mode=ext(fr)), "normal", ("fr_iss_run",), TS + (1024,)),
        "reals_interpreted": (lambda fr: fr.ISS(words(fr, "[1][2]", "[12][3]", "[1][1][3]", "[3]")),
                              "normal", ("fr_iss_run",), TS),
        "indices_total": (lambda fr: fr.ISS(w23(fr), mode=ext(fr), weighting=W(fr).Indices(total=True)),
                          "normal", ("fr_iss_run",), TS),
        "indices_nontotal": (lambda fr: fr.ISS(w23(fr), mode=ext(fr), weighting=W(fr).Indices()),
                             "normal", ("fr_iss_run",), TS),
        "l1": (lambda fr: fr.ISS(w23(fr), mode=ext(fr), weighting=W(fr).L1(on_prepared=True)),
               "normal", ("fr_iss_run", "fr_pathlen_lookup"), TS),
        "arctic": (lambda fr: fr.ISS(w23(fr), mode=ext(fr), semiring=S(fr).Arctic()),
                   "normal", ("fr_iss_run",), TS),
        "arctic_argmax": (lambda fr: fr.ISS(w23(fr), mode=ext(fr), semiring=S(fr).Arctic(argmax=True)),
                          "normal", ("fr_iss_run", "fr_arctic_argmax"), TS),
        "bayesian": (lambda fr: fr.ISS(w23(fr), mode=ext(fr), semiring=S(fr).Bayesian()),
                     "uniform", ("fr_iss_run",), TS),
        "generic_reals": (lambda fr: fr.ISS([fr.words.Word(s) for s in generic], mode=ext(fr)),
                          "normal", ("fr_iss_run", "fr_letter_rows"), TS),
        "generic_bayesian": (lambda fr: fr.ISS([fr.words.Word(s) for s in generic], mode=ext(fr),
                                               semiring=S(fr).Bayesian()),
                             "uniform", ("fr_iss_run", "fr_letter_rows", "fr_rows_unshift"), TS),
        "coswiss": (lambda fr: cos(fr), "uniform", ("fr_iss_run",), TS),
        "coswiss_dropout": (lambda fr: cos(fr, dropout=0.2), "uniform", ("fr_iss_run",), TS),
        "coswiss_ffn": (lambda fr: cos(fr, ffn_size=2), "uniform", ("fr_iss_run", "fr_coswiss_ffn"), TS),
        "coswiss_terms": (lambda fr: fr.CosWISS(words(fr, "[1][2]", "[2]"), [0.3, 0.5], exponent=9,
                                                total_weighting=True),
                          "uniform", ("fr_iss_run", "fr_coswiss_combine"), TS),
    }


ISS_CASES = _iss_cases()


@gpu
@covers("fr_iss_run", "fr_pathlen_lookup", "fr_arctic_argmax", "fr_letter_rows", "fr_rows_unshift",
        "fr_coswiss_ffn", "fr_coswiss_combine")
@pytest.mark.parametrize("name,T", [(n, T) for n, c in ISS_CASES.items() for T in c[3]])
def test_forward_materialising(fr, abi, record_property, name, T):
    make, kind, entries, _ = ISS_CASES[name]
    iss = make(fr)
    X = draw(T, 1, kind)
    if iss.requires_fitting:
        np.random.seed(7)
        iss.fit(X)
    want = run(lambda b: iss.transform_device(b), T, f"ISS.transform_device {name} T={T}",
               record_property, kind)
    abi.expect(*entries)
    if name == "reals_static":      # the anchor of this section: the oracle, row-wise to 1e-6
        from oracle import ref_numpy as orc
        ref = orc.iss_transform(X, [str(w) for w in iss.words], "EXTENDED")
        rowwise_close(want[0], ref)
        if T == 1024:
            assert iss._plan(0, len(iss.words)).static_program_index() > 0


# ------------------------------------------------------------------ fused
def _fruit(fr, preps, iss, sieves, X, lengths=None):
    fruit = fr.Fruit("streams")
    for p in preps:
        fruit.add(p)
    fruit.add(iss)
    for s in sieves:
        fruit.add(s)
    fruit.get_slice().fit_sample_size = 1.0
    np.random.seed(3)
    fruit.fit(X)
    return fruit


def _fused_cases():
    """name -> (preparateurs, ISS, sieves, input kind, must fuse, entries)."""
    def make(fr, name):
        P, V, W, S = fr.preparation, fr.sieving, fr.iss.weighting, fr.iss.semiring
        ext = fr.ISSMode.EXTENDED
        w23 = fr.words.of_weight(2, dim=3)
        plain = lambda: fr.ISS(w23, mode=ext)                      # noqa: E731
        band = (0.5, 1.0)
        return {
            "npi_mpi_end": ([], fr.ISS(w23, mode=ext, weighting=W.Indices()),
                            [V.NPI(q=band), V.MPI(q=band), V.END()]),
            "max_min_xpi": ([], plain(), [V.MAX(q=(-1, 0, 1)), V.MIN(cut=[40, -1]), V.XPI(q=band)]),
            "cur": ([], plain(), [V.CUR(q=band), V.END()]),
            "ppv_cpv": ([], plain(), [V.PPV(quantile=0.5), V.CPV(quantile=[0.25, 0.75])]),
            "lpi": ([], plain(), [V.LPI(q=band), V.END()]),
            "inc_std": ([P.INC(), P.STD()], plain(), [V.NPI(q=band), V.END()]),
            "arctic_argmax": ([], fr.ISS(w23, mode=ext, semiring=S.Arctic(argmax=True)),
                              [V.NPI(q=band), V.MPI(), V.END()]),
        }[name]
    fused = {"npi_mpi_end": "fr_pipeline_run", "max_min_xpi": "fr_pipeline_run", "cur": "fr_pipeline_run",
             "ppv_cpv": "fr_pipeline_run", "lpi": None, "inc_std": "fr_pipeline_run",
             "arctic_argmax": "fr_pipeline_run"}
    return make, fused


FUSED_MAKE, FUSED = _fused_cases()


def slice_call(fr, slc, shape, lengths=None):
    """``FruitSlice.transform_device`` on a DEVICE buffer: the host array it is handed gives the
    shape alone, the cache hands out the buffer as its upload of that array."""
    host = np.zeros(shape)

    def call(buf):
        cache = fr.cache.SharedSeedCache(host)
        cache.adopt_device_input(buf)
        return slc.transform_device(host, cache=cache, lengths=lengths)
    return call


SUMMED = ("MPI", "CUR", "AVG", "STD")      # band sums of real numbers: wave partials, arrival order


def loose_columns(fruit):
    """The band-sum columns of a fruit's features: iterated sum by iterated sum, sieve by sieve,
    the sieve's own features (no label is asked: an argmax ISS has none)."""
    out = []
    for slc in fruit:
        per = [type(sv).__name__ in SUMMED for sv in slc.get_sieves() for _ in range(sv.nfeatures())]
        assert slc.nfeatures() % len(per) == 0
        out += per * (slc.nfeatures() // len(per))
    assert len(out) == fruit.nfeatures()
    return np.array(out)


@gpu
@covers("fr_pipeline_run", "fr_iss_run", "fr_sieve")
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", list(FUSED))
def test_fused_slice(fr, abi, generic_kernels, record_property, name, T):
    X = draw(T, 1, "walk")
    fruit = _fruit(fr, *FUSED_MAKE(fr, name), X)
    slc = fruit.get_slice()
    want = run(slice_call(fr, slc, X.shape), T, f"FruitSlice.transform_device {name} T={T}",
               record_property, "walk", loose=loose_columns(fruit))
    if FUSED[name] is None:
        assert slc._fused(T) is None
        abi.expect("fr_iss_run", "fr_sieve")
    else:
        assert slc._fused(T) is not None and slc._fused(T).jit_loaded() == 0
        abi.expect("fr_pipeline_run")
    assert np.isfinite(want[0]).all()
    if name == "npi_mpi_end" and T == 100:      # the anchor of this section
        _oracle_features(fruit, X, want[0])


def _oracle_features(fruit, X, got):
    """The assertion of tests/test_preparation_gpu.py::test_golden_fruit: counting features exact
    wherever the oracle sees no element within 1e-10 of a threshold, the others to 1e-6."""
    from oracle import ref_numpy as orc
    spec = {"slices": [{"iss": [{"words": [str(w) for w in fruit.get_slice().get_iss()[0].words],
                                 "mode": "EXTENDED", "weighting": {"kind": "Indices"}}],
                        "sieves": [{"kind": "NPI", "q": [0.5, 1.0]}, {"kind": "MPI", "q": [0.5, 1.0]},
                                   {"kind": "END"}], "fit_sample_size": 1.0}]}
    np.random.seed(3)
    ref, expo = orc.fruit_transform_exposure(spec, orc.fruit_fit(spec, X), X, rel=1e-10)
    assert got.shape == ref.shape
    for c in range(got.shape[1]):
        lb = fruit.label(c)
        if "NPI" in lb:
            d = got[:, c] != ref[:, c]
            assert not (d & (expo[:, c] == 0)).any(), lb
            assert np.all(np.abs(got[:, c] - ref[:, c]) <= expo[:, c]), lb
        elif "MPI" in lb:
            quiet = expo[:, c] == 0
            np.testing.assert_allclose(got[quiet, c], ref[quiet, c], rtol=RTOL, atol=1e-9, err_msg=lb)
        else:
            np.testing.assert_allclose(got[:, c], ref[:, c], rtol=RTOL, atol=1e-9, err_msg=lb)


@gpu
@covers("fr_pipeline_run")
def test_fused_slice_compiled_kernel(fr, abi, monkeypatch, record_property):
    """One of the above with the pipeline's own kernel loaded (hipRTC)."""
    monkeypatch.setenv("FRUITS_HIP_JIT", "1")
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    T = 1100
    X = draw(T, 1, "walk")
    fruit = _fruit(fr, *FUSED_MAKE(fr, "npi_mpi_end"), X)
    slc = fruit.get_slice()
    pipe = slc._fused(T)
    pipe.prepare(N)
    if pipe.jit_loaded() == 0:
        pytest.skip("hipRTC is not installed")
    run(slice_call(fr, slc, X.shape), T, "FruitSlice.transform_device, compiled kernel",
        record_property, "walk", loose=loose_columns(fruit))
    abi.expect("fr_pipeline_run")


@gpu
@covers("fr_pipeline_run")
def test_fused_plan_in_pieces(fr, abi, monkeypatch, record_property):
    """A plan in pieces (the knobs of test_hip_parity.py::test_large_plan_in_pieces, its smallest
    variant): one launch per piece type, the gather of the row blocks - all on the caller's stream."""
    monkeypatch.setenv("FRUITS_HIP_JIT", "1")
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    monkeypatch.setenv("FRUITS_HIP_DEBUG", "pieces=1,piece_min=50,piece_nodes=12")
    T, shape = 600, (N, 2, 600)
    X = draw(T, 1, "walk", shape)
    words = list(fr.words.of_weight(4, dim=2)) + [fr.words.SimpleWord("[1][-2][11][2]")]
    V = fr.sieving
    fruit = _fruit(fr, [fr.preparation.INC()],
                   fr.ISS(words, mode=fr.ISSMode.EXTENDED, weighting=fr.iss.weighting.Indices()),
                   [V.NPI(q=(0.5, 1.0)), V.NPI(), V.END()], X)
    slc = fruit.get_slice()
    pipe = slc._fused(T)
    assert pipe is not None and pipe.plan.nodes >= 60
    pipe.prepare(N)
    if pipe.pieces_loaded() == 0:
        pytest.skip("hipRTC is not installed")
    run(slice_call(fr, slc, shape), T, "FruitSlice.transform_device, plan in pieces", record_property,
        "walk", shape)
    assert pipe.last_launch()["family"] == "fused_pieces"
    abi.expect("fr_pipeline_run")


def _lengths(T):
    return np.array([T, T - 1, T // 2, 9, T - 37, T // 3 + 1] * 6, dtype=np.int64)[:N]


@gpu
@covers("fr_pipeline_run", "fr_sieve_implicit_lengths", "fr_standardize_lengths", "fr_increments",
        "fr_iss_run", "fr_sieve")
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("fused", ["1", "0"])
def test_ragged_slice(fr, abi, generic_kernels, monkeypatch, record_property, fused, T):
    """``lengths=``: the fused path, and the launches of the materialising one."""
    monkeypatch.setenv("FRUITS_AMD_FUSED", fused)
    X = draw(T, 1, "walk")
    P, V = fr.preparation, fr.sieving
    fruit = _fruit(fr, [P.INC(), P.STD()], fr.ISS(fr.words.of_weight(2, dim=3), mode=fr.ISSMode.EXTENDED),
                   [V.NPI(), V.PPV(quantile=[0.0, 0.5], constant=True), V.END()], X)
    slc = fruit.get_slice()
    run(slice_call(fr, slc, X.shape, _lengths(T)), T, f"ragged transform_device fused={fused} T={T}",
        record_property, "walk")
    if fused == "1":
        abi.expect("fr_pipeline_run")
    else:
        abi.expect("fr_increments", "fr_standardize_lengths", "fr_iss_run", "fr_sieve",
                   "fr_sieve_implicit_lengths")


# ------------------------------------------------------------------ standalone kernels
def _fitted(p, shape, seed, X=None):
    np.random.seed(seed)
    p.fit(np.broadcast_to(0.0, shape) if X is None else X)
    return p


@gpu
@covers("fr_prep_mask", "fr_prep_pointwise")
@pytest.mark.parametrize("T", TS)
def test_filter_preparateurs(fr, abi, record_property, T):
    """The preparateurs of kernels_filter.hip through their classes, bit for bit."""
    P = fr.preparation
    X = draw(T, 1)
    preps = [_fitted(P.DIL(0.05), X.shape, 1), P.CTS(7), _fitted(P.QTC(0.3, lower=True, bound=9.0), X.shape, 2, X),
             P.SPE(0.5), P.SPE(0.5, "additive"), _fitted(P.DOT(3), X.shape, 3), _fitted(P.PDD(), X.shape, 4)]
    for p in preps:
        run(lambda b, p=p: p._transform_device(b), T, f"{p} T={T}", record_property)
    abi.expect("fr_prep_mask", "fr_prep_pointwise")


@gpu
@covers("fr_increments", "fr_standardize", "fr_standardize_lengths", "fr_pre_transform", "fr_nan_to_num",
        "fr_pathlen_lookup")
@pytest.mark.parametrize("T", TS)
def test_streaming_kernels(fr, nat, torch, abi, record_property, T):
    P = fr.preparation
    X = draw(T, 1)
    for what, call in (("increments", lambda b: nat.increments(b, 3)),
                       ("increments with a head", lambda b: nat.increments(b, 2, head_src=b, head=2)),
                       ("INC(2, depth=2)", lambda b: P.INC(2, 2)._transform_device(b)),
                       ("standardize", lambda b: nat.standardize(b, True, 1e-5)),
                       ("STD(var=False)", lambda b: P.STD(var=False)._transform_device(b)),
                       ("pathlen_lookup L2", lambda b: nat.pathlen_lookup(b, norm=2, relative=1))):
        want = run(call, T, f"{what} T={T}", record_property)
        if what == "increments":        # the anchor: bit for bit, as tests/test_hip_parity.py holds it
            ref = np.zeros_like(X)
            ref[:, :, 3:] = X[:, :, 3:] - X[:, :, :-3]
            np.testing.assert_array_equal(want[0], ref)
    lengths_d = nat.to_device(_lengths(T).astype(np.int32), dtype=np.int32)
    torch.cuda.synchronize()
    run(lambda b: nat.standardize(b, True, 1e-5, lengths_d=lengths_d), T, f"standardize, lengths T={T}",
        record_property)
    for inc in (0, 1, 2):
        run(lambda b, inc=inc: nat.pre_transform(b, inc), T, f"pre_transform inc={inc} T={T}", record_property,
            shape=(N, T))
    # nan_to_num: the NaNs and infinities ARE the data here (in the true input alone)
    holes = draw(T, 1)
    holes[::3, 1, ::7] = np.nan
    holes[1, 2, 5] = np.inf
    want, report = so.behind_producer(lambda b: nat.nan_to_num(b.clone()), [holes], [draw(T, 2)],
                                      what=f"nan_to_num T={T}", finite=False)
    so.note(record_property, report)
    np.testing.assert_array_equal(want[0], np.nan_to_num(holes, nan=0.0))
    abi.expect("fr_increments", "fr_standardize", "fr_standardize_lengths", "fr_pre_transform",
               "fr_nan_to_num", "fr_pathlen_lookup")


SIEVE_KINDS = ("NPI", "MPI", "XPI", "LPI", "MAX", "MIN", "END", "CUR")


@gpu
@covers("fr_sieve", "fr_pre_transform", "fr_iss_run")
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("kind", SIEVE_KINDS)
def test_sieve(fr, nat, torch, abi, record_property, kind, T):
    """``fr_sieve`` for every kind and differencing order -1, 0, 2, through the classes (order -1:
    a cumulative sum by the plan of the word ``[1]`` in front of the sieve) and the wrapper."""
    V = fr.sieving
    cut, q = [T // 3, -1], (-1, 0, 1)
    incs = (-1, 0, 2) if kind in ("NPI", "MPI", "XPI", "LPI") else (None,)
    for inc in incs:
        sv = getattr(V, kind)(cut, q, inc) if inc is not None else (
            V.END(cut) if kind == "END" else getattr(V, kind)(cut, q))

        def call(b, sv=sv):
            out = torch.zeros((N, sv.nfeatures()), dtype=torch.float64, device=b.device)
            sv.transform_device(b, out, 0)
            return out
        loose = np.ones(sv.nfeatures(), dtype=bool) if kind == "MPI" else None
        want = run(call, T, f"{sv} T={T}", record_property, "walk", (N, T), loose=loose)
        if kind == "END":               # the anchor: the gathered elements themselves
            A = draw(T, 1, "walk", (N, T))
            np.testing.assert_array_equal(want[0], A[:, [T // 3 - 1, T - 1]])
    abi.expect("fr_sieve")
    if incs != (None,):
        # the raw wrapper, every order the ABI takes, into a column block of a wider tensor
        cuts_d = nat.to_device(np.array([[0, T // 3, T]], dtype=np.int64), dtype=np.int64)
        q_d = nat.to_device(np.array([-np.inf, 0.0, np.inf]))
        torch.cuda.synchronize()
        code = getattr(nat, f"FR_SIEVE_{kind}")

        def raw(b):
            out = torch.zeros((N, 7), dtype=torch.float64, device=b.device)
            return nat.sieve(code, b, 2, cuts_d, q_d, out, out_col=2)
        loose = np.array([False, False, True, True, True, True, False]) if kind == "MPI" else None
        run(raw, T, f"nat.sieve {kind} inc=2 T={T}", record_property, "walk", (N, T), loose=loose)


@gpu
@covers("fr_sieve_implicit", "fr_sieve_implicit_lengths")
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("kind", ["PPV", "CPV"])
def test_sieve_implicit(fr, torch, abi, record_property, kind, T):
    for segments in (False, True):
        sv = getattr(fr.sieving, kind)(quantile=[-0.3, 0.0, 0.4], constant=True, segments=segments)
        sv.fit(np.zeros((2, 4)))
        for lengths in (None, _lengths(T)):
            def call(b, sv=sv, lengths=lengths):
                out = torch.zeros((N, sv.nfeatures()), dtype=torch.float64, device=b.device)
                sv.transform_device(b, out, 0, lengths=lengths)
                return out
            want = run(call, T, f"{kind} segments={segments} lengths={lengths is not None} T={T}",
                       record_property, "walk", (N, T))
            if kind == "PPV" and not segments and lengths is None:      # the anchor: a proportion
                A = draw(T, 1, "walk", (N, T))
                ref = np.stack([(A >= v).sum(axis=1) / T for v in (-0.3, 0.0, 0.4)], axis=1)
                np.testing.assert_allclose(want[0], ref, rtol=1e-12, atol=0)
    abi.expect("fr_sieve_implicit", "fr_sieve_implicit_lengths")


@gpu
@covers("fr_sieve_pick")
@pytest.mark.parametrize("T", TS)
def test_sieve_pick(fr, nat, torch, abi, record_property, T):
    from fruits_amd import nn
    V = fr.sieving
    head = nn._Head([V.END([T // 2, -1]), V.MAX([T // 3, -1], (-1, 0, 1)), V.MIN()])
    spec, spec_d, cuts_d, q_d = head.tables(T, torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()
    K = 4
    want = run(lambda b: nat.sieve_pick(b, spec, spec_d, cuts_d, q_d, head.F), T, f"sieve_pick T={T}",
               record_property, "walk", (K, N, T))
    A = draw(T, 1, "walk", (K, N, T))
    feat, pos = want
    assert feat.shape == (N, K, head.F) and pos.dtype == np.int32
    np.testing.assert_array_equal(feat[:, :, 1], A[:, :, T - 1].T)          # END(-1)
    np.testing.assert_array_equal(feat[:, :, -1], A.min(axis=2).T)          # MIN over the row
    picked = pos >= 0
    n, k, _ = np.nonzero(picked)
    np.testing.assert_array_equal(feat[picked], A[k, n, pos[picked]])
    abi.expect("fr_sieve_pick")


@gpu
@covers("fr_prep_fir", "fr_prep_project", "fr_prep_normalize", "fr_prep_leadlag")
def test_raw_preparateur_wrappers(fr, nat, torch, abi, record_property):
    """The ``_native`` wrappers of kernels_prep.hip themselves (the classes:
    tests/test_preparation_gpu.py::test_non_default_stream)."""
    T = 1100
    X = draw(T, 1)
    rin = _fitted(fr.preparation.RIN(5), X.shape, 2)
    jld = _fitted(fr.preparation.JLD(2), X.shape, 3)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)                              # noqa: E731
    dev = lambda a, dt=np.float64: nat.to_device(np.ascontiguousarray(a, dtype=dt), dtype=dt)   # noqa: E731
    nd, dd = i32(rin._ndim_per_kernel), i32(rin._dims_per_kernel)
    rin_t = (dev(rin._kernel[:dd.size]), rin._kernel.shape[1], dev(nd, np.int32), dev(dd, np.int32), nd, dd)
    jn, jd = i32(jld._ndim_per_kernel), i32(jld._dims_per_kernel)
    jld_t = (dev(jld._kernel), dev(jld._bias_weights), dev(jn, np.int32), dev(jd, np.int32), jn, jd)
    torch.cuda.synchronize()
    for what, call in (("prep_normalize", lambda b: nat.prep_normalize(b, False)),
                       ("prep_leadlag", lambda b: nat.prep_leadlag(b)),
                       ("prep_moving_average", lambda b: nat.prep_moving_average(b, 7)),
                       ("prep_fir", lambda b: nat.prep_fir(b, *rin_t)),
                       ("prep_project", lambda b: nat.prep_project(b, *jld_t))):
        run(call, T, what, record_property)
    abi.expect("fr_prep_fir", "fr_prep_project", "fr_prep_normalize", "fr_prep_leadlag")


@gpu
@covers("fr_memcpy_h2d", "fr_memcpy_d2h", "fr_stream_sync")
def test_raw_copies_and_stream_sync(nat, torch, abi, record_property):
    """fr_memcpy_h2d / fr_memcpy_d2h queue a copy on the given stream and fr_stream_sync waits for
    it: a download behind the producer holds the produced values, an upload lands behind it.  They
    wait by contract (pageable host memory): checked on the result alone."""
    T = 1100
    L = nat.lib()

    def call(b):
        st = nat.stream_ptr()
        host = np.empty(tuple(b.shape))
        nat.check(L.fr_memcpy_d2h(host.ctypes.data_as(C.c_void_p), nat.dptr(b), C.c_int64(host.nbytes), st))
        nat.check(L.fr_stream_sync(st))
        back = torch.empty_like(b)
        up = host * 2.0
        nat.check(L.fr_memcpy_h2d(nat.dptr(back), up.ctypes.data_as(C.c_void_p), C.c_int64(up.nbytes), st))
        nat.check(L.fr_stream_sync(st))
        return back
    want = run(call, T, "fr_memcpy_d2h / fr_stream_sync / fr_memcpy_h2d", record_property, synchronising=True)
    np.testing.assert_array_equal(want[0], draw(T, 1) * 2.0)
    abi.expect("fr_memcpy_h2d", "fr_memcpy_d2h", "fr_stream_sync")


# ------------------------------------------------------------------ fit (SYNCHRONISING)
def _thresholds(slc):
    from fruits_amd.fruit import _leaf
    out = []
    for row in slc._sieves_extended:
        for sv in row:
            if sv.requires_fitting:
                out.append(np.asarray(_leaf(sv)._quantiles, dtype=np.float64))
    return np.concatenate(out)


@gpu
@covers("fr_select_ranks_begin")
@pytest.mark.parametrize("T", TS)
def test_fit_behind_a_producer(fr, torch, abi, generic_kernels, record_property, T):
    """``Fruit.fit`` of a two-slice fruit whose sample is gathered on the device from a buffer that
    is still being produced: the thresholds of the default-stream fit, bit for bit; and
    ``Fruit.transform`` / ``to_host`` behind the same producer."""
    V = fr.sieving
    fruit = fr.Fruit("fit on a side stream")
    fruit.add(fr.preparation.INC(), fr.ISS(fr.words.of_weight(2, dim=3), mode=fr.ISSMode.EXTENDED),
              V.NPI(q=(0.3, 0.7, 1.0)), V.MPI(q=(0.5, 1.0)), V.END())
    fruit.cut()
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=3), mode=fr.ISSMode.EXTENDED, semiring=fr.iss.semiring.Arctic()),
              V.NPI(q=(0.5, 1.0), inc=0), V.PPV(quantile=0.5))
    for k in range(2):
        fruit.get_slice(k).fit_sample_size = 1.0
    host = np.zeros((N, D, T))
    loose = loose_columns(fruit)

    def fit(b):
        cache = fr.cache.SharedSeedCache(host)
        cache.adopt_device_input(b)
        np.random.seed(5)
        fruit.fit(host, cache=cache)
        th = np.concatenate([_thresholds(fruit.get_slice(k)) for k in range(2)])
        return torch.from_numpy(th).cuda()

    def transform(b):
        cache = fr.cache.SharedSeedCache(host)
        cache.adopt_device_input(b)
        return torch.from_numpy(fruit.transform(host, cache=cache)).cuda()
    want = run(fit, T, f"Fruit.fit T={T}", record_property, "walk", synchronising=True)
    assert np.isfinite(want[0]).sum() >= 18 * 4
    abi.expect("fr_select_ranks_begin")
    # the anchor: every finite threshold is np.quantile's of the oracle's rows, as the device-side
    # fit's own tests hold it (tests/test_select_gpu.py: exact order statistics)
    from oracle import ref_numpy as orc
    X = draw(T, 1, "walk")
    inc = np.zeros_like(X)
    inc[:, :, 1:] = X[:, :, 1:] - X[:, :, :-1]
    its = orc.iss_transform(inc, [str(w) for w in fr.words.of_weight(2, dim=3)], "EXTENDED")
    first = np.sort(want[0][:3])            # row 0, NPI(q=(0.3, 0.7, 1.0)) at inc 1
    ref = np.quantile(orc.pre_transform(its[0], 1), [0.3, 0.7])
    np.testing.assert_allclose(first[:2], ref, rtol=RTOL)
    run(transform, T, f"Fruit.transform T={T}", record_property, "walk", synchronising=True, loose=loose)


@gpu
@covers("fr_select_ranks_begin")
@pytest.mark.parametrize("T", TS)
def test_selection_begun_on_a_side_stream(nat, torch, abi, record_property, T):
    """``Selection`` begun on the side stream behind the producer of its block and ended from the
    default-stream context; ``select_ranks`` (synchronous) behind the same producer."""
    from oracle import ref_numpy as orc
    rows = 3
    A, wrong = draw(T, 1, "normal", (rows, N, T)), draw(T, 2, "normal", (rows, N, T))
    n = N * T
    jobs = [(r, inc, k) for r in range(rows) for inc in (0, 1, 2) for k in (0, n // 3, n // 2, n - 1)]
    jr, ji, jk = (list(v) for v in zip(*jobs))
    ref = np.array([np.sort(orc.pre_transform(A[r], inc).ravel())[k] for r, inc, k in jobs])
    want = torch.from_numpy(A).cuda()
    np.testing.assert_array_equal(nat.select_ranks(want, jr, ji, jk), ref)
    wrong_d = torch.from_numpy(wrong).cuda()
    nat.select_ranks(wrong_d.clone(), jr, ji, jk)        # (the scratch now holds the wrong block's passes)
    side = so.side_streams(1)[0]
    buf = wrong_d.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        so.delay(so.FLOOR_MS)
        buf.copy_(want)
        produced = torch.cuda.Event()
        produced.record()
        sel = nat.Selection(buf, jr, ji, jk)
        pending = not produced.query()
    got = sel.result()                                   # (the default-stream context)
    side.synchronize()
    record_property("Selection pending", pending)
    np.testing.assert_array_equal(got, ref)
    assert pending, "fr_select_ranks_begin returned only after its producer had finished"
    run(lambda b: torch.from_numpy(nat.select_ranks(b, jr, ji, jk)).cuda(), T, f"select_ranks T={T}",
        record_property, shape=(rows, N, T), synchronising=True)
    abi.expect("fr_select_ranks", "fr_select_ranks_begin")


# ------------------------------------------------------------------ backward
def _grad_cases(fr):
    from fruits_amd import nn
    W, S, V = fr.iss.weighting, fr.iss.semiring, fr.sieving
    words = [fr.words.SimpleWord(s) for s in ("[1]", "[1][2]", "[12][3]", "[1][2][3]")]
    ext = fr.ISSMode.EXTENDED
    sieves = lambda T: [V.END([T // 2, -1]), V.MAX([T // 3, -1], (-1, 0, 1)), V.MIN()]      # noqa: E731
    # (one weighting object per case, as a training loop holds one: the functional forms find
    # their ISS by it, and a new one per call would build - and destroy - a plan per call)
    indices, plateaus = W.Indices(), W.Plateaus(4)
    return {
        "iss": (lambda X, T: nn.iss(X, words, ext), "normal", ("fr_iss_backward",)),
        "max_iss_arctic": (lambda X, T: nn.max_iss(X, words, ext, semiring=S.Arctic()), "normal",
                           ("fr_iss_backward_max",)),
        "max_iss_bayesian": (lambda X, T: nn.max_iss(X, words, ext, semiring=S.Bayesian()), "uniform",
                             ("fr_iss_backward_max",)),
        "weighted_indices": (lambda X, T: nn.weighted_iss(X, words, ext, weighting=indices), "normal",
                             ("fr_iss_backward_weighted",)),
        "weighted_plateaus": (lambda X, T: nn.weighted_iss(X, words, ext, weighting=plateaus), "normal",
                              ("fr_iss_backward_weighted",)),
        "features": (lambda X, T: nn.iss_features(X, words, ext, sieves(T)), "normal",
                     ("fr_sieve_pick", "fr_iss_backward_picked")),
        "features_weighted": (lambda X, T: nn.iss_features(X, words, ext, sieves(T), weighting=indices),
                              "normal", ("fr_sieve_pick", "fr_iss_backward_picked")),
    }


GRAD_NAMES = ("iss", "max_iss_arctic", "max_iss_bayesian", "weighted_indices", "weighted_plateaus",
              "features", "features_weighted")


@gpu
@covers("fr_iss_backward", "fr_iss_backward_max", "fr_iss_backward_weighted", "fr_iss_backward_picked",
        "fr_sieve_pick", "fr_iss_run")
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", GRAD_NAMES)
def test_backward(fr, torch, abi, record_property, name, T):
    """Forward under the side stream on an ``X`` that is still being produced, the upstream gradient
    produced on that stream too, ``backward()`` called from the DEFAULT-stream context: autograd runs
    it on the forward's stream and ``stream_ptr()`` must see that.  Outputs and ``X.grad`` bit for
    bit those of the default-stream run."""
    forward, kind, entries = _grad_cases(fr)[name]
    shape_x = (9, D, T)
    X = draw(T, 1, kind, shape_x)
    probe = forward(torch.from_numpy(X).cuda(), T)
    shape_g = tuple(probe.shape)
    torch.cuda.synchronize()

    def call(xb, gb):
        x = xb.detach().requires_grad_(True)
        y = forward(x, T)
        side = torch.cuda.current_stream()
        with torch.cuda.stream(torch.cuda.default_stream()):
            y.backward(gb)
        # (autograd has ordered the caller's stream behind the backward pass; the side stream goes
        # on behind the caller's before X.grad is read there)
        side.wait_stream(torch.cuda.default_stream())
        return y.detach(), x.grad
    G = draw(T, 3, "normal", shape_g)
    want, report = so.behind_producer(call, [X, G], [draw(T, 2, kind, shape_x), draw(T, 4, "normal", shape_g)],
                                      what=f"nn {name} forward + backward T={T}")
    so.note(record_property, report)
    abi.expect("fr_iss_run", *entries)
    if name == "iss":       # the anchor: the derived bound of tests/test_grad_gpu.py
        import iss_bounds as ib
        import iss_grad_ref as gr
        strings = ["[1]", "[1][2]", "[12][3]", "[1][2][3]"]
        hp = gr.iss_grad(X, G, strings, "EXTENDED")
        A = gr.iss_grad(X, G, strings, "EXTENDED", magnitude=True)
        ib.check_bound(want[1], hp, A, gr.n_ops_grad(strings, T, "EXTENDED"), f"streams grad T={T}",
                       family="grad")


# ------------------------------------------------------------------ tables replaced in flight
def _quantile_tables(nat, monkeypatch, fruit_of, T):
    """(pipeline, its threshold table) of a fitted fruit: what ``_fused`` hands set_quantiles."""
    seen = []
    real = nat.Pipeline.set_quantiles

    def keep(self, quant):
        seen.append(np.array(quant, copy=True))
        return real(self, quant)
    monkeypatch.setattr(nat.Pipeline, "set_quantiles", keep)
    pipe = fruit_of.get_slice()._fused(T)
    monkeypatch.setattr(nat.Pipeline, "set_quantiles", real)
    assert pipe is not None and len(seen) == 1
    return pipe, seen[0]


@gpu
@covers("fr_pipeline_run")
@pytest.mark.parametrize("jit", ["0", "1"])
def test_set_quantiles_in_flight(fr, nat, torch, monkeypatch, record_property, jit):
    """fr_pipeline_set_quantiles (a re-fit's thresholds) while a run of the pipeline waits behind
    its producer: the queued run gives the OLD thresholds' features, the next one the new ones'.
    ``jit`` 0: the generic kernel reads the device table the setter rewrites; 1: the pipeline's own
    kernel holds the thresholds as immediates and is dropped."""
    monkeypatch.setenv("FRUITS_HIP_JIT", jit)
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    T = 1100
    X = draw(T, 1, "walk")
    fruit = _fruit(fr, *FUSED_MAKE(fr, "npi_mpi_end"), X)
    pipe, q_old = _quantile_tables(nat, monkeypatch, fruit, T)
    other = _fruit(fr, *FUSED_MAKE(fr, "npi_mpi_end"), draw(T, 3, "walk") * 2.0 + 0.5)
    _, q_new = _quantile_tables(nat, monkeypatch, other, T)
    assert q_old.shape == q_new.shape and not np.array_equal(q_old, q_new)
    lookup = fruit.get_slice().get_iss()[0].lookup_device(torch.from_numpy(X).cuda())
    torch.cuda.synchronize()

    def set_old():
        pipe.set_quantiles(q_old)
        if jit == "1":
            pipe.prepare(N)
    if jit == "1":
        set_old()
        if pipe.jit_loaded() == 0:
            pytest.skip("hipRTC is not installed")
    report = so.replaced_in_flight(lambda b: pipe.run(b, lookup), set_old, lambda: pipe.set_quantiles(q_new),
                                   [X], [draw(T, 2, "walk")], what=f"set_quantiles jit={jit}",
                                   loose=loose_columns(fruit))
    so.note(record_property, report)


@gpu
@covers("fr_pipeline_run")
def test_set_preparation_in_flight(fr, nat, torch, generic_kernels, record_property):
    """fr_pipeline_set_preparation: the same pipeline on the raw input (increments formed while
    staging) and then on an input it takes as prepared."""
    T = 1100
    X = draw(T, 1, "walk")
    fruit = _fruit(fr, [fr.preparation.INC()], fr.ISS(fr.words.of_weight(2, dim=3), mode=fr.ISSMode.EXTENDED),
                   [fr.sieving.NPI(), fr.sieving.END()], X)
    pipe = fruit.get_slice()._fused(T)
    assert pipe is not None and pipe.set_preparation(D, 1)
    report = so.replaced_in_flight(lambda b: pipe.run(b, None), lambda: pipe.set_preparation(D, 1),
                                   lambda: pipe.set_preparation(D), [X], [draw(T, 2, "walk")],
                                   what="set_preparation")
    so.note(record_property, report)


@gpu
@covers("fr_pipeline_run")
def test_set_lengths_in_flight(fr, nat, torch, generic_kernels, record_property):
    """fr_pipeline_set_series_cuts / fr_pipeline_set_lengths: a second ragged call with other
    lengths while the first is queued."""
    T = 1100
    X = draw(T, 1, "walk")
    V = fr.sieving
    fruit = _fruit(fr, [], fr.ISS(fr.words.of_weight(2, dim=3), mode=fr.ISSMode.EXTENDED),
                   [V.NPI(), V.PPV(quantile=[0.0, 0.5], constant=True), V.END()], X)
    slc = fruit.get_slice()
    pipe = slc._fused(T, ragged=True)
    assert pipe is not None
    first, second = _lengths(T), _lengths(T)[::-1].copy()

    def arm(lengths):
        slc._arm_lengths(pipe, lengths, nat.to_device(lengths.astype(np.int32), dtype=np.int32))
    report = so.replaced_in_flight(lambda b: pipe.run(b, None), lambda: arm(first), lambda: arm(second),
                                   [X], [draw(T, 2, "walk")], what="set_series_cuts / set_lengths")
    so.note(record_property, report)


@gpu
@covers("fr_iss_run")
def test_coswiss_set_dropout_in_flight(fr, nat, torch, record_property):
    """fr_coswiss_set_dropout: the mask of a re-fitted dropout CosWISS while a run is queued."""
    T = 1100
    X = draw(T, 1, "uniform")
    cw = ISS_CASES["coswiss_dropout"][0](fr)
    np.random.seed(1)
    cw.fit(X)
    old = cw._dropout_indices.copy()
    np.random.seed(2)
    cw.fit(X)
    new = cw._dropout_indices.copy()
    assert not np.array_equal(old, new)
    plan = cw._plan(0, len(cw.words))
    report = so.replaced_in_flight(lambda b: plan.run(b, None), lambda: nat.coswiss_set_dropout(plan, old, T),
                                   lambda: nat.coswiss_set_dropout(plan, new, T), [X], [draw(T, 2, "uniform")],
                                   what="coswiss_set_dropout")
    so.note(record_property, report)


@gpu
@covers("fr_pipeline_run")
def test_set_argmax_in_flight(fr, nat, torch, generic_kernels, record_property):
    """fr_pipeline_set_argmax is a construction-time setter: on a pipeline that has its thresholds
    the library refuses it (it would free the word table), so there is no replacing that table under
    a queued run - the refusal itself is held here, from the host while a run waits behind its
    producer, and the queued run and the one after it give the one result."""
    T = 1100
    X = draw(T, 1, "walk")
    fruit = _fruit(fr, *FUSED_MAKE(fr, "arctic_argmax"), X)
    slc = fruit.get_slice()
    pipe = slc._fused(T)
    assert pipe is not None
    lens = np.array([len(w) for w in slc.get_iss()[0].words], dtype=np.int32)

    def again():
        with pytest.raises(ValueError, match="before fr_pipeline_set_quantiles"):
            nat.check(nat.lib().fr_pipeline_set_argmax(pipe._h, C.c_int32(len(lens)),
                                                       lens.ctypes.data_as(C.POINTER(C.c_int32))),
                      "fr_pipeline_set_argmax")
    report = so.replaced_in_flight(lambda b: pipe.run(b, None), again, again, [X], [draw(T, 2, "walk")],
                                   what="set_argmax", distinct=False, loose=loose_columns(fruit))
    so.note(record_property, report)


# ------------------------------------------------------------------ one object, two streams
@gpu
@covers("fr_iss_run", "fr_pipeline_run", "fr_prep_fir", "fr_sieve", "fr_iss_backward")
@pytest.mark.parametrize("T", TS)
def test_one_object_two_streams(fr, nat, torch, generic_kernels, record_property, T):
    """Two inputs through the SAME object on two side streams, enqueued alternately: all per-call
    state lives in the caller's workspace, so each result is that input's own serial result."""
    from fruits_amd import nn
    V = fr.sieving
    a, b, wrong = draw(T, 1, "walk"), draw(T, 3, "walk"), draw(T, 2, "walk")
    iss = fr.ISS(fr.words.of_weight(2, dim=3), mode=fr.ISSMode.EXTENDED, weighting=fr.iss.weighting.Indices())
    plan = iss._plan(0, len(iss.words))
    lookup = iss.lookup_device(torch.from_numpy(a).cuda())
    fruit = _fruit(fr, [], iss.copy(), [V.NPI(q=(0.5, 1.0)), V.MPI(q=(0.5, 1.0)), V.END()], a)
    pipe = fruit.get_slice()._fused(T)
    assert pipe is not None
    wb = int(nat.lib().fr_pipeline_workspace_bytes(pipe._h, N, 1)) + 1
    rin = _fitted(fr.preparation.RIN(5), a.shape, 2)
    sv = V.NPI([T // 3, -1], (-1, 0, 1), 1)
    torch.cuda.synchronize()

    def piped(x):       # (per-call work=: a workspace of the call's own, from the call's stream)
        return pipe.run(x, lookup, work=torch.empty(wb, dtype=torch.uint8, device=x.device))

    def sieved(x):
        out = torch.zeros((N, sv.nfeatures()), dtype=torch.float64, device=x.device)
        sv.transform_device(x[:, 0, :], out, 0)
        return out

    def grad(x):
        xr = x.detach().requires_grad_(True)
        y = nn.iss(xr, fr.words.of_weight(2, dim=3), fr.ISSMode.EXTENDED)
        y.backward(torch.cos(y.detach()))
        return y.detach(), xr.grad
    for what, call, loose in (("Plan.run", lambda x: plan.run(x, lookup), None),
                              ("Pipeline.run", piped, loose_columns(fruit)),
                              ("RIN", lambda x: rin._transform_device(x), None),
                              ("NPI", sieved, None),
                              ("nn.iss forward + backward", grad, None)):
        _, _, report = so.two_streams(call, [a], [b], [wrong], what=f"{what} on two streams T={T}", loose=loose)
        so.note(record_property, report)
