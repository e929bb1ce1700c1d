"""Every fused walk family against the derived elementwise bound of tests/iss_bounds.py.

``Fruit.transform`` runs one fused launch per slice; the rows are never written, so they are read
through sieves: ``END`` at the cuts ``probe_positions(T) + 1`` (every position where the parts of a
scan meet), and the sum- and selection-valued features the fused epilogue forms itself - ``MAX``,
``MIN``, ``MPI(inc=0)``, ``MPI(inc=1)`` over [0, T//3) and [T//3, T) - with OPEN bands: the
thresholds of the fitted sieve copies are overwritten with (-2 max A, +2 max A), so that every
element takes part on both sides and no exposure rule is needed.  What a feature is compared with
and the bound on the difference come from ``iss_bounds.feature_reference``: long-double oracle
runs on the CPU, no measured number.

The pattern of ``test_pieces_within_bound``: a fruit fitted on the normal input
(``np.random.seed(4)``), ``slc._fused(T)``, ``pipe.run(Xd, iss.lookup_device(Xd))`` as
``Fruit.transform`` runs it, the device's own lookup read back for the oracle, the family asserted
from ``pipe.last_launch()``.  64 series, a zero-mean and a positive input, the five weightings.

Families (``_native.WALK_FAMILIES``): ``fused`` - the generic record loop of walk_fused.h, one
group per series and the host's own choice of several, its TOTALINC and HIGHORD instances, INC
fused into the staging; ``fused_packed`` - the wave-per-series kernel; ``fused_jit`` - the
pipeline's own run-time compiled kernel with the sieves as immediates, with the plan as
straight-line code (fwalk_static) and with the node shapes of a large plan (fwalk_shaped); the fused
CosWISS pipelines, cooperative and wave per unit.  The largest err / bound per family is printed at
the end (``ISS-RATIO fused...``)."""
import hashlib
from collections import OrderedDict

import numpy as np
import pytest

import iss_bounds as ib
from oracle import ref_numpy as orc
from test_hip_parity import make_weighting

pytestmark = pytest.mark.gpu
N_SERIES = 64
BAND_KINDS = ("MAX", "MIN", "MPI0", "MPI1")
Q_FITTED = (0.1, 0.9)            # (any fitted pair: the thresholds are overwritten after the fit)


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    yield fruits_amd
    _ORACLE.clear()
    ib.print_ratios()


@pytest.fixture(scope="module")
def hiprtc(fr):
    """Skips the tests of run-time compiled kernels where hipRTC is not installed - asked once,
    before any of their work: a program that then fails to compile or load is a failure."""
    from test_hip_parity import _require_hiprtc
    strs = ib.FAMILY_WORDS["static_jit"][1]
    plan = fr.ISS([fr.words.SimpleWord(s) for s in strs], mode=fr.ISSMode.EXTENDED)._plan(0, len(strs))
    assert plan.static_schedule(1) is not None
    _require_hiprtc(plan)


def _env(monkeypatch, **knobs):
    """No kernel of a pipeline's own unless the test asks for it; the FRUITS_HIP_DEBUG knobs."""
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    monkeypatch.setenv("FRUITS_HIP_DEBUG", ",".join(f"{k}={v}" for k, v in knobs.items()))


# ------------------------------------------------------------------ the oracle, paid once
# (hp, A, n) does not depend on the family: keyed by what it is computed from.  Cases that share
# a key follow each other (the variant is the innermost parameter), so a few entries suffice; the
# oldest go once the long doubles held pass _ORACLE_BYTES.
_ORACLE = OrderedDict()
_ORACLE_BYTES = 768 << 20


def _held(entry):
    hp, A, _ = entry
    return hp.nbytes + (0 if A is hp else A.nbytes)


def _oracle(words, T, dist, weighting, lookup, compute):
    digest = None if lookup is None else hashlib.sha1(np.ascontiguousarray(lookup).tobytes()).hexdigest()
    key = (tuple(words), T, dist, weighting, digest)
    if key in _ORACLE:
        _ORACLE.move_to_end(key)
        return _ORACLE[key]
    _ORACLE[key] = compute()
    while len(_ORACLE) > 1 and sum(_held(v) for v in _ORACLE.values()) > _ORACLE_BYTES:
        _ORACLE.popitem(last=False)
    return _ORACLE[key]


# ------------------------------------------------------------------ one fused pipeline, held to the bound
def _open_bands(slc, band):
    """The thresholds of every fitted sieve copy of the slice overwritten with ``band`` (as
    test_hip_parity.transplant_thresholds does with the oracle's): a band that takes every
    element.  The fused pipelines are built again from the copies."""
    from fruits_amd.fruit import _leaf
    n = 0
    for row in slc._sieves_extended:
        for sv in row:
            leaf = _leaf(sv)
            if leaf.requires_fitting:
                assert len(leaf._quantiles) == 2
                leaf._quantiles = band.copy()
                n += 1
    assert n > 0
    slc._fused_cache = {}


class _Case:
    """A fitted fruit of one ISS under the sieves of the module, its inputs, the device's own
    lookups and the oracles.  Sieves: END at the probe cuts; of ``kinds`` MAX, MIN, MPI(inc=0),
    MPI(inc=1) over [0, T//3) and [T//3, T), each with one fitted band that is then opened;
    ``extra_inc``: a counting sieve NPI(inc=extra_inc) behind them - its counts are not asserted,
    it selects the kernel instance."""

    def __init__(self, fr, iss, D, T, words, weighting, N=N_SERIES, kinds=BAND_KINDS, extra_inc=None,
                 inc_prep=False, coswiss=None):
        from fruits_amd import _native as nat
        from fruits_amd.cache import SharedSeedCache
        self.nat, self.D, self.T, self.N, self.kinds = nat, D, T, N, tuple(kinds)
        dists = ("positive", "zero_mean") if coswiss else ("normal", "uniform")
        draw = (lambda d: ib.coswiss_input(d, N, T)) if coswiss else (lambda d: ib.reals_input(d, N, D, T))
        sv = fr.sieving
        self.cuts = [p + 1 for p in ib.probe_positions(T)]
        self.cut = [T // 3, -1]
        make = {"MAX": lambda: sv.MAX(cut=self.cut, q=Q_FITTED), "MIN": lambda: sv.MIN(cut=self.cut, q=Q_FITTED),
                "MPI0": lambda: sv.MPI(cut=self.cut, q=Q_FITTED, inc=0),
                "MPI1": lambda: sv.MPI(cut=self.cut, q=Q_FITTED, inc=1)}
        sieves = [sv.END(cut=self.cuts)] + [make[k]() for k in self.kinds]
        if extra_inc is not None:
            sieves.append(sv.NPI(inc=extra_inc))
        self.per_sum = len(self.cuts) + 2 * len(self.kinds) + (extra_inc is not None)
        fruit = fr.Fruit("fused bounds")
        if inc_prep:
            fruit.add(fr.preparation.INC)
        fruit.add(iss)
        fruit.add(*sieves)
        self.slc = slc = fruit.get_slice()
        slc.fit_sample_size = 1.0
        np.random.seed(4)
        fruit.fit(draw(dists[0]))
        self.iss = slc._iss[0]
        # the inputs, the device's own lookups and the oracles of both distributions first: the
        # open band has to take every element of both
        self.runs = []
        for dist in dists:
            X = draw(dist)
            cache = SharedSeedCache(X)
            Xd = cache.input_device(X)
            slc._attach(cache)                   # (the weighting reads the raw input from the cache)
            lk = None if coswiss else self.iss.lookup_device(Xd)
            lk_host = None if lk is None else nat.to_host(lk)
            P = orc.inc_transform(X) if inc_prep else X
            if coswiss:
                freqs, exponent, total = coswiss
                ref = _oracle(words, T, dist, ("coswiss", tuple(freqs), exponent, total, N), None,
                              lambda: ib.coswiss_reference(P, words, freqs, exponent, total))
            else:
                spec = ib.WEIGHTINGS[weighting]
                total = bool(spec and spec.get("total", False))
                ref = _oracle(words, T, dist, (weighting, N, inc_prep), lk_host,
                              lambda: ib.reals_reference(P, words, "EXTENDED", None, lk_host, total))
            self.runs.append((dist, cache, Xd, lk, ref))
        if self.kinds:
            _open_bands(slc, ib.open_band(np.array([float(np.max(r[4][1])) for r in self.runs])))
        self.pipe = slc._fused(T)
        assert self.pipe is not None
        self._refs = {}

    def features(self, feats):
        """{kind: (K, N, C)} of the (N, K * per_sum) features of a run, in sieve order."""
        K, nE = self.pipe.rows, len(self.cuts)
        assert feats.shape == (self.N, K * self.per_sum), (feats.shape, K, self.per_sum)
        rows = feats.reshape(self.N, K, self.per_sum).transpose(1, 0, 2)
        out = {"END": rows[:, :, :nE]}
        for i, kind in enumerate(self.kinds):
            out[kind] = rows[:, :, nE + 2 * i:nE + 2 * i + 2]
        return out

    def check(self, what, family, launch, groups=0, precondition=True):
        """Runs the pipeline on both inputs the way ``Fruit.transform`` does and holds every
        feature to its bound; ``launch(last_launch)`` asserts the kernel that ran."""
        for dist, cache, Xd, lk, (hp, A, n) in self.runs:
            self.slc._attach(cache)
            feats = self.nat.to_host(self.pipe.run(Xd, lk, groups=groups))
            launch(self.pipe.last_launch())
            where = f"{what} {dist}"
            if dist == "uniform" and precondition:
                assert ib.positive_precondition(hp, A) <= 1.0, where
            assert hp.shape[0] == self.pipe.rows, where
            for kind, got in self.features(feats).items():
                if (dist, kind) not in self._refs:        # (the same for every launch of the case)
                    self._refs[dist, kind] = ib.feature_reference(kind, hp, A, n,
                                                                  self.cuts if kind == "END" else self.cut)
                ib.check_features(got, *self._refs[dist, kind], f"{where} {kind}", family)


def _reals_case(fr, D, strs, T, weighting, **kw):
    iss = fr.ISS([fr.words.SimpleWord(s) for s in strs], mode=fr.ISSMode.EXTENDED,
                 weighting=make_weighting(fr, ib.WEIGHTINGS[weighting]))
    return _Case(fr, iss, D, T, strs, weighting, **kw)


def _is_total(weighting):
    return bool((ib.WEIGHTINGS[weighting] or {}).get("total", False))


def _ran(family, **fields):
    """An assertion on ``last_launch()``: the family and, as values or predicates, other fields."""
    def check(ran):
        assert ran["family"] == family, ran
        for k, v in fields.items():
            assert (v(ran[k]) if callable(v) else ran[k] == v), (k, ran)
    return check


# ------------------------------------------------------------------ fused: the generic record loop
# extra: None - the sieve set; 1 - plus NPI(inc=1) (a differencing count: on a totally weighted
# plan the TOTALINC instance, which MPI(inc=1) asks for as well); 3 - plus NPI(inc=3): the HIGHORD
# instance, five carry slots per node.  The multi-chunk lengths take the extras.
FUSED_CASES = [(T, w, e) for T in ib.LENGTHS for w in ib.WEIGHTINGS
               for e in ((None, 1, 3) if T in (1025, 3000) else (None,))]


@pytest.mark.parametrize("T,weighting,extra", FUSED_CASES, ids=lambda v: str(v))
def test_fused_within_bound(fr, monkeypatch, T, weighting, extra):
    """walk_fused.h's record loop (no kernel of the pipeline's own: FRUITS_AMD_AUTO_PREPARE=0;
    packed=0 keeps it on short series): whole series (groups=1) and the host's own choice, which
    for 64 series is several groups per series - chunk carries in LDS from T = 1025 on."""
    _env(monkeypatch, packed=0)
    case = _reals_case(fr, *ib.FAMILY_WORDS["lean"], T, weighting, extra_inc=extra)
    assert case.pipe.jit_loaded() == 0 and case.pipe.pieces_loaded() == 0
    what = f"fused T={T} {weighting} extra={extra}"
    case.check(what + " G=1", "fused", _ran("fused", G=1), groups=1)
    case.check(what + " G=host", "fused", _ran("fused", G=lambda g: g > 1))


@pytest.mark.parametrize("weighting", ["none", "indices_total", "l1"])
def test_fused_inc_in_the_staging(fr, monkeypatch, weighting):
    """INC formed while the launch stages the RAW rows (fr_pipeline_set_preparation), two chunks:
    the pipeline is handed the raw input, the oracle the float64 INC(X) (one subtraction per
    element: the same on both sides)."""
    _env(monkeypatch, packed=0)
    T = 1025
    # (the zero-padded first increment is 0: the words that divide by a letter stay out)
    D, strs = ib.FAMILY_WORDS["lean"]
    case = _reals_case(fr, D, [s for s in strs if "-" not in s], T, weighting, inc_prep=True)
    chain = case.slc._fusable_preparation(T)
    assert chain is not None and chain[0] == 1
    assert case.pipe.set_preparation(case.D, *chain)
    assert case.pipe.raw_dims == case.D != 0               # the raw input goes in
    # (U[0, 1) differenced is no positive input: no precondition to state)
    case.check(f"fused INC T={T} {weighting}", "fused_inc_staged", _ran("fused"), precondition=False)


# ------------------------------------------------------------------ fused_packed: a wave per series
PACKED_LENGTHS = (1, 2, 63, 128, 129, 256, 300)


def _packed_admits(T, strs):
    """launch_choice.h packed_supported for a word set."""
    levels = max(len(orc.parse_word(s)) for s in strs)
    return (T <= 256 and levels <= 8) or (T <= 384 and levels <= 4)


@pytest.mark.parametrize("weighting", list(ib.WEIGHTINGS))
@pytest.mark.parametrize("T", [T for T in PACKED_LENGTHS if _packed_admits(T, ib.FAMILY_WORDS["packed"][1])])
def test_fused_packed_within_bound(fr, monkeypatch, T, weighting):
    """walk_packed.h under sieves: one, two and three pieces of 128 elements per wave.  A totally
    weighted plan under a differencing sieve is the cooperative kernel's alone (launch_choice.h
    walk_is_packed; test_fused_within_bound runs that combination at these lengths too), so under
    a total weighting this family is held to END, MAX, MIN and MPI(inc=0)."""
    _env(monkeypatch)
    kinds = BAND_KINDS[:3] if _is_total(weighting) else BAND_KINDS
    case = _reals_case(fr, *ib.FAMILY_WORDS["packed"], T, weighting, kinds=kinds)
    case.check(f"fused_packed T={T} {weighting}", "fused_packed", _ran("fused_packed"))


# ------------------------------------------------------------------ fused_jit: the pipeline's own kernel
JIT_LENGTHS = (63, 300, 1024, 1025, 3000)


# (the two variants of a case follow each other: they share its oracle)
JIT_CASES = [(T, w, v) for T in JIT_LENGTHS for w in ib.WEIGHTINGS for v in ("immediates", "static")]


@pytest.mark.parametrize("T,weighting,variant", JIT_CASES, ids=lambda v: str(v))
def test_fused_jit_within_bound(fr, hiprtc, monkeypatch, T, weighting, variant):
    """The fused walk compiled for its pipeline (hipRTC).  ``immediates``: the sieves' kinds,
    orders, shapes and cuts as constants, the plan still decoded record by record (fused_static=0,
    ``prepare(N, plan_too=False)``); ``static``: the plan as straight-line code as well
    (fwalk_static).  packed=0: short series have no kernel of their own otherwise."""
    _env(monkeypatch, packed=0, **({"fused_static": 0} if variant == "immediates" else {}))
    case = _reals_case(fr, *ib.FAMILY_WORDS["interpreter"], T, weighting)
    pipe = case.pipe
    assert pipe.jit_loaded() == 0 and pipe.plan.nodes <= 128
    pipe.prepare(N_SERIES, plan_too=variant == "static")
    assert pipe.jit_loaded() >= 1, "the pipeline's own kernel did not compile or load"
    assert pipe.jit_loaded(static_only=True) == (1 if variant == "static" else 0)
    assert pipe.pieces_loaded() == 0
    case.check(f"fused_jit {variant} T={T} {weighting}", f"fused_jit_{variant}", _ran("fused_jit"))


# every fourth word of test_fused_kernel_compiled_for_its_pipeline[large_plan]'s set and its last:
# 146 nodes, 146 rows (all 281 words: 398 rows, ten seconds of long-double oracle per case)
LARGE_PLAN = orc.of_weight_strings(5, 2)[::4] + ["[1][-2][11][2]"]


@pytest.mark.parametrize("T", [300, 1025])
@pytest.mark.parametrize("weighting", ["indices", "indices_total"])
def test_fused_jit_shaped_within_bound(fr, hiprtc, monkeypatch, weighting, T):
    """A plan of more than 128 nodes that is NOT cut into pieces (pieces=0): its own kernel knows the
    node shapes (fwalk_shaped), the records still come from the table.  16 series."""
    _env(monkeypatch, packed=0, pieces=0)
    case = _reals_case(fr, 2, LARGE_PLAN, T, weighting, N=16)
    pipe = case.pipe
    assert pipe.plan.nodes > 128 and pipe.jit_loaded() == 0
    pipe.prepare(16)
    assert pipe.pieces_loaded() == 0
    assert pipe.jit_loaded(static_only=True) == 1, "the pipeline's own kernel did not compile or load"
    case.check(f"fused_jit shaped T={T} {weighting}", "fused_jit_shaped", _ran("fused_jit"))


# ------------------------------------------------------------------ fused CosWISS
N_COS = 6        # (test_coswiss_within_bound's: the oracle evaluates the (S+1)^L expanded terms one by one)
COS_FUSED = [(p, e, T) for T in (100, 450, 1030, 2051) for e in (1, 2, 6) for p in ((0, 1) if T <= 384 else (0,))]


@pytest.mark.parametrize("packed,exponent,T", COS_FUSED, ids=lambda v: str(v))
def test_fused_coswiss_within_bound(fr, monkeypatch, packed, exponent, T):
    """CosWISS under sieves in one launch (coswiss.h with the fused epilogue), the cooperative and
    the wave-per-unit kernel (T <= 384 unless the knob says 0, capi_walk.cpp run_coswiss), total
    weighting and not; the rows read through END at the probe cuts.  A CosWISS launch leaves no
    record (``last_launch`` is the trie walk's): asserted is that none was left - the pipeline did
    not run a trie walk - and the family a ratio is recorded under is the knob's."""
    _env(monkeypatch, packed=packed)
    words = ib.coswiss_words(T, exponent)
    family = "fused_coswiss_packed" if packed else "fused_coswiss_cooperative"
    for total in (False, True):
        cw = fr.CosWISS([fr.words.SimpleWord(s) for s in words], ib.COS_FREQS, exponent=exponent,
                        total_weighting=total)
        case = _Case(fr, cw, 2, T, words, None, N=N_COS, kinds=(), coswiss=(ib.COS_FREQS, exponent, total))
        assert case.pipe.plan.rows == len(words) * len(ib.COS_FREQS)
        case.check(f"{family} exponent={exponent} T={T} total={total}", family, _ran(None),
                   precondition=False)
