"""Per-series lengths at batch sizes and on seeds the small tests do not reach.

A. Every series of every fused launch shape of test_walk_batch.py (``FUSED``), through the ragged
   pipeline: N follows the resident round R of a ragged probe launch, the lengths sit at the edges of
   the kernel family (a wave of 64, the packed limit, the chunks of 256 / 512, T - 1, T) and are
   dealt over the series by a seeded permutation.  The input is small integers, so every iterated
   sum is an exact integer in any association and ALL N rows are compared bit for bit with the dense
   call on the truncated sub-batch of their length class - another T, usually another kernel
   family, no cut table.  One series per class, the last series and the first of the second round
   are anchored to the numpy oracle (``oracle_features``).  The oracle knows NPI, MPI, XPI, MAX, MIN
   and END: these columns are compared, exactly; CUR, PPV and CPV are held by the dense call alone.
   None of the sieves of ``launch_sieves`` is fitted (their bands are (0, inf], (-inf, inf] and
   constants), so both sides have the same thresholds by construction.

   A sixth shape takes the knobs that cut a DENSE pipeline of this plan into pieces.  A ragged
   pipeline names per-series cut slots and therefore has no run-time compiled kernel, pieces
   included (``jit_uniform`` in csrc/capi_pipeline.cpp): the case asserts that the
   plan has a cover of pieces, that the ragged launch nevertheless took the generic ``fused``
   instance with no piece loaded, and checks all N series of it like the others.

   Rounds: series n of a launch with G groups per series lies in round ``n * G // R``.  Every round
   of at least four series per class holds every class (asserted); the one series of the partial
   last round of N = 2 R + 1 is given a length below T and is one of the oracle's anchors.  A launch
   of one round (two groups at N = 261 / 264, the wave-per-series kernel, the sixth shape) is
   asserted by thirds of the batch instead.

B. Every slice of ``_supported()`` of test_lengths_host.py - the list the host gate is tested on -
   is run on the device, as it is (LPI: materialising) and without LPI (fused).  The rule, read from
   the seeds: a slice whose preparateurs contain an ``STD`` or whose ISS has a weighting is
   REAL-VALUED, every other one is EXACT (integer rows from integer input).  Exact slices keep their
   whole band of sieves and are compared bit for bit on every column; real-valued ones take the
   unbounded form of every band sieve (``q = (-1, 1)``; PPV / CPV left out - a fitted or constant
   threshold may tie under another association), their counting columns (NPI, LPI) equal the
   reference's and the segment length that length and cut imply, the others meet the project's bar
   rtol 1e-6 / atol 1e-9.  Two different tails give the same bits, and so do tails of +-1e160 -
   but for the band sums (MPI, CUR, AVG, STD) of a real-valued slice on a workgroup-per-unit
   launch, which do not give the same bits for the same input twice (the comment in the test).

C. Tails of +-1e160: finite, their products are not, their sums are ``inf - inf``.

D. Small surface cases.

Seconds per case are printed (``lengths_batch ...``)."""
import time

import numpy as np
import pytest

from test_hip_parity import oracle_features, sieve_kinds
from test_lengths_gpu import (LAUNCH_SHAPES, int_input, launch_fruit, launch_sieves, per_series,
                              real_input, spread, with_tails)
from test_lengths_host import _supported
from test_walk_batch import FUSED, _words

pytestmark = pytest.mark.gpu

PACKED_CLASSES = [1, 2, 3, 5, 63, 64, 65, 128, 129, 199, 200]


def chunked_classes(T):
    return [4, 255, 256, 257, 511, 512, 513, T - 1, T]


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


# ------------------------------------------------------------------------------ A: launch shapes
def deal(classes, N, seed, tail_from=None):
    """N lengths: the classes in equal shares, dealt by a seeded permutation (a period would match
    a group or XCD count).  The series from ``tail_from`` on (a partial last round too small to
    hold every class) take the classes below the largest in turn."""
    classes = np.asarray(classes, dtype=np.int64)
    rng = np.random.default_rng(seed)
    lengths = classes[rng.permutation(N) % len(classes)]
    if tail_from is not None and tail_from < N:
        short = rng.permutation(classes[classes < classes.max()])
        lengths[tail_from:] = np.resize(short[short > 3], N - tail_from)
    return lengths


def rounds_of(N, G, R):
    """The round of workgroups series n of a launch with G groups per series starts in."""
    return np.arange(N) * G // R


def parts_of(N, G, R, packed):
    """The parts of the batch every class has to occur in: the rounds of the launch, or thirds of
    the batch for a launch of one round and for the wave-per-series kernel."""
    rounds = rounds_of(N, G, R)
    if packed or rounds.max() == 0:
        return np.arange(N) * 3 // N
    return rounds


def check_deal(lengths, classes, parts):
    """Every part of at least four series per class holds every class; fewer than a quarter of
    the neighbours share a length."""
    full = 0
    for p in np.unique(parts):
        here = lengths[parts == p]
        if len(here) >= 4 * len(classes):
            assert set(here.tolist()) == set(classes), (p, sorted(set(classes) - set(here.tolist())))
            full += 1
    assert full >= 2, (full, np.bincount(parts))
    assert (lengths[1:] == lengths[:-1]).mean() < 0.25


def batch_fruit(fr, words, extra=()):
    fruit = fr.Fruit("ragged batch")
    fruit.add(fr.ISS(words, mode=fr.ISSMode.EXTENDED))
    fruit.add(*launch_sieves(fr), *extra)
    fruit.get_slice().fit_sample_size = 1.0
    return fruit


ORACLE_SIEVES = [{"kind": "NPI"}, {"kind": "NPI", "inc": 2}, {"kind": "MPI", "cut": [3, -1]}, {"kind": "XPI"},
                 {"kind": "MAX"}, {"kind": "MIN", "cut": [-3, -1]}, {"kind": "END"}]
ORACLE_KINDS = ("NPI", "MPI", "XPI", "MAX", "MIN", "END")


def first_difference(got, want, what, N):
    ne = got != want
    if ne.any():
        n, c = np.argwhere(ne)[0]
        print(f"lengths_batch {what}: first difference at series {n}, column {c}; "
              f"{int(ne.any(axis=1).sum())} of {N} series differ")
    return not ne.any()


def ragged_batch(fr, monkeypatch, name, words, D, T, classes, n_of, want=None, env=None, extra=(),
                 packed=False, pieces=False):
    """One case of A; ``want``: the launch record the ragged pipeline has to name, None for a
    slice that materialises."""
    t0 = time.perf_counter()
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    fruit = batch_fruit(fr, words, extra)
    slc = fruit.get_slice()
    np.random.seed(5)
    fruit.fit(int_input(1, (24, D, T)))                           # dense, 24 series
    labels = [fruit.label(i) for i in range(fruit.nfeatures())]
    pipe = slc._fused(T, ragged=True)
    assert (pipe is not None) == (want is not None)
    # the probe: 8 series through the RAGGED pipeline
    probe = None
    if pipe is not None:
        fruit.transform(int_input(2, (8, D, T)), lengths=np.asarray(classes[-8:]))
        assert slc._fused(T, ragged=True) is pipe
        probe = pipe.last_launch()
    N = int(n_of(probe))
    expect = {} if want is None else want(N, probe)
    G = int(expect.get("G", 1))                  # (the groups per series the case is about)
    R = int((probe or {}).get("resident") or N)
    rounds = rounds_of(N, G, R)
    small_tail = None
    if not packed and rounds.max() > 0 and (rounds == rounds.max()).sum() < 4 * len(classes):
        small_tail = int(np.argmax(rounds == rounds.max()))
    lengths = deal(classes, N, len(name), tail_from=small_tail)
    X = int_input(len(name) + N, (N, D, T))
    X1 = with_tails(X, lengths, 1)
    got = fruit.transform(X1, lengths=lengths)
    assert got.shape == (N, fruit.nfeatures()) and np.isfinite(got).all()
    # (1) the branch
    ran = None
    if pipe is not None:
        ran = pipe.last_launch()
        assert {k: ran[k] for k in expect} == expect, (name, N, ran)
        assert pipe.jit_loaded() == 0 and pipe.pieces_loaded() == 0
        if pieces:
            cover = pipe.plan.pieces(8)
            assert cover is not None and len(cover["types"]) >= 2
        if not packed:
            G = int(ran["G"])
            rounds = rounds_of(N, G, R)
    check_deal(lengths, classes, parts_of(N, G, R, packed))
    # (2) every series against the dense call on the truncated sub-batch of its class
    ref = np.full_like(got, np.nan)
    for L in classes:
        idx = np.flatnonzero(lengths == L)
        ref[idx] = fruit.transform(np.ascontiguousarray(X[idx, :, :L]))
    assert first_difference(got, ref, name, N), (name, N)
    np.testing.assert_array_equal(got, ref)
    # (3) the oracle: one series per class, the last one, the first of the second round
    anchors = {int(np.flatnonzero(lengths == L)[0]) for L in classes} | {N - 1}
    second = np.flatnonzero(rounds == 1)
    if len(second):
        anchors.add(int(second[0]))
    cols = np.isin(sieve_kinds(labels), ORACLE_KINDS)
    spec = {"slices": [{"iss": [{"words": [str(w) for w in words], "mode": "EXTENDED"}],
                        "sieves": ORACLE_SIEVES}]}
    for n in sorted(anchors):
        Xn = np.ascontiguousarray(X[n:n + 1, :, :lengths[n]])
        want_n, _ = oracle_features(spec, Xn, Xn, np_seed=0)
        np.testing.assert_array_equal(got[n, cols], want_n[0], err_msg=f"{name} series {n} L={lengths[n]}")
    # (4) other tails, the same bits
    again = fruit.transform(with_tails(X, lengths, 2), lengths=lengths)
    assert first_difference(again, got, name + " tails", N), (name, N)
    # (5) the lengths act: a short series is not its padded self ...
    dense = fruit.transform(X1)
    short = lengths < T
    acted = (got != dense).any(axis=1)
    assert acted[short].all(), (name, np.flatnonzero(short & ~acted)[:10])
    np.testing.assert_array_equal(got[~short], dense[~short])
    # ... and series of one and the same (nowhere zero) data have the row of their class: equal
    # inside a class, different between any two
    base = np.where(X[:1] == 0, 1.0, X[:1])
    same = fruit.transform(with_tails(np.repeat(base, N, axis=0), lengths, 3), lengths=lengths)
    rows = {}
    for L in classes:
        idx = np.flatnonzero(lengths == L)
        assert (same[idx] == same[idx[0]]).all(), (name, L)
        rows[L] = same[idx[0]].tobytes()
    assert len(set(rows.values())) == len(classes), name
    print(f"lengths_batch {name}: N={N} T={T} R={R} ran={ran} anchors={len(anchors)} "
          f"seconds={time.perf_counter() - t0:.2f}")


@pytest.mark.parametrize("name", list(FUSED))
def test_fused_shapes(fr, monkeypatch, name):
    case = FUSED[name]
    which, T = case["which"], case["T"]
    packed = name == "fused_packed"
    ragged_batch(fr, monkeypatch, name, _words(fr, which), 3 if which == "P23" else 2, T,
                 PACKED_CLASSES if packed else chunked_classes(T), case["n_of"], case["want"],
                 env=case.get("env"), packed=packed)


def test_fused_under_the_pieces_knobs(fr, monkeypatch):
    """The knobs of test_pieces_within_bound on of_weight(4, 2) (115 nodes): a dense pipeline of
    this plan runs in pieces, the ragged one on the generic instance (module docstring)."""
    ragged_batch(fr, monkeypatch, "fused_pieces_knobs", _words(fr, "P42"), 2, 700, chunked_classes(700),
                 lambda p: 203, lambda N, p: dict(family="fused", persistent=0),
                 env={"FRUITS_HIP_DEBUG": "pieces=1,piece_min=30,piece_nodes=8,packed=0"}, pieces=True)


def test_materialising_batch(fr, monkeypatch):
    """LPI: the slice materialises - ``fr_sieve`` with N cut rows, ``fr_sieve_implicit_lengths``
    over a grid of N."""
    ragged_batch(fr, monkeypatch, "materialising", fr.words.of_weight(2, dim=2), 2, 700,
                 chunked_classes(700), lambda p: 300, None, extra=[fr.sieving.LPI()], packed=True)


# ------------------------------------------------------------------------------ B: the gate's list
SLICES = _supported()
B_SHAPE = (12, 2, 300)
B_CLASSES = [1, 2, 3, 5, 64, 65, 128, 129, 255, 256, 257, 300]
SUMMED = ("MPI", "CUR", "AVG", "STD")      # band sums of real numbers: wave partials, arrival order


def _inner_preps(prep):
    yield prep
    inner = getattr(prep, "_preparateur", None)
    if inner is not None:
        yield from _inner_preps(inner)


def is_real_valued(slc):
    """The rule of section B: an STD preparateur (wrapped ones too) or a weighting."""
    std = any(type(q).__name__ == "STD" for p in slc._preparateurs for q in _inner_preps(p))
    return std or any(iss.weighting is not None for iss in slc._iss)


def _leaf(sv):
    while hasattr(sv, "_sieve"):
        sv = sv._sieve
    return sv


def _describe(slc):
    preps = "+".join(">".join(type(q).__name__ for q in _inner_preps(p)) for p in slc._preparateurs) or "-"
    iss = slc._iss[0]
    weighting = "-" if iss.weighting is None else type(iss.weighting).__name__ + (
        "(total)" if getattr(iss.weighting, "_total", getattr(iss.weighting, "total", False)) else "")
    return f"{preps}|{type(iss.semiring).__name__}|{weighting}|{iss.mode.name}"


def sieves_of(slc, real, lpi):
    """Copies of the slice's sieves: all of them for an exact slice; for a real-valued one the
    unbounded form of every band sieve, PPV / CPV left out.  ``lpi=False``: without LPI."""
    out = []
    for sv in slc._sieves:
        kind = type(_leaf(sv)).__name__
        if kind == "LPI" and not lpi:
            continue
        if real and kind in ("PPV", "CPV"):
            continue
        sv = sv.copy()
        if real and kind != "END":
            _leaf(sv)._q = (-1.0, 1.0)
        out.append(sv)
    return out


def column_map(slc):
    """Per feature column of a slice: (kind of the leaf sieve, the sieve, feature within it)."""
    cols = []
    for _ in range(slc.niteratedsums()):
        for sv in slc._sieves:
            cols += [(type(_leaf(sv)).__name__, sv, j) for j in range(sv.nfeatures())]
    return cols


@pytest.mark.parametrize("variant", ["as_is", "no_lpi"])
@pytest.mark.parametrize("i", range(len(SLICES)), ids=lambda i: f"{i:02d}:{_describe(SLICES[i])}")
def test_supported_slice_runs(fr, i, variant):
    """Slice i of ``_supported()``, as it is or without LPI (section B of the module docstring).

    Measured on the MI355X for the one exception to "two tails, the same bits": the fused slices
    with ``Indices(total=True)`` (13, 14, 21, 29, 30; family ``fused``, G = 5 at T = 300) gave, for
    the SAME input three times, 3 to 15 of 1260 / 1620 entries that differ, all of them MPI, CUR,
    AVG or STD columns, at most 4.4e-16 relative (4.5e-13 absolute on a CUR of 2050); two different
    tails differ in as many entries by as much.  The other slices run ``fused_packed`` at this T
    (one wave per series) and repeat bit for bit."""
    from fruits_amd import _native as nat
    from fruits_amd.lengths import resolve_cuts
    t0 = time.perf_counter()
    src = SLICES[i]
    real = is_real_valued(src)
    N, D, T = B_SHAPE
    fruit = fr.Fruit(variant)
    fruit.add(*(p.copy() for p in src._preparateurs), *(s.copy() for s in src._iss),
              *sieves_of(src, real, lpi=variant == "as_is"))
    slc = fruit.get_slice()
    if not real:        # (no column of an exact slice is left out)
        assert slc.nfeatures() == src.nfeatures() - (0 if variant == "as_is" else src.niteratedsums())
    lengths = np.asarray(B_CLASSES)[np.random.default_rng(i).permutation(N)]
    X = (real_input if real else int_input)(100 + i, B_SHAPE)
    np.random.seed(3)
    fruit.fit(with_tails(X, lengths, 1), lengths=lengths)
    got = fruit.transform(with_tails(X, lengths, 1), lengths=lengths)
    # fused exactly where the dense batch fuses: with LPI never, without it always
    ragged, dense = slc._fused(T, ragged=True), slc._fused(T)
    assert (ragged is not None) == (dense is not None) == (variant == "no_lpi"), (ragged, dense)
    if ragged is not None:
        assert ragged.last_launch()["family"].startswith("fused") and ragged.jit_loaded() == 0
    columns = column_map(slc)
    # Other tails, the same bits - except where the same INPUT does not give the same bits twice:
    # the workgroup-per-unit fused kernels add the wave partials of a band sum (MPI; CUR / AVG /
    # STD) in LDS in arrival order (test_walk_batch.py, test_large_plan_in_pieces), which only
    # integers do not notice.  Such a column of a real-valued slice is held to the bar between
    # the tails too, and to tails of +-1e160 (section C): what a sum takes from them is not lost
    # in its last bits.  Wave-per-series launches and the materialising sieves add in one order.
    in_order = ragged is None or ragged.last_launch()["family"] == "fused_packed"
    summed = np.array([real and not in_order and kind in SUMMED for kind, _, _ in columns])
    again = fruit.transform(with_tails(X, lengths, 2), lengths=lengths)
    np.testing.assert_array_equal(got[:, ~summed], again[:, ~summed])
    np.testing.assert_allclose(again[:, summed], got[:, summed], rtol=1e-6, atol=1e-9)
    if real:
        over = nat.to_host(slc.transform_device(overflow_tails(X, lengths), lengths=lengths))
        assert np.isfinite(over).all(), [fruit.label(c) for c in np.flatnonzero(~np.isfinite(over).all(axis=0))]
        np.testing.assert_array_equal(over[:, ~summed], got[:, ~summed])
        np.testing.assert_allclose(over[:, summed], got[:, summed], rtol=1e-6, atol=1e-9)
    want = per_series(fruit, X, lengths)             # (N = 12: one call per length class)
    assert got.shape == want.shape == (N, fruit.nfeatures())
    for c, (kind, sv, j) in enumerate(columns):
        lb = f"{fruit.label(c)} lengths={lengths.tolist()}"
        if not real:
            np.testing.assert_array_equal(got[:, c], want[:, c], err_msg=lb)
        elif kind in ("NPI", "LPI"):
            # every element of the segment is inside (-inf, inf]: its length
            rows = resolve_cuts(_leaf(sv)._cut, lengths)
            np.testing.assert_array_equal(got[:, c], (rows[:, j + 1] - rows[:, j]).astype(float), err_msg=lb)
            np.testing.assert_array_equal(got[:, c], want[:, c], err_msg=lb)
        else:
            np.testing.assert_allclose(got[:, c], want[:, c], rtol=1e-6, atol=1e-9, err_msg=lb)
    print(f"lengths_batch supported {i:02d} {variant} {'real' if real else 'exact'} {_describe(src)}: "
          f"F={fruit.nfeatures()} seconds={time.perf_counter() - t0:.2f}")


# ------------------------------------------------------------------------------ C: overflowing tails
def overflow_tails(X, lengths):
    """X with +1e160, -1e160, ... behind every series' length."""
    Y = X.copy()
    T = X.shape[2]
    sign = np.where(np.arange(T) % 2 == 0, 1e160, -1e160)
    for n, L in enumerate(lengths):
        Y[n, :, L:] = sign[L:]
    return Y


def _semiring_fruit(fr, semiring):
    words = [fr.words.SimpleWord(s) for s in ("[1]", "[2]", "[1][2]", "[11][2]")]
    fruit = fr.Fruit(semiring)
    fruit.add(fr.ISS(words, mode=fr.ISSMode.EXTENDED, semiring=getattr(fr.semiring, semiring)()))
    fruit.add(*launch_sieves(fr))
    return fruit


OVERFLOW = list(LAUNCH_SHAPES) + ["Arctic", "Bayesian", "lpi"]


@pytest.mark.parametrize("case", OVERFLOW)
def test_tails_that_overflow(fr, monkeypatch, case):
    import torch
    t0 = time.perf_counter()
    if case in LAUNCH_SHAPES:
        shape, weight, classes, debug = LAUNCH_SHAPES[case]
        if debug:
            monkeypatch.setenv("FRUITS_HIP_DEBUG", debug)
        fruit = launch_fruit(fr, weight, shape[1])
    elif case == "lpi":
        shape, classes = (12, 2, 700), [1, 2, 3, 5, 64, 255, 256, 257, 512, 513, 699, 700]
        fruit = launch_fruit(fr, 2, 2, extra=[fr.sieving.LPI()])
    else:
        shape, classes = (12, 2, 200), [1, 2, 3, 5, 64, 65, 128, 129, 199, 200]
        fruit = _semiring_fruit(fr, case)
    X = int_input(sum(shape), shape)
    lengths = spread(classes, shape[0])
    np.random.seed(3)
    fruit.fit(with_tails(X, lengths, 1), lengths=lengths)
    slc = fruit.get_slice()
    assert (slc._fused(shape[2], ragged=True) is None) == (case == "lpi")
    plain = slc.transform_device(with_tails(X, lengths, 1), lengths=lengths)
    huge = overflow_tails(X, lengths)
    with np.errstate(over="ignore"):
        assert np.isfinite(huge).all() and not np.isfinite(huge[lengths < shape[2]] ** 2).all()
    over = slc.transform_device(huge, lengths=lengths)
    # (before the nan_to_num of Fruit.transform: nothing there for it to replace)
    assert torch.isfinite(plain).all(), torch.nonzero(~torch.isfinite(plain))[:5]
    assert torch.isfinite(over).all(), torch.nonzero(~torch.isfinite(over))[:5]
    assert first_difference(over.cpu().numpy(), plain.cpu().numpy(), f"overflow {case}", shape[0])
    assert torch.equal(over.view(torch.int64), plain.view(torch.int64))
    print(f"lengths_batch overflow {case}: seconds={time.perf_counter() - t0:.2f}")


# ------------------------------------------------------------------------------ D: the surface
def test_fruit_of_two_slices(fr):
    """One fusing slice and one with LPI: fit_transform is fit then transform, every row the
    per-series call's."""
    shape = (12, 2, 300)
    X = int_input(51, shape)
    lengths = np.asarray(B_CLASSES)[np.random.default_rng(51).permutation(12)]

    def make():
        fruit = launch_fruit(fr, 2, 2)
        fruit.cut()
        fruit.add(fr.ISS(fr.words.of_weight(1, dim=2)), fr.sieving.NPI, fr.sieving.LPI, fr.sieving.END)
        return fruit
    one, two = make(), make()
    np.random.seed(7)
    both = one.fit_transform(with_tails(X, lengths, 1), lengths=lengths)
    np.random.seed(7)
    two.fit(with_tails(X, lengths, 1), lengths=lengths)
    np.testing.assert_array_equal(both, two.transform(with_tails(X, lengths, 2), lengths=lengths))
    assert one.get_slice(0)._fused(300, ragged=True) is not None
    assert one.get_slice(1)._fused(300, ragged=True) is None
    assert both.shape == (12, one.nfeatures())
    np.testing.assert_array_equal(both, per_series(one, X, lengths))


def test_one_series(fr):
    X = int_input(52, (1, 2, 300))
    lengths = np.array([129])
    fruit = launch_fruit(fr, 2, 2)
    np.random.seed(7)
    fruit.fit(X)
    got = fruit.transform(with_tails(X, lengths, 1), lengths=lengths)
    np.testing.assert_array_equal(got, fruit.transform(np.ascontiguousarray(X[:, :, :129])))
    assert not np.array_equal(got, fruit.transform(with_tails(X, lengths, 1)))


def test_lengths_of_any_integer_type(fr):
    shape = (12, 2, 200)
    lengths = spread([1, 2, 3, 5, 64, 65, 128, 129, 199, 200], 12)
    X = with_tails(int_input(53, shape), lengths, 1)
    fruit = launch_fruit(fr, 2, 2)
    np.random.seed(7)
    fruit.fit(X, lengths=lengths)
    want = fruit.transform(X, lengths=lengths)
    assert not np.array_equal(want, fruit.transform(X))
    for other in (lengths.astype(np.int32), lengths.astype(np.uint8), [int(v) for v in lengths]):
        np.testing.assert_array_equal(fruit.transform(X, lengths=other), want)


def test_transform_device_returns_the_device_tensor(fr):
    import torch
    shape = (12, 2, 300)
    lengths = np.asarray(B_CLASSES)
    X = with_tails(int_input(54, shape), lengths, 1)
    fruit = launch_fruit(fr, 2, 2)
    np.random.seed(7)
    fruit.fit(X, lengths=lengths)
    slc = fruit.get_slice()
    dev = slc.transform_device(X, lengths=lengths)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.shape == (12, slc.nfeatures())
    np.testing.assert_array_equal(dev.cpu().numpy(), slc.transform(X, lengths=lengths))
    np.testing.assert_array_equal(np.nan_to_num(dev.cpu().numpy()), fruit.transform(X, lengths=lengths))
