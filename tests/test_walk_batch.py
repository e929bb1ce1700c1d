"""Every series of every launch shape of the trie walk.

A unit (series n, group g) is decoded from a workgroup or unit index in five places (the static
programs' loop and their mixed launch's tail, the interpreter's strided grid and its prefetch, the
lean and the fused walk, the wave-per-series kernels), with a plain and an XCD-aware numbering.
Which of them runs is the host's choice (csrc/launch_choice.h); every case here names the branch
it is about, asserts through ``Plan.last_launch()`` that this branch ran, and checks ALL N series:

(a) no NaN of the prefill is left;
(b) ``last_launch()`` is the branch the case names;
(c) the tensor is bit-identical to the same plan run over the same input in slabs of 64
    consecutive series (5 below 128 series; the last slab ragged): a slab is a small batch - all
    groups, one round, trivial numbering - so the big launch has to reproduce it per series
    whatever its grid does (groups agree, static = interpreter = lean);
(d) the slabs agree with the oracle over the whole batch, by the bar of test_hip_parity.py for the
    semiring and weighting; the Reals rows of 96 of the series (one slab whole) also by the derived
    elementwise bound of iss_bounds.py.

The series are independent draws: a row computed from another series' input is off by O(1).
Shapes that are defined against one resident round R of workgroups take R from the record of a
probe launch of the same plan (8 series), not from the literal 1536 of an MI355X.

Where a branch is not what the plain shape gives, the case reaches it the way the host's rules
allow and keeps the assertion: of_weight(2,3) has ahead-of-time static programs for every even
T <= 1024, so its interpreter and lean cases at T = 1000 run under FRUITS_HIP_STATIC=0 (the slabs
under the default environment: static program against interpreter); the lean walk "by the plan's
size" has two groups for R / 2 <= N < R, the caller's nine groups stay on the interpreter while
9 N < 2 R, and a weighted plan stages more rows and has a smaller R (768), so those N follow R.

Fused launches (``Fruit.transform``) are compared with slabs of 64 through the same fitted fruit:
counts, END, MAX and MIN exactly, MPI and CUR to rtol 1e-10 / atol 1e-12 (wave partials are added
in arrival order - the tolerance of test_experiment_fruits_full_size for batch independence)."""
import time

import numpy as np
import pytest

import iss_bounds as ib
from conftest import gen_input
from test_hip_parity import build_fruit, rowwise_close, sieve_kinds

pytestmark = pytest.mark.gpu

CACHE = 256.0 * 1024 * 1024      # csrc/launch_choice.h, kInfinityCacheBytes


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    yield fruits_amd
    ib.print_ratios()


def _words(fr, which):
    return fr.words.of_weight(2, dim=3) if which == "P23" else fr.words.of_weight(4, dim=2)


def _make_iss(fr, which, semiring="Reals", weighting=None):
    wt = None
    if weighting is not None:
        kw = {k: v for k, v in weighting.items() if k != "kind"}
        wt = getattr(fr.iss.weighting, weighting["kind"])(**kw)
    return fr.ISS(_words(fr, which), mode=fr.ISSMode.EXTENDED,
                  semiring=getattr(fr.semiring, semiring)(), weighting=wt)


def _input(seed, N, D, T, walk=False):
    X = gen_input({"seed": seed, "dist": "normal", "shape": [N, D, T]})
    # (L1 weighting: a cumulated walk, so that the path lengths differ from series to series)
    return np.ascontiguousarray(X.cumsum(axis=2) / 8.0) if walk else X


def _probe(fr, iss, D, T, n=8):
    """The record of a launch of `n` series of zeros: what the device reports as a resident round
    (``resident``; ``mixed_resident`` where the launch falls into the cache-sized window of a
    static program, from 768 series on)."""
    import torch
    from fruits_amd import _native as nat
    dev = nat.require_device()
    plan = iss._plan(0, len(iss.words))
    Xd = torch.zeros((n, D, T), dtype=torch.float64, device=dev)
    lk = None if iss.weighting is None else torch.zeros((1, T), dtype=torch.float64, device=dev)
    plan.run(Xd, lk)
    torch.cuda.synchronize()
    return plan.last_launch()


def _first_difference(big, slab):
    """(first differing (k, n, t), number of series that differ) of two (K, N, T) device tensors."""
    import torch
    ne = big.view(torch.int64) != slab.view(torch.int64)
    series = ne.any(dim=2).any(dim=0)
    flat = int(torch.nonzero(ne.reshape(-1))[0])
    K, N, T = big.shape
    return (flat // (N * T), flat // T % N, flat % T), int(series.sum())


def _check_oracle(iss, words, X, got, weighting, semiring, lookup_dev=None, name=""):
    """(d): `got` (K, N, T) against the oracle over the whole batch; returns the deviation.
    Reals rows are held to the derived elementwise bound too (iss_bounds: the long-double oracle
    with the device's own lookup) - on 96 series: every series of the first slab of 64 and 32
    spread over the other slabs, the last series among them; a batch of at most 96 series whole.
    The series outside these are held to the row-wise bar above alone ((c) compares a series
    with the same series of the big launch, not with another one)."""
    from oracle import c_oracle as corc
    from oracle import ref_numpy as orc
    lookup, total = orc._weight_lookup(weighting, X, X)
    ref = corc.iss_transform(X, [str(w) for w in words], "EXTENDED", None, lookup, total,
                             semiring=semiring)
    if semiring == "Arctic" or (semiring == "Bayesian" and weighting is None):
        np.testing.assert_array_equal(got, ref)    # max is exact, the letters multiply in order
        return 0.0
    dev = rowwise_close(got, ref)
    if semiring == "Reals":
        ib.check_reals(got, X, [str(w) for w in words], "EXTENDED", None, lookup_dev, total,
                       what=f"walk_batch {name}", family="walk_batch", whole=64)
    return dev


def _materialising(fr, monkeypatch, name, which, T, n_of, want, *, env=None, groups=0,
                   semiring="Reals", weighting=None, walk=False, seed=0, probe_n=8):
    """One case of the table: `n_of(record of the probe)` series, `want(N, probe)` the branch."""
    import torch
    from fruits_amd import _native as nat
    t0 = time.perf_counter()
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    iss = _make_iss(fr, which, semiring, weighting)
    words = iss.words
    D = 3 if which == "P23" else 2
    probe = _probe(fr, iss, D, T, probe_n)
    N = int(n_of(probe))
    X = _input(seed + N, N, D, T, walk)
    iss._attach_cache(X)
    Xd = nat.to_device(X)
    lk = iss.lookup_device(Xd)
    plan = iss._plan(0, len(words))
    K = plan.rows
    big = torch.full((K, N, T), float("nan"), dtype=torch.float64, device=Xd.device)
    plan.run(Xd, lk, out=big, groups=groups)
    torch.cuda.synchronize()
    ran = plan.last_launch()
    # the slabs: small batches under the default environment and the host's own group count
    for k in (env or {}):
        monkeypatch.delenv(k)
    step = 64 if N >= 128 else 5
    slab = torch.full((K, N, T), float("nan"), dtype=torch.float64, device=Xd.device)
    for a in range(0, N, step):
        b = min(a + step, N)
        plan.run(Xd[a:b], lk if lk is None or lk.shape[0] == 1 else lk[a:b], out=slab[:, a:b],
                 strides=(N * T, T))
    torch.cuda.synchronize()
    # (a) every row was written
    assert not torch.isnan(big).any(), name
    assert not torch.isnan(slab).any(), name
    # (b) the branch
    expect = want(N, probe)
    assert {k: ran[k] for k in expect} == expect, (name, N, ran)
    # (c) the big launch reproduces the small batches, series by series
    same = torch.equal(big.view(torch.int64), slab.view(torch.int64))
    if not same:
        where, n_series = _first_difference(big, slab)
        print(f"walk_batch {name}: N={N} first difference at (k, n, t) = {where}, "
              f"{n_series} of {N} series differ")
    assert same, (name, N)
    # (d) and those are right
    got = nat.to_host(slab)
    del big, slab
    dev = _check_oracle(iss, words, X, got, weighting, semiring,
                        lookup_dev=None if lk is None else nat.to_host(lk), name=name)
    print(f"walk_batch {name}: N={N} T={T} ran={ran} oracle_dev={dev:.3e} "
          f"seconds={time.perf_counter() - t0:.2f}")


def _first_beyond_static_window(T, dims, K):
    """The first N whose input + output exceed 1.4 x the Infinity Cache (launch_choice.h)."""
    N = int(1.4 * CACHE // (8 * T * (dims + K)))
    while 8.0 * N * T * (dims + K) <= 1.4 * CACHE:
        N += 1
    return N


def _xcd(N):
    return 1 if N % 8 == 0 else 0


NO_STATIC = {"FRUITS_HIP_STATIC": "0"}    # (of_weight(2,3) has ahead-of-time programs for T <= 1024)
BEYOND = _first_beyond_static_window(1024, 3, 18)

MATERIALISING = {
    # 1: static program, all groups, one workgroup per unit
    "static_small_xcd": dict(which="P23", T=1024, n_of=lambda p: 40, want=lambda N, p: dict(
        family="static_aot", G=3, persistent=0, xcd_map=1, wt=0, lds_pad=0, tail_series=0, n_whole=N)),
    "static_small_plain": dict(which="P23", T=1024, n_of=lambda p: 37, want=lambda N, p: dict(
        family="static_aot", G=3, persistent=0, xcd_map=0, wt=0, lds_pad=0, tail_series=0, n_whole=N)),
    # 2: the mixed launch: one resident round of whole series, the tail program's finer units behind
    "static_mixed_tail16": dict(which="P23", T=1024, probe_n=768,
                                n_of=lambda p: p["mixed_resident"] + 16, want=lambda N, p: dict(
        family="static_aot", G=1, persistent=0, wt=1, lds_pad=0, tail_series=16,
        n_whole=p["mixed_resident"], mixed_resident=p["mixed_resident"])),
    "static_mixed_tail13": dict(which="P23", T=1024, probe_n=768,
                                n_of=lambda p: p["mixed_resident"] + 13, want=lambda N, p: dict(
        family="static_aot", G=1, persistent=0, wt=1, lds_pad=0, tail_series=13,
        n_whole=p["mixed_resident"], mixed_resident=p["mixed_resident"])),
    # 3: beyond 1.4 x the cache: three groups, LDS pad, write-through instance
    "static_stream_plain": dict(which="P23", T=1024, n_of=lambda p: BEYOND, want=lambda N, p: dict(
        family="static_aot", G=3, persistent=0, xcd_map=0, wt=1, lds_pad=1, tail_series=0, n_whole=N)),
    "static_stream_xcd": dict(which="P23", T=1024, n_of=lambda p: (BEYOND + 7) // 8 * 8,
                              want=lambda N, p: dict(
        family="static_aot", G=3, persistent=0, xcd_map=1, wt=1, lds_pad=1, tail_series=0, n_whole=N)),
    # 4: interpreter, two groups, the strided grid with a partial second round
    "interp_g2_plain": dict(which="P23", T=1000, env=NO_STATIC, n_of=lambda p: 1001, strided=True,
                            want=lambda N, p: dict(family="interpreter", G=2, persistent=1, xcd_map=0)),
    "interp_g2_xcd": dict(which="P23", T=1000, env=NO_STATIC, n_of=lambda p: 1000, strided=True,
                          want=lambda N, p: dict(family="interpreter", G=2, persistent=1, xcd_map=1)),
    # 5: interpreter, whole series, non-temporal input (1 to 1.5 x the cache)
    "interp_g1_nt": dict(which="P23", T=1000, env=NO_STATIC, n_of=lambda p: 1700, strided=True,
                         want=lambda N, p: dict(family="interpreter", G=1, persistent=1, nt_input=1)),
    # 6: lean walk because the units fill two rounds
    "lean_two_rounds_plain": dict(which="P23", T=1000, env=NO_STATIC,
                                  n_of=lambda p: 2 * p["resident"] + 1, want=lambda N, p: dict(
        family="lean", G=3, persistent=0, xcd_map=0, resident=p["resident"])),
    "lean_two_rounds_xcd": dict(which="P23", T=1000, env=NO_STATIC,
                                n_of=lambda p: (2 * p["resident"] + 7) // 8 * 8, want=lambda N, p: dict(
        family="lean", G=3, persistent=0, xcd_map=1, resident=p["resident"])),
    # 7: lean walk because of the plan's size (115 nodes), two groups: R / 2 <= N < R
    "lean_long_plan_plain": dict(which="P42", T=600, n_of=lambda p: (p["resident"] // 2 + 5) | 1,
                                 want=lambda N, p: dict(
        family="lean", G=2, persistent=0, xcd_map=0, resident=p["resident"])),
    "lean_long_plan_xcd": dict(which="P42", T=600, n_of=lambda p: (p["resident"] // 2 + 12) // 8 * 8,
                               want=lambda N, p: dict(
        family="lean", G=2, persistent=0, xcd_map=1, resident=p["resident"])),
    # 8: interpreter, two time chunks, the carries in LDS
    "interp_two_chunks": dict(which="P23", T=1100, n_of=lambda p: p["resident"] + 64, strided=True,
                              want=lambda N, p: dict(
        family="interpreter", G=1, persistent=1, carry_in_lds=1, resident=p["resident"])),
    # 9: wave per series, four series per workgroup, N % 4 == 3
    "packed_persistent": dict(which="P23", T=200, n_of=lambda p: 8195, want=lambda N, p: dict(
        family="packed", persistent=1)),
    "packed_per_unit": dict(which="P23", T=100, n_of=lambda p: 1027, want=lambda N, p: dict(
        family="packed", persistent=0)),
    # 10: the caller's group count (all nine units), the strided grid in its second round
    "interp_g9_plain": dict(which="P23", T=1000, groups=9, strided=True, n_of=lambda p: p["resident"] // 9 + 31,
                            want=lambda N, p: dict(family="interpreter", G=9, persistent=1, xcd_map=_xcd(N))),
    "interp_g9_xcd": dict(which="P23", T=1000, groups=9, strided=True, n_of=lambda p: (p["resident"] // 9 + 38) // 8 * 8,
                          want=lambda N, p: dict(family="interpreter", G=9, persistent=1, xcd_map=1)),
    # 11: L1 weighting: exp tables of N lookup rows
    # (five staged rows: fewer resident workgroups than the unweighted plan, so N follows R)
    "interp_l1": dict(which="P23", T=1000, n_of=lambda p: p["resident"] + 164, walk=True, strided=True,
                      weighting={"kind": "L1"},
                      want=lambda N, p: dict(family="interpreter", G=1, persistent=1)),
    "interp_l1_total": dict(which="P23", T=1000, n_of=lambda p: p["resident"] + 164, walk=True, strided=True,
                            weighting={"kind": "L1", "total": True},
                            want=lambda N, p: dict(family="interpreter", G=1, persistent=1)),
    # 12: the lean walk once per semiring / weighting
    "lean_indices": dict(which="P23", T=1000, n_of=lambda p: 2 * p["resident"] + 1,
                         weighting={"kind": "Indices"},
                         want=lambda N, p: dict(family="lean", G=3, persistent=0, xcd_map=0)),
    "lean_arctic": dict(which="P23", T=1000, n_of=lambda p: 2 * p["resident"] + 1, semiring="Arctic",
                        want=lambda N, p: dict(family="lean", G=3, persistent=0, xcd_map=0)),
    "lean_bayesian": dict(which="P23", T=1000, n_of=lambda p: 2 * p["resident"] + 1, semiring="Bayesian",
                          want=lambda N, p: dict(family="lean", G=3, persistent=0, xcd_map=0)),
}


@pytest.mark.parametrize("name", list(MATERIALISING))
def test_materialising(fr, monkeypatch, name):
    case = dict(MATERIALISING[name])
    want = case.pop("want")
    if case.pop("strided", False):
        # the case is about the strided grid in a partial SECOND round: more units than one
        # resident round, fewer than two
        def want(N, p, inner=want):
            out = inner(N, p)
            assert p["resident"] < N * out["G"] < 2 * p["resident"], (name, N, p)
            return out
    _materialising(fr, monkeypatch, name, want=want, seed=len(name), **case)


def test_coswiss(fr):
    """CosWISS - the word set and exponents of test_coswiss_long_series - at N = 1700: its launch is
    not choose_walk_launch's (no branch to assert), slabs and oracle as above."""
    import torch
    from fruits_amd import _native as nat
    from oracle import ref_numpy as orc
    t0 = time.perf_counter()
    N, T = 1700, 1000
    X = gen_input({"seed": 13, "dist": "normal", "shape": [N, 2, T]}) / np.sqrt(T)
    X[:, 1] = np.abs(X[:, 1]) + 0.5
    words = ["[1]", "[2][1]", "[1][2][2]", "[12][1][-2][1]"]
    freqs = [0.15, 0.5]
    Xd = nat.to_device(X)
    for exponent in (1, 2):
        cw = fr.CosWISS([fr.words.SimpleWord(s) for s in words], freqs, exponent=exponent,
                        total_weighting=False)
        shape = (len(words) * len(freqs), N, T)
        big = cw.transform_device(Xd, out=torch.full(shape, float("nan"), dtype=torch.float64,
                                                     device=Xd.device))
        slab = torch.full(shape, float("nan"), dtype=torch.float64, device=Xd.device)
        for a in range(0, N, 64):
            slab[:, a:a + 64] = cw.transform_device(Xd[a:a + 64])
        torch.cuda.synchronize()
        assert not torch.isnan(big).any() and not torch.isnan(slab).any()
        same = torch.equal(big.view(torch.int64), slab.view(torch.int64))
        if not same:
            print("walk_batch coswiss: first difference, series that differ:", _first_difference(big, slab))
        assert same, exponent
        out = nat.to_host(slab)
        ref = orc.coswiss_transform(X, words, freqs, exponent, False)
        scale = np.abs(ref).max(axis=2, keepdims=True)
        bound = 1e-6 * np.maximum(np.abs(ref), 1e-3 * scale)    # (test_coswiss_long_series' bar)
        assert np.all(np.abs(out - ref) <= bound), exponent
        # (the first slab of 64 whole and 32 series spread over the others: iss_bounds.series_subset)
        ib.check_coswiss(out, X, words, freqs, exponent, False, what=f"walk_batch coswiss exponent={exponent}",
                         family="walk_batch_coswiss", whole=64)
        print(f"walk_batch coswiss exponent={exponent}: oracle_dev="
              f"{np.max(np.abs(out - ref) / np.maximum(np.abs(ref), 1e-3 * scale)):.3e}")
    print(f"walk_batch coswiss: seconds={time.perf_counter() - t0:.2f}")


# ---------------------------------------------------------------------------------- fused
def _fused(fr, monkeypatch, name, which, T, sieves, n_of, want, env=None):
    import torch
    t0 = time.perf_counter()
    monkeypatch.setenv("FRUITS_AMD_AUTO_PREPARE", "0")     # the built-in kernels, whatever a cache holds
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    D = 3 if which == "P23" else 2
    spec = {"name": name, "slices": [{"iss": [{"words": [str(w) for w in _words(fr, which)],
                                               "mode": "EXTENDED"}],
                                      "sieves": sieves, "fit_sample_size": 1.0}]}
    fruit = build_fruit(fr, spec)
    np.random.seed(5)
    fruit.fit(_input(1, 24, D, T))
    pipe = next(iter(fruit))._fused(T)
    assert pipe is not None
    fruit.transform(_input(2, 8, D, T))                    # the probe: one resident round
    probe = pipe.last_launch()
    N = int(n_of(probe))
    X = _input(len(name) + N, N, D, T)
    feats = fruit.transform(X)
    torch.cuda.synchronize()
    ran = pipe.last_launch()
    expect = want(N, probe)
    assert {k: ran[k] for k in expect} == expect, (name, N, ran)
    assert feats.shape == (N, fruit.nfeatures()) and np.isfinite(feats).all()
    slabs = np.concatenate([fruit.transform(np.ascontiguousarray(X[a:a + 64])) for a in range(0, N, 64)])
    kinds = sieve_kinds([fruit.label(i) for i in range(fruit.nfeatures())])
    summed = np.isin(kinds, ("MPI", "CUR"))
    assert set(kinds[~summed]) <= {"NPI", "LPI", "XPI", "END", "MAX", "MIN"}
    exact = feats[:, ~summed] == slabs[:, ~summed]
    if not exact.all():
        n, f = np.argwhere(~exact)[0]
        print(f"walk_batch {name}: N={N} first difference at series {n}, column {f}; "
              f"{int((~exact).any(axis=1).sum())} of {N} series differ")
    assert exact.all(), (name, N)
    np.testing.assert_allclose(feats[:, summed], slabs[:, summed], rtol=1e-10, atol=1e-12)
    print(f"walk_batch {name}: N={N} T={T} ran={ran} seconds={time.perf_counter() - t0:.2f}")


SIEVES_14 = [{"kind": "NPI"}, {"kind": "MPI"}, {"kind": "END"}, {"kind": "MAX"}, {"kind": "CUR"}]
SIEVES_15 = [{"kind": "NPI"}, {"kind": "MPI"}, {"kind": "END"}]
TWO_GROUPS = {"FRUITS_HIP_DEBUG": "groups=2"}

FUSED = {
    # 14: one workgroup per series, the whole (N, F) block
    "fused_plain": dict(which="P23", T=1000, sieves=SIEVES_14, n_of=lambda p: 2 * p["resident"] + 1,
                        want=lambda N, p: dict(family="fused", G=1, persistent=0, resident=p["resident"])),
    "fused_even": dict(which="P23", T=1000, sieves=SIEVES_14, n_of=lambda p: 2 * p["resident"],
                       want=lambda N, p: dict(family="fused", G=1, persistent=0, resident=p["resident"])),
    # 15: two groups per series
    "fused_g2_plain": dict(which="P42", T=600, sieves=SIEVES_15, env=TWO_GROUPS, n_of=lambda p: 261,
                           want=lambda N, p: dict(family="fused", G=2, persistent=0, xcd_map=0)),
    "fused_g2_xcd": dict(which="P42", T=600, sieves=SIEVES_15, env=TWO_GROUPS, n_of=lambda p: 264,
                         want=lambda N, p: dict(family="fused", G=2, persistent=0, xcd_map=1)),
    # 16: wave per series
    "fused_packed": dict(which="P23", T=200, sieves=SIEVES_14, n_of=lambda p: 8195,
                         want=lambda N, p: dict(family="fused_packed", persistent=0)),
}


@pytest.mark.parametrize("name", list(FUSED))
def test_fused(fr, monkeypatch, name):
    _fused(fr, monkeypatch, name, **FUSED[name])
