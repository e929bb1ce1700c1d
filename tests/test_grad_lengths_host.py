"""Per-series lengths in the backward pass without a GPU: the setter
fr_plan_set_grad_lengths and the refusals it adds to the four backward entries, the per-series
cut table of fr_sieve_pick, the errors of ``check_lengths`` through every new Python entry, and
the cut table ``_Head`` builds.  Every ABI call below fails on the host: its pointers are never
dereferenced."""
import ctypes as C

import numpy as np
import pytest

import ragged_grad_ref as rr


def tab(*rows):
    return np.array(rows, dtype=np.int32)


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# ---------------------------------------------------------------- the ABI
def test_setter_is_exported_and_versioned():
    from fruits_amd import _native as nat
    L = nat.lib()
    assert "fr_plan_set_grad_lengths" in nat.EXPORTS and callable(L.fr_plan_set_grad_lengths)
    assert L.fr_version() >= 142


def test_no_new_entry_takes_a_stream():
    """The lengths are state of the plan, delivered without a stream (as fr_pipeline_set_lengths)."""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(os.path.dirname(here), "include", "fruits_hip.h")).read()
    decl = re.search(r"int fr_plan_set_grad_lengths\(([^;]*)\);", header)
    assert decl and "stream" not in decl.group(1)
    assert decl.group(1).count(",") == 2


def test_setter_and_mismatch_are_refused_before_any_device_call():
    from fruits_amd import _native as nat
    L = nat.lib()
    i64, i32 = C.c_int64, C.c_int32
    p, q, r, s = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))      # never dereferenced
    null = C.c_void_p(0)
    rows = np.array([1], dtype=np.int32)
    one = [np.ones(1, np.float32)]
    plans = {
        "fr_iss_backward": nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1]),
        "fr_iss_backward_max": nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1], arctic=True),
        "fr_iss_backward_weighted": nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1],
                                             [np.ones(1, np.float32), np.ones(2, np.float32)], nat.FR_W_TOTAL),
    }
    assert one
    # the setter's own refusals
    assert L.fr_plan_set_grad_lengths(None, p, i64(3)) == nat.FR_E_ARG
    assert "fr_plan_set_grad_lengths: null plan" in nat.last_error()
    assert L.fr_plan_set_grad_lengths(plans["fr_iss_backward"]._h, p, i64(-1)) == nat.FR_E_ARG
    assert "fr_plan_set_grad_lengths: bad shape" in nat.last_error()

    def dense(name, N):
        plan = plans[name]
        if name == "fr_iss_backward_weighted":
            return L.fr_iss_backward_weighted(plan._h, p, i64(N), i64(2), i64(5), q, i64(1), q, i64(1), i64(5),
                                              i64(5), i64(1), i32p(rows), r, s, C.c_void_p(4096 * 5),
                                              C.c_void_p(4096 * 6), null)
        return getattr(L, name)(plan._h, p, i64(N), i64(2), i64(5), q, q, i64(1), i64(5), i64(5), i64(1),
                                i32p(rows), r, s, null)

    def picked(name, N):
        plan = plans[name]
        weighted = name == "fr_iss_backward_weighted"
        return L.fr_iss_backward_picked(plan._h, p, i64(N), i64(2), i64(5), null if weighted else q,
                                        q if weighted else null, i64(1 if weighted else 0), q, q, i64(1),
                                        i32(2), i32p(rows), r if weighted else null, s,
                                        C.c_void_p(4096 * 5) if weighted else null, C.c_void_p(4096 * 6), null)

    for name, plan in plans.items():
        assert L.fr_plan_set_grad_lengths(plan._h, p, i64(3)) == 0
        for who, call in ((name, dense), ("fr_iss_backward_picked", picked)):
            assert call(name, 2) == nat.FR_E_ARG, who
            text = nat.last_error()
            assert text.startswith(who + ":") and "set for 3 series" in text and "brings 2" in text, text
            # the entry's own checks still come first
            assert call(name, -1) == nat.FR_E_ARG and "bad shape" in nat.last_error()
        # cleared (a null table, whatever N): armed for nothing - a call of no series is served
        assert L.fr_plan_set_grad_lengths(plan._h, None, i64(7)) == 0
        assert dense(name, 0) == 0 and picked(name, 0) == 0
        # armed for no series: only a call of no series matches
        assert L.fr_plan_set_grad_lengths(plan._h, p, i64(0)) == 0
        assert dense(name, 0) == 0
        assert dense(name, 2) == nat.FR_E_ARG and "set for 0 series" in nat.last_error()
        assert L.fr_plan_set_grad_lengths(plan._h, None, i64(0)) == 0


def test_sieve_pick_per_series_cuts_are_checked_before_any_device_call():
    from fruits_amd import _native as nat
    L = nat.lib()
    i64, i32 = C.c_int64, C.c_int32
    p = C.c_void_p(4096)        # never dereferenced
    null = C.c_void_p(0)
    S = nat.FR_SIEVE_SERIES_CUTS
    END, MAX, MIN = nat.FR_SIEVE_END | S, nat.FR_SIEVE_MAX | S, nat.FR_SIEVE_MIN | S
    good = [[END, 0, 2, 0, 0, 0], [MAX, 2, 3, 0, 3, 1], [MIN, 2, 3, 3, 2, 5]]

    def call(spec=good, K=2, N=3, T=9, cuts=p, n_cuts=15, F=7):
        sp = np.ascontiguousarray(spec, dtype=np.int32)
        return L.fr_sieve_pick(p, i64(K), i64(N), i64(T), p, i32p(sp), i32(len(spec)), cuts, i64(n_cuts), p,
                               i64(5), i32(F), p, p, null)

    def changed(s, col, value):
        out = [list(r) for r in good]
        out[s][col] = value
        return out

    cases = [
        (lambda: call(changed(1, 0, nat.FR_SIEVE_MAX)), "sieve 1 and sieve 0 differ in FR_SIEVE_SERIES_CUTS"),
        (lambda: call(changed(0, 0, nat.FR_SIEVE_END)), "sieve 1 and sieve 0 differ in FR_SIEVE_SERIES_CUTS"),
        (lambda: call(n_cuts=16), "n_cuts = 16 is no multiple of N = 3"),
        # the table has 5 slots for the sieves in all - but a series' row is 4 long, or the row
        # index lies behind it
        (lambda: call(n_cuts=12), "sieve 1 has a cut row outside a series' row of the cut table"),
        (lambda: call(changed(2, 1, 3)), "sieve 2 has a cut row outside a series' row of the cut table"),
        (lambda: call(changed(0, 1, -1)), "sieve 0 has a cut row outside a series' row of the cut table"),
        (lambda: call(changed(1, 0, nat.FR_SIEVE_NPI | S)), "sieve 1 is no selecting sieve"),
        (lambda: call(F=8), "the sieves have 7 features, not F = 8"),
        (lambda: call(cuts=null), "null device pointer"),
    ]
    for fn, text in cases:
        assert fn() == nat.FR_E_ARG, text
        assert text in nat.last_error(), (text, nat.last_error())
    # nothing to do, after the same checks
    assert call(N=0, n_cuts=5) == 0 and call(K=0) == 0


# ---------------------------------------------------------------- fruits_amd.nn
def entries(fr, nn):
    """Every Python entry that takes lengths, as ``call(X, lengths)``."""
    from fruits_amd.iss.weighting import Indices
    words = [fr.words.SimpleWord("[1][2]")]
    ext, sv = fr.ISSMode.EXTENDED, fr.sieving
    sieves = [sv.END([-1]), sv.MAX([2, -1])]
    arctic, ind = fr.semiring.Arctic(), Indices()
    return {
        "iss": lambda X, L: nn.iss(X, words, ext, lengths=L),
        "max_iss": lambda X, L: nn.max_iss(X, words, ext, semiring=arctic, lengths=L),
        "weighted_iss": lambda X, L: nn.weighted_iss(X, words, ext, weighting=ind, lengths=L),
        "ISSLayer": lambda X, L: nn.ISSLayer(words, ext)(X, lengths=L),
        "MaxISSLayer": lambda X, L: nn.MaxISSLayer(words, ext, semiring=arctic)(X, L),
        "WeightedISSLayer": lambda X, L: nn.WeightedISSLayer(words, ext, weighting=ind)(X, lengths=L),
        "FeatureLayer": lambda X, L: nn.FeatureLayer(words, ext, sieves)(X, lengths=L),
        "iss_features_ragged": lambda X, L: nn.iss_features_ragged(X, L, words, ext, sieves),
    }


def test_input_checks_come_before_the_lengths():
    """On a host tensor every entry names X first, as it does without lengths - whatever the
    lengths are."""
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    X = torch.zeros((2, 2, 5), dtype=torch.float64)
    for name, call in entries(fr, nn).items():
        for lengths in (np.array([5, 4]), np.array([9, 0]), np.array([1.5, 2.0]), torch.tensor([5, 4])):
            with pytest.raises(TypeError, match="GPU"):
                call(X, lengths)
        with pytest.raises(TypeError, match="float64"):
            call(X.float(), np.array([9, 0]))
        with pytest.raises(IndexError, match="references dimension 2"):
            call(X[:, :1], np.array([9, 0]))


def test_lengths_errors_at_the_unit_that_raises_them():
    """``nn._ragged_lengths`` is ``check_lengths`` for arrays and tensors alike; a dense batch -
    no lengths, or all equal to T - is None."""
    import torch
    from fruits_amd import nn
    from fruits_amd.lengths import check_lengths
    for wrap in (np.asarray, torch.tensor):
        with pytest.raises(TypeError, match="array of integers"):
            nn._ragged_lengths(wrap([1.0, 2.0]), 2, 5)
        with pytest.raises(TypeError, match="array of integers"):
            nn._ragged_lengths(wrap([True, False]), 2, 5)
        with pytest.raises(ValueError, match=r"shape \(2,\)"):
            nn._ragged_lengths(wrap([1, 2, 3]), 2, 5)
        with pytest.raises(ValueError, match=r"shape \(2,\)"):
            nn._ragged_lengths(wrap([[1, 2]]), 2, 5)
        with pytest.raises(ValueError, match="1..5"):
            nn._ragged_lengths(wrap([0, 2]), 2, 5)
        with pytest.raises(ValueError, match="1..5"):
            nn._ragged_lengths(wrap([6, 2]), 2, 5)
        got = nn._ragged_lengths(wrap([5, 2]), 2, 5)
        assert got.dtype == np.int64 and got.tolist() == [5, 2]
        np.testing.assert_array_equal(got, check_lengths(np.array([5, 2]), 2, 5))
        assert nn._ragged_lengths(wrap([5, 5]), 2, 5) is None
    assert nn._ragged_lengths(torch.tensor([3, 5], dtype=torch.int32), 2, 5).tolist() == [3, 5]
    assert nn._ragged_lengths(None, 2, 5) is None
    assert nn._ragged_lengths(np.zeros(0, dtype=np.int64), 0, 5) is None


def test_the_two_refusals_stay():
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    words, sv = [fr.words.SimpleWord("[1][2]")], fr.sieving
    X = torch.zeros((2, 2, 5), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="lengths=.*iss_features_ragged"):
        nn.iss_features(X, words, fr.ISSMode.SINGLE, [sv.END()], lengths=np.array([5, 4]))
    with pytest.raises(NotImplementedError, match=r"lengths=.*FeatureLayer\(\.\.\.\)\(X, lengths="):
        nn.FeatureLayer(words, fr.ISSMode.SINGLE, [sv.END()], lengths=np.array([5, 4]))
    assert "iss_features_ragged" in nn.__all__
    # what the dense entry refuses, the ragged one refuses in the same words
    for refused, text in ((sv.NPI(), "NPI counts"), (sv.MAX([0.5]), "float")):
        with pytest.raises(NotImplementedError, match=text):
            nn.iss_features_ragged(X, np.array([5, 4]), words, fr.ISSMode.SINGLE, [refused])


def test_head_cut_table_is_the_sieves_own_resolution():
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    from fruits_amd.lengths import resolve_cuts, resolve_end_cuts
    sv = fr.sieving
    head = nn._Head([sv.END([-1]), sv.END([2]), sv.MAX([2, -1]), sv.MIN([-1])])
    lengths = rr.deal((2, 3, 4, 5, 63, 64, 2051), 2, seed=3)
    spec, cuts, q = head.host_series_tables(lengths)
    want = np.concatenate([resolve_end_cuts([-1], lengths), resolve_end_cuts([2], lengths),
                           resolve_cuts([2, -1], lengths), resolve_cuts([-1], lengths)], axis=1)
    assert cuts.dtype == np.int64 and cuts.flags.c_contiguous and cuts.shape == (14, 2 + 2 + 3 + 2)
    np.testing.assert_array_equal(cuts, want)
    S = nat.FR_SIEVE_SERIES_CUTS
    assert spec.tolist() == [[nat.FR_SIEVE_END | S, 0, 2, 0, 0, 0], [nat.FR_SIEVE_END | S, 2, 2, 0, 0, 1],
                             [nat.FR_SIEVE_MAX | S, 4, 3, 0, 2, 2], [nat.FR_SIEVE_MIN | S, 7, 2, 2, 2, 4]]
    assert q.tolist() == [-np.inf, np.inf, -np.inf, np.inf]
    # END reads index + 1 - 1 < L_n; the bands end at the series' end
    assert (cuts[:, 1] == lengths).all() and (cuts[:, 3] == 2).all()
    assert (cuts[:, 4:] <= lengths[:, None]).all() and (cuts[:, 6] == lengths).all()
    # all lengths equal: the rows of the dense table
    dense = head.host_tables(9)[1]
    np.testing.assert_array_equal(head.host_series_tables(np.full(3, 9))[1], np.tile(dense, (3, 1)))


def test_end_cut_outside_a_series_is_an_index_error():
    import fruits_amd as fr
    from fruits_amd import nn
    head = nn._Head([fr.sieving.END([3])])
    with pytest.raises(IndexError, match=r"index 2 is out of bounds for axis 1 with size 2 .*series 1"):
        head.host_series_tables(np.array([5, 2, 4]))
    head.host_series_tables(np.array([5, 3, 4]))
