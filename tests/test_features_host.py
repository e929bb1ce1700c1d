"""The differentiable features without a GPU: the numpy reference of the selecting sieves against
a brute-force loop, the refusals of fruits_amd.nn.iss_features / FeatureLayer - all raised before
any device call -, the two ABI entries and their host-side argument checks."""
import os

import numpy as np
import pytest

import features_grad_ref as fg

HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")


# ---------------------------------------------------------------- the reference
def brute_pick(Y, sieves):
    """The definitions, one element at a time."""
    N, K, T = Y.shape
    feats, poss = [], []
    for n in range(N):
        for k in range(K):
            row, fs, ps = Y[n, k], [], []
            for s in sieves:
                cuts = fg.cut_row(s[1], T)
                for j in range(len(cuts) - 1):
                    if s[0] == "END":
                        idx = cuts[j + 1] - 1
                        idx = idx + T if idx < 0 else idx
                        fs.append(row[idx])
                        ps.append(idx)
                        continue
                    for b in range(len(s[2]) - 1):
                        best, at = None, -1
                        for t in range(max(cuts[j], 0), min(cuts[j + 1], T)):
                            v = row[t]
                            if not (s[2][b] < v <= s[2][b + 1]):
                                continue
                            # strictly better only: the first of equal extremes stays
                            if best is None or (v > best if s[0] == "MAX" else v < best):
                                best, at = v, t
                        fs.append(0.0 if best is None else best)
                        ps.append(at)
            feats.append(fs)
            poss.append(ps)
    F = len(feats[0])
    return np.array(feats).reshape(N, K, F), np.array(poss, dtype=np.int32).reshape(N, K, F)


def sieve_list(T):
    h = T // 2 or 1
    return [("END", (-1,)), ("END", (1, h, -1)), ("MAX", (-1,), (-INF, INF)),
            ("MIN", (h, -1), (-INF, INF)), ("MAX", (-1,), (-INF, 0.0, INF))]


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8, 13])
def test_pick_equals_the_brute_force_loop(T):
    rng = np.random.default_rng([1, T])
    Y = rng.integers(-2, 3, size=(3, 4, T)).astype(np.float64)       # ties everywhere
    Y[0, 0] = np.abs(Y[0, 0]) + 1.0                                  # an empty band (-inf, 0]
    Y[1, 1] = -np.abs(Y[1, 1])                                       # an empty band (0, inf)
    sieves = sieve_list(T) + [("MIN", (-1,), (-INF, -1.0, 1.0, INF)), ("MAX", (2, 2, -1), (-INF, INF))]
    feats, pos = fg.pick(Y, sieves)
    want_f, want_p = brute_pick(Y, sieves)
    assert feats.shape == pos.shape == (3, 4, fg.nfeatures(sieves)) and pos.dtype == np.int32
    np.testing.assert_array_equal(feats, want_f)
    np.testing.assert_array_equal(pos, want_p)
    assert (pos == -1).any() and ((pos >= 0) & (pos < T) | (pos == -1)).all()
    # a feature is the element at its position
    n, k, f = np.nonzero(pos >= 0)
    np.testing.assert_array_equal(feats[n, k, f], Y[n, k, pos[n, k, f]])
    assert (feats[pos < 0] == 0.0).all()
    if T >= 5:
        assert (fg.attained(Y, sieves) > 1).any()


def test_pick_takes_the_first_of_equal_extremes_and_signed_zeros_tie():
    Y = np.array([[[1.0, 3.0, 3.0, -2.0, -2.0, 3.0], [-0.0, 0.0, -0.0, 0.0, 0.0, -0.0]]])
    feats, pos = fg.pick(Y, [("MAX", (-1,), (-INF, INF)), ("MIN", (-1,), (-INF, INF)),
                             ("MAX", (3, -1), (-INF, INF)), ("MIN", (-1,), (-INF, 0.0, INF))])
    assert pos[0, 0].tolist() == [1, 3, 1, 5, 3, 0]
    assert feats[0, 0].tolist() == [3.0, -2.0, 3.0, 3.0, -2.0, 1.0]
    assert pos[0, 1].tolist() == [0, 0, 0, 3, 0, -1]
    assert fg.attained(Y, [("MAX", (-1,), (-INF, INF))])[0, :, 0].tolist() == [3, 6]


def test_dense_upstream_scatters_and_sums():
    pos = np.array([[[0, 2, 2, -1], [3, 3, 3, 0]]], dtype=np.int32)
    g = np.array([[1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0]])
    G = fg.dense_upstream(pos, g, 4)
    assert G.tolist() == [[[1.0, 0.0, 6.0, 0.0], [128.0, 0.0, 0.0, 112.0]]]
    np.testing.assert_array_equal(fg.dense_upstream(pos, g.reshape(1, 2, 4), 4), G)


def test_spec_of_reads_the_sieves():
    from fruits_amd.sieving import END, MAX, MIN
    assert fg.spec_of(END([1, -1])) == ("END", (1, -1))
    assert fg.spec_of(MAX([-1], q=(-1, 0, 1))) == ("MAX", (-1,), (-INF, 0.0, INF))
    fitted = MIN([3, -1], q=(-1, 0.25, 1))
    fitted.fit(np.arange(8.0)[None, :])
    assert fg.spec_of(fitted) == ("MIN", (3, -1), (-INF, 1.75, INF))
    assert fg.nfeatures([END([1, -1]), fitted]) == 2 + 4


# ---------------------------------------------------------------- fruits_amd.nn
def test_import_stays_lazy():
    import subprocess
    import sys
    code = ("import sys, fruits_amd\n"
            "assert 'torch' not in sys.modules and 'fruits_amd.nn' not in sys.modules\n"
            "import fruits_amd.nn as m\n"
            "assert callable(m.iss_features) and 'iss_features' in m.__all__\n"
            "assert 'FeatureLayer' in m.__all__\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(HERE))


def test_refusals_need_no_device():
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    from fruits_amd import sieving as sv
    from fruits_amd.iss.weighting import L1, Indices, Plateaus
    words = [fr.words.SimpleWord("[1][2]")]
    X = torch.zeros((2, 2, 5), dtype=torch.float64)
    good = [sv.END([-1]), sv.MAX([2, -1], q=(-1, 0, 1)), sv.MIN([-1])]
    configs = [{}, {"semiring": fr.semiring.Arctic()}, {"semiring": fr.semiring.Bayesian()},
               {"weighting": Indices()}, {"weighting": Plateaus(3, total=True)}]
    for kw in configs:
        # a supported configuration on a host tensor: the input checks of nn.iss, the device last
        layer = nn.FeatureLayer(words, fr.ISSMode.EXTENDED, good, **kw)
        assert list(layer.parameters()) == [] and "6 features" in repr(layer)
        with pytest.raises(TypeError, match="GPU"):
            nn.iss_features(X, words, fr.ISSMode.SINGLE, good, **kw)
        with pytest.raises(TypeError, match="GPU"):
            layer(X)
        with pytest.raises(TypeError, match="float64"):
            nn.iss_features(X.float(), words, fr.ISSMode.SINGLE, good, **kw)
        with pytest.raises(TypeError, match=r"\(N, D, T\)"):
            layer(X[0])
        with pytest.raises(IndexError, match="references dimension 2 but the input has only 1"):
            nn.iss_features(X[:, :1], words, fr.ISSMode.SINGLE, good, **kw)
        # the sieves are refused first, by name and with the reason
        refused = [
            (sv.END([0.5]), r"END.*float \(coquantile\) cut"),
            (sv.MAX([0.25, -1]), r"MAX.*float \(coquantile\) cut"),
            (sv.NPI(), "NPI.*NPI counts.*zero almost everywhere"),
            (sv.XPI(), "XPI.*zero almost everywhere"),
            (sv.LPI(), "LPI.*zero almost everywhere"),
            (sv.PPV(), "PPV.*zero almost everywhere"),
            (sv.CPV(), "CPV.*zero almost everywhere"),
            (sv.MPI(), "MPI.*no selection"),
            (sv.CUR(), "CUR.*no selection"),
            (sv.AVG(), "AVG.*no selection"),
            (sv.STD(), "STD.*no selection"),
            (sv.INC(sv.MAX()), "INC.*wrappers INC / INT"),
            (sv.INT(sv.END()), "INT.*wrappers INC / INT"),
        ]
        for sieve, text in refused:
            with pytest.raises(NotImplementedError, match=text):
                nn.iss_features(X, words, fr.ISSMode.SINGLE, [good[0], sieve], **kw)
            with pytest.raises(NotImplementedError, match=text):
                nn.FeatureLayer(words, fr.ISSMode.SINGLE, [sieve], **kw)
        with pytest.raises(NotImplementedError, match="lengths="):
            nn.iss_features(X, words, fr.ISSMode.SINGLE, good, lengths=np.array([5, 4]), **kw)
        with pytest.raises(NotImplementedError, match="lengths="):
            nn.FeatureLayer(words, fr.ISSMode.SINGLE, good, lengths=np.array([5, 4]), **kw)
        with pytest.raises(ValueError, match="at least one sieve"):
            nn.FeatureLayer(words, fr.ISSMode.SINGLE, [], **kw)
        with pytest.raises(TypeError, match="sequence of sieves"):
            nn.iss_features(X, words, fr.ISSMode.SINGLE, good[0], **kw)
        # more than 256 features per iterated sum
        with pytest.raises(ValueError, match="257 features.*at most 256"):
            nn.FeatureLayer(words, fr.ISSMode.SINGLE, [sv.END(list(range(1, 258)))], **kw)
        nn.FeatureLayer(words, fr.ISSMode.SINGLE, [sv.END(list(range(1, 257)))], **kw)
        # a sieve that needs its fit: the existing error, before the input is looked at
        unfitted = sv.MAX([-1], q=(-1, 0.5, 1))
        with pytest.raises(RuntimeError, match="not been fitted"):
            nn.iss_features(X, words, fr.ISSMode.SINGLE, [unfitted], **kw)
        with pytest.raises(RuntimeError, match="not been fitted"):
            nn.FeatureLayer(words, fr.ISSMode.SINGLE, [unfitted], **kw)(X)
        unfitted.fit(np.arange(10.0)[None, :])
        with pytest.raises(TypeError, match="GPU"):
            nn.iss_features(X, words, fr.ISSMode.SINGLE, [unfitted], **kw)
    # the configuration names the adjoint and is checked by the check of that adjoint
    with pytest.raises(NotImplementedError, match="depends on the input"):
        nn.FeatureLayer(words, fr.ISSMode.SINGLE, good, weighting=L1())
    with pytest.raises(NotImplementedError, match="argmax"):
        nn.iss_features(X, words, fr.ISSMode.SINGLE, good, semiring=fr.semiring.Arctic(argmax=True))
    with pytest.raises(NotImplementedError, match="generic"):
        nn.FeatureLayer([fr.words.Word("[DIM(1)][ABS(2)]")], fr.ISSMode.SINGLE, good)
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.FeatureLayer(fr.CosWISS(words, freqs=[0.5]), fr.ISSMode.SINGLE, good)
    # an ISS carries its configuration
    for op in (fr.ISS(words), fr.ISS(words, semiring=fr.semiring.Arctic()), fr.ISS(words, weighting=Indices())):
        with pytest.raises(TypeError, match="GPU"):
            nn.FeatureLayer(op, sieves=good)(X)


def test_head_tables():
    """The spec table of fr_sieve_pick: kinds, cut rows, thresholds and the features' columns."""
    from fruits_amd import _native as nat
    from fruits_amd import nn
    from fruits_amd import sieving as sv
    head = nn._Head([sv.END([1, 5, -1]), sv.MAX([-1], q=(-1, 0, 1)), sv.MIN([5, -1])])
    spec, cuts, q = head.host_tables(10)
    assert head.F == 3 + 2 + 2
    assert spec.tolist() == [[nat.FR_SIEVE_END, 0, 4, 0, 0, 0], [nat.FR_SIEVE_MAX, 4, 2, 0, 3, 3],
                             [nat.FR_SIEVE_MIN, 6, 3, 3, 2, 5]]
    assert cuts.tolist() == [0, 1, 5, 10, 0, 10, 0, 5, 10] and cuts.dtype == np.int64
    assert q.tolist() == [-INF, 0.0, INF, -INF, INF]
    with pytest.raises(IndexError, match="out of bounds"):
        nn._Head([sv.END([12])]).host_tables(10)


# ---------------------------------------------------------------- the ABI entries
def test_new_entries_are_exported():
    from fruits_amd import _native as nat
    L = nat.lib()
    with open(os.path.join(os.path.dirname(HERE), "include", "fruits_hip.h")) as f:
        header = f.read()
    for name in ("fr_sieve_pick", "fr_iss_backward_picked"):
        assert name in nat.EXPORTS and hasattr(L, name)
        assert header.count(f"int {name}(") == 1
    assert header.count("int fr_iss_backward(") == 1 and header.count("int fr_iss_backward_max(") == 1
    assert header.count("int fr_iss_backward_weighted(") == 1
    assert L.fr_version() >= 141


def test_sieve_pick_checks_before_any_device_call():
    import ctypes as C
    from fruits_amd import _native as nat
    L = nat.lib()
    i64, i32 = C.c_int64, C.c_int32
    p = C.c_void_p(4096)        # never dereferenced: every call below fails before a launch
    null = C.c_void_p(0)
    END, MAX, MIN = nat.FR_SIEVE_END, nat.FR_SIEVE_MAX, nat.FR_SIEVE_MIN
    good = [[END, 0, 2, 0, 0, 0], [MAX, 2, 3, 0, 3, 1], [MIN, 2, 3, 3, 2, 5]]

    def call(spec=good, K=2, N=3, T=9, A=p, spec_d=p, cuts=p, n_cuts=5, q=p, n_q=5, F=7, feat=p, pos=p,
             host=True):
        sp = np.ascontiguousarray(spec, dtype=np.int32)
        return L.fr_sieve_pick(A, i64(K), i64(N), i64(T), spec_d,
                               sp.ctypes.data_as(C.POINTER(C.c_int32)) if host else None,
                               i32(len(spec)), cuts, i64(n_cuts), q, i64(n_q), i32(F), feat, pos, null)

    def changed(s, col, value):
        out = [list(r) for r in good]
        out[s][col] = value
        return out

    cases = [
        (lambda: call(K=-1), nat.FR_E_ARG, "bad shape"),
        (lambda: call(T=0), nat.FR_E_ARG, "bad shape"),
        (lambda: call(spec=[]), nat.FR_E_ARG, "bad shape"),
        (lambda: call(F=0), nat.FR_E_ARG, "bad shape"),
        (lambda: call(F=257), nat.FR_E_LIMIT, "at most 256 features per row, not 257"),
        (lambda: call(T=2 ** 31), nat.FR_E_LIMIT, "positions are 32-bit"),
        (lambda: call(host=False), nat.FR_E_ARG, "null host table"),
        (lambda: call(changed(1, 0, nat.FR_SIEVE_NPI)), nat.FR_E_ARG, "sieve 1 is no selecting sieve"),
        (lambda: call(changed(0, 0, nat.FR_SIEVE_CUR)), nat.FR_E_ARG, "sieve 0 is no selecting sieve"),
        (lambda: call(changed(2, 0, nat.FR_SIEVE_PPV)), nat.FR_E_ARG, "sieve 2 is no selecting sieve"),
        (lambda: call(changed(0, 2, 1)), nat.FR_E_ARG, "sieve 0 has a cut row outside the cut table"),
        (lambda: call(changed(1, 1, -1)), nat.FR_E_ARG, "sieve 1 has a cut row outside the cut table"),
        (lambda: call(n_cuts=4), nat.FR_E_ARG, "sieve 1 has a cut row outside the cut table"),
        (lambda: call(changed(1, 4, 1)), nat.FR_E_ARG, "sieve 1 has thresholds outside the threshold table"),
        (lambda: call(n_q=4), nat.FR_E_ARG, "sieve 2 has thresholds outside the threshold table"),
        (lambda: call(changed(2, 3, -2)), nat.FR_E_ARG, "sieve 2 has thresholds outside"),
        (lambda: call(changed(2, 5, 4)), nat.FR_E_ARG, "sieve 2 begins at feature 4, not at 5"),
        (lambda: call(F=8), nat.FR_E_ARG, "the sieves have 7 features, not F = 8"),
        (lambda: call(F=6), nat.FR_E_ARG, "the sieves have more than 6 features, not F = 6"),
        (lambda: call(A=null), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(spec_d=null), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(cuts=null), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(q=null), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(feat=null), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(pos=null), nat.FR_E_ARG, "null device pointer"),
    ]
    for fn, code, text in cases:
        assert fn() == code, text
        assert text in nat.last_error(), (text, nat.last_error())
        assert nat.last_error().startswith("fr_sieve_pick: ")
    # nothing to do: no rows - after the same checks
    assert call(K=0, A=null, feat=null, pos=null) == 0
    assert call(N=0, A=null, feat=null, pos=null) == 0
    assert call(N=0, F=8) == nat.FR_E_ARG


def test_picked_entry_checks_before_any_device_call():
    """fr_iss_backward_picked dispatches on the plan's kind and validates like the entry of that
    kind, plus the pairs - all on the host."""
    import ctypes as C
    from fruits_amd import _native as nat
    L = nat.lib()
    i64, i32 = C.c_int64, C.c_int32
    p = C.c_void_p(4096)        # never dereferenced: every call below fails before a launch
    null = C.c_void_p(0)
    tab = lambda *rows: np.array(rows, dtype=np.int32)
    f32 = lambda *v: np.array(v, dtype=np.float32)
    tables = [tab([1]), tab([1, 0], [0, 1])]
    rows = np.array([1], dtype=np.int32)

    def call(plan, X=p, N=2, D=2, T=5, S=p, lk=p, lr=1, pos=p, w=p, K=1, F=3, rp=rows,
             Cs=C.c_void_p(12288), A=C.c_void_p(16384), aux=C.c_void_p(20480), dX=None):
        return L.fr_iss_backward_picked(
            plan._h if plan is not None else None, X, i64(N), i64(D), i64(T), S, lk, i64(lr), pos, w,
            i64(K), i32(F), rp.ctypes.data_as(C.POINTER(C.c_int32)) if rp is not None else None,
            Cs, A, aux, C.c_void_p(8192) if dX is None else dX, null)

    plans = {
        "reals": nat.Plan(tables, [1, 1]),
        "arctic": nat.Plan(tables, [1, 1], None, nat.FR_W_NONE, arctic=True),
        "bayesian": nat.Plan(tables, [1, 1], None, nat.FR_W_NONE, bayesian=True),
        "nontotal": nat.Plan(tables, [1, 1], [f32(1.0), f32(1.0, 0.5)], nat.FR_W_NONTOTAL),
        "total": nat.Plan(tables, [1, 1], [f32(1.0), f32(1.0, 0.5)], nat.FR_W_TOTAL),
    }
    for name, prefix in plans.items():
        weighted = name in ("nontotal", "total")
        assert prefix.nodes == 2
        cases = [
            (lambda: call(prefix, N=-1), nat.FR_E_ARG, "bad shape"),
            (lambda: call(prefix, D=0), nat.FR_E_ARG, "bad shape"),
            (lambda: call(prefix, K=-1), nat.FR_E_ARG, "bad shape"),
            (lambda: call(prefix, F=0), nat.FR_E_ARG, "at least one (position, weight) pair"),
            (lambda: call(prefix, F=-4), nat.FR_E_ARG, "at least one (position, weight) pair"),
            (lambda: call(prefix, F=257), nat.FR_E_LIMIT, "at most 256 pairs per row, not 257"),
            (lambda: call(prefix, T=2 ** 31), nat.FR_E_LIMIT, "positions are 32-bit"),
            (lambda: call(prefix, rp=None), nat.FR_E_ARG, "null host table"),
            (lambda: call(prefix, D=1), nat.FR_E_DIM, "references dimension 2 but the input has only 1"),
            (lambda: call(prefix, X=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, pos=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, w=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, A=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, dX=p), nat.FR_E_ARG, "must not alias"),
            (lambda: call(prefix, rp=np.array([2], dtype=np.int32)), nat.FR_E_ARG, "names prefix 2 of 2"),
        ]
        if weighted:
            cases += [
                (lambda: call(prefix, lr=3), nat.FR_E_ARG, "1 or N rows, not 3"),
                (lambda: call(prefix, lk=null), nat.FR_E_ARG, "null device pointer"),
                (lambda: call(prefix, Cs=null), nat.FR_E_ARG, "null device pointer"),
                (lambda: call(prefix, aux=null), nat.FR_E_ARG, "null device pointer"),
                (lambda: call(prefix, A=C.c_void_p(12288)), nat.FR_E_ARG, "distinct buffers"),
            ]
        else:
            cases += [(lambda: call(prefix, S=null), nat.FR_E_ARG, "null device pointer")]
        for fn, code, text in cases:
            assert fn() == code, (name, text)
            assert text in nat.last_error(), (name, text, nat.last_error())
            assert nat.last_error().startswith("fr_iss_backward_picked: ")
        # the pointers of the other kinds are not looked at
        unused = dict(lk=null, lr=0, Cs=null, aux=null) if not weighted else dict(S=null)
        assert call(prefix, T=0, **unused) == 0
        assert call(prefix, N=0, X=null, pos=null, w=null, A=null, **unused) == 0
        assert call(prefix, T=0, rp=np.array([7], dtype=np.int32)) == nat.FR_E_ARG
    # wrong plans
    wrong = [
        (None, "null plan"),
        (nat.Plan([tab([1, 0], [0, 1])], [1]), "not a prefix plan"),
        (nat.CosPlan([tab([1])], [0.5], 1, False), "a CosWISS plan has no backward pass"),
        (nat.Plan([tab([1])], [1], [f32(1.0)], nat.FR_W_TOTAL, arctic=True),
         "fr_iss_backward_max differentiates the unweighted ones"),
    ]
    for plan, text in wrong:
        assert call(plan) == nat.FR_E_ARG, text
        assert text in nat.last_error() and nat.last_error().startswith("fr_iss_backward_picked: ")
    # the dense entries keep their texts
    assert L.fr_iss_backward(plans["total"]._h, p, i64(2), i64(2), i64(5), p, p, i64(1), i64(5), i64(5), i64(1),
                             rows.ctypes.data_as(C.POINTER(C.c_int32)), p, C.c_void_p(8192), null) == nat.FR_E_ARG
    assert "fr_iss_backward: the plan is not an unweighted Reals trie plan" in nat.last_error()
