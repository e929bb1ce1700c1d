"""Host tests of the band features (fruits_amd.nn.iss_band_features, fr_sieve_heads,
fr_sieve_heads_adjoint): the numpy reference against a brute-force loop, the
oracle and the reference's golden CUR numbers; its gradient against central differences in exact
rational arithmetic; the refusals; the ABI entries' host checks."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import heads_grad_ref as hg

HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")

# segments that start past 0, a band split at 0, every order the issue names, selecting sieves
SIEVES = [
    ("MPI", (-1,), (-INF, INF), 0),
    ("MPI", (3, -1), (-INF, 0.0, INF), 1),
    ("MPI", (-1,), (-INF, 0.0, INF), 2),
    ("MPI", (5, -1), (-INF, INF), 8),
    ("CUR", (-1,), (-INF, INF)),
    ("CUR", (1, 4, -1), (-INF, 0.0, INF)),
    ("END", (-1,)),
    ("MAX", (-1,), (-INF, INF)),
    ("MIN", (4, -1), (-INF, 0.0, INF)),
]


def rows(N, K, T, seed, integer=True):
    rng = np.random.default_rng([seed, N, K, T])
    if integer:
        return rng.integers(-4, 5, size=(N, K, T)).astype(np.float64)
    return rng.standard_normal((N, K, T))


# ---------------------------------------------------------------- the reference itself
def brute_heads(Y, sieves):
    """Element by element, in Python floats."""
    N, K, T = Y.shape
    feats = np.zeros((N, K, hg.nfeatures(sieves)))
    comp = np.zeros((N, K, hg.nfeatures(sieves)), dtype=np.int32)
    for n in range(N):
        for k in range(K):
            f = 0
            for s in sieves:
                D = [float(v) for v in Y[n, k]]
                for _ in range(hg.order_of(s)):
                    D = [0.0] + [D[t] - D[t - 1] for t in range(1, T)]
                cut = hg.fg.cut_row(s[1], T)
                for j in range(len(cut) - 1):
                    if s[0] == "END":
                        p = cut[j + 1] - 1
                        p += T if p < 0 else 0
                        feats[n, k, f], comp[n, k, f] = D[p], p
                        f += 1
                        continue
                    for b in range(len(s[2]) - 1):
                        inside = [t for t in range(max(cut[j], 0), min(cut[j + 1], T)) if s[2][b] < D[t] <= s[2][b + 1]]
                        vals = [D[t] for t in inside]
                        if s[0] == "MPI":
                            feats[n, k, f] = sum(vals) / len(vals) if vals else 0.0
                            comp[n, k, f] = len(vals)
                        elif s[0] == "CUR":
                            feats[n, k, f] = sum(v * v for v in vals)
                            comp[n, k, f] = len(vals)
                        elif vals:
                            ext = max(vals) if s[0] == "MAX" else min(vals)
                            feats[n, k, f], comp[n, k, f] = ext, inside[vals.index(ext)]
                        else:
                            comp[n, k, f] = -1
                        f += 1
    return feats, comp


@pytest.mark.parametrize("T", [1, 2, 3, 9, 12])
def test_heads_against_a_brute_force_loop(T):
    Y = rows(3, 2, T, seed=1)
    feats, comp = hg.heads(Y, SIEVES)
    want_f, want_c = brute_heads(Y, SIEVES)
    assert comp.dtype == np.int32 and feats.shape == comp.shape == (3, 2, hg.nfeatures(SIEVES))
    np.testing.assert_array_equal(comp, want_c)
    np.testing.assert_array_equal(feats, want_f)          # (small integers: every sum is exact)
    Yr = rows(3, 2, T, seed=2, integer=False)
    feats, comp = hg.heads(Yr, SIEVES)
    want_f, want_c = brute_heads(Yr, SIEVES)
    np.testing.assert_array_equal(comp, want_c)
    np.testing.assert_allclose(feats, want_f, rtol=1e-14, atol=0)


@pytest.mark.parametrize("inc", [0, 1, 2, 8])
def test_mpi_against_the_oracle(inc):
    from oracle import ref_numpy as orc
    T, q = 40, (-INF, -0.5, 0.0, INF)
    A = rows(6, 1, T, seed=3 + inc, integer=False)[:, 0]
    spec = ("MPI", (7, 20, -1), q, inc)
    feats, comp = hg.heads(A[:, None, :], [spec])
    cuts = np.tile(np.asarray(hg.fg.cut_row(spec[1], T), dtype=np.int64), (6, 1))
    want = orc.mpi_backend(orc.pre_transform(A, inc), cuts, np.asarray(q))
    np.testing.assert_allclose(feats[:, 0], want, rtol=1e-13, atol=0)
    np.testing.assert_array_equal(hg.increments(A, inc), orc.pre_transform(A, inc))
    assert (comp >= 0).all() and comp.sum() == 6 * T


def test_cur_against_the_golden_numbers():
    with open(os.path.join(HERE, "golden", "golden_curvature.json")) as f:
        manifest = json.load(f)
    arrays = np.load(os.path.join(HERE, "golden", "golden_curvature.npz"))
    seen = 0
    for case in manifest["sieve"]:
        spec = case["spec"]
        cut = spec["kw"].get("cut", -1)
        cut = tuple(cut) if isinstance(cut, list) else (cut,)
        if spec["kind"] not in ("CUR", "AVG", "STD") or any(isinstance(c, float) for c in cut):
            continue
        q = tuple(INF if v == "inf" else (-INF if v == "-inf" else v) for v in case["quantiles"])
        feats, _ = hg.heads(arrays[case["x"]][:, None, :], [("CUR", cut, q)])
        np.testing.assert_allclose(feats[:, 0], arrays[case["out"]], rtol=1e-12, atol=0, err_msg=case["name"])
        seen += 1
    assert seen >= 20


# ---------------------------------------------------------------- the gradient, exactly
def fraction_features(row, sieves, held):
    """The features of ``row`` (a list of Fractions), each band sieve's over the elements
    ``held[f]`` and each selecting one's at the position ``held[f]``."""
    T, out, f = len(row), [], 0
    for s in sieves:
        D = list(row)
        for _ in range(hg.order_of(s)):
            D = [Fraction(0)] + [D[t] - D[t - 1] for t in range(1, T)]
        for _ in range(len(s[1]) * (1 if s[0] == "END" else len(s[2]) - 1)):
            if s[0] == "MPI":
                out.append(sum((D[t] for t in held[f]), Fraction(0)) / len(held[f]) if held[f] else Fraction(0))
            elif s[0] == "CUR":
                out.append(sum((D[t] * D[t] for t in held[f]), Fraction(0)))
            else:
                out.append(D[held[f]] if held[f] >= 0 else Fraction(0))
            f += 1
    return out


@pytest.mark.parametrize("T", [2, 3, 9, 12])
def test_band_upstream_against_exact_central_differences(T):
    """MPI is linear and CUR quadratic on a fixed mask, a selecting feature one element: central
    differences in rational arithmetic ARE the derivative.  The step is smaller than the distance
    of every D[t] to every threshold, so no element changes its band; integer gradients whose MPI
    columns are multiples of the count make every operation of band_upstream exact."""
    N, K = 2, 2
    rng = np.random.default_rng([7, T])
    # integers, every other step moved by 1/4: D of the orders 1 and 2 - the sieves with a band
    # split at 0 - is an integer +- 1/4 or +- 1/2 behind t = 0, never 0
    Y = rng.integers(-4, 5, size=(N, K, T)).astype(np.float64)
    Y += 0.25 * (np.arange(T) % 2)
    feats, comp = hg.heads(Y, SIEVES)
    dist = hg.threshold_distance(Y, SIEVES)
    h = Fraction(1, 1 << 12)
    # E^8 of a unit step moves an element by at most 2^8 h
    assert dist > float(h) * 2 ** 8, dist
    F = comp.shape[-1]
    kinds = [s[0] for s in SIEVES for _ in range(len(s[1]) * (1 if s[0] == "END" else len(s[2]) - 1))]
    g = rng.integers(-3, 4, size=(N, K, F)).astype(np.float64)
    for f, kind in enumerate(kinds):
        if kind == "MPI":
            g[:, :, f] *= np.maximum(comp[:, :, f], 1)
    G = hg.band_upstream(Y, SIEVES, comp, g)
    assert np.abs(G).max() > 0
    for n in range(N):
        for k in range(K):
            # the masks and positions of the unperturbed row
            held, f = [], 0
            for s in SIEVES:
                if s[0] in hg.SELECTING:
                    for _ in range(len(s[1]) * (1 if s[0] == "END" else len(s[2]) - 1)):
                        held.append(int(comp[n, k, f]))
                        f += 1
                    continue
                D = hg.increments(Y[n:n + 1, k:k + 1], hg.order_of(s))
                for mask in hg.masks(D, s):
                    held.append([int(t) for t in np.nonzero(mask[0, 0])[0]])
                    assert len(held[-1]) == comp[n, k, f]
                    f += 1
            row = [Fraction(float(v)) for v in Y[n, k]]
            gf = [Fraction(float(v)) for v in g[n, k]]
            for t in range(T):
                up = fraction_features(row[:t] + [row[t] + h] + row[t + 1:], SIEVES, held)
                down = fraction_features(row[:t] + [row[t] - h] + row[t + 1:], SIEVES, held)
                want = sum(((a - b) / (2 * h) * w for a, b, w in zip(up, down, gf)), Fraction(0))
                assert Fraction(float(G[n, k, t])) == want, (n, k, t)


def test_empty_bands_carry_no_gradient():
    # a positive rising row: the band (-inf, 0] of its increments is empty
    Y = np.cumsum(np.ones((1, 1, 9)), axis=-1)
    sieves = [("MPI", (-1,), (-INF, -1.0, INF), 1), ("CUR", (-1,), (-INF, -1.0, INF))]
    feats, comp = hg.heads(Y, sieves)
    assert comp[0, 0].tolist() == [0, 9, 0, 9] and feats[0, 0, 0] == 0.0 and feats[0, 0, 2] == 0.0
    g = np.array([[[5.0, 0.0, 7.0, 0.0]]])
    G = hg.band_upstream(Y, sieves, comp, g)
    assert not G.any() and not np.signbit(G).any()
    g[0, 0, 1] = 9.0
    assert hg.band_upstream(Y, sieves, comp, g).any()


def test_ragged_reference_is_the_truncated_one():
    Y = rows(3, 2, 12, seed=5)
    lengths = np.array([1, 7, 12])
    feats, comp = hg.heads(Y, SIEVES[:5] + SIEVES[6:8], lengths)
    g = np.random.default_rng(6).standard_normal(feats.shape)
    G = hg.band_upstream(Y, SIEVES[:5] + SIEVES[6:8], comp, g, lengths)
    for n, L in enumerate(lengths):
        f1, c1 = hg.heads(Y[n:n + 1, :, :L], SIEVES[:5] + SIEVES[6:8])
        np.testing.assert_array_equal(feats[n:n + 1], f1)
        np.testing.assert_array_equal(comp[n:n + 1], c1)
        np.testing.assert_array_equal(G[n:n + 1, :, :L],
                                      hg.band_upstream(Y[n:n + 1, :, :L], SIEVES[:5] + SIEVES[6:8], c1, g[n:n + 1]))
        assert not G[n, :, L:].any() and not np.signbit(G[n, :, L:]).any()


# ---------------------------------------------------------------- refusals
def test_refusals_by_message():
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    from fruits_amd import sieving as sv
    from fruits_amd.iss.weighting import Indices
    words = [fr.words.SimpleWord("[1]"), fr.words.SimpleWord("[1][2]")]
    X = torch.zeros((2, 2, 9), dtype=torch.float64)
    good = [sv.MPI([-1], inc=1), sv.CUR([-1]), sv.END([-1])]
    for kw in ({}, {"semiring": fr.semiring.Arctic()}, {"weighting": Indices()}):
        refused = [
            (sv.MPI([-1], inc=-1), "MPI.*cumulated rows"),
            (sv.MPI([-1], inc=9), "MPI.*only inc 0 ... 8"),
            (sv.MPI([0.5, -1]), "float \\(coquantile\\) cut"),
            (sv.CUR([0.5, -1]), "float \\(coquantile\\) cut"),
            (sv.NPI(), "NPI counts"),
            (sv.XPI(), "XPI counts"),
            (sv.LPI(), "LPI counts"),
            (sv.PPV(), "PPV counts"),
            (sv.CPV(), "CPV counts"),
            (sv.INC(sv.MPI()), "INC.*wrappers INC / INT"),
            (sv.INT(sv.CUR()), "INT.*wrappers INC / INT"),
        ]
        for sieve, text in refused:
            with pytest.raises(NotImplementedError, match=text):
                nn.iss_band_features(X, words, fr.ISSMode.SINGLE, [good[0], sieve], **kw)
            with pytest.raises(NotImplementedError, match=text):
                nn.BandFeatureLayer(words, fr.ISSMode.SINGLE, [sieve], **kw)
            with pytest.raises(NotImplementedError, match=text):
                nn.iss_band_features_ragged(X, np.array([5, 9]), words, fr.ISSMode.SINGLE, [sieve], **kw)
        with pytest.raises(NotImplementedError, match="lengths="):
            nn.iss_band_features(X, words, fr.ISSMode.SINGLE, good, lengths=np.array([5, 4]), **kw)
        with pytest.raises(NotImplementedError, match="lengths="):
            nn.BandFeatureLayer(words, fr.ISSMode.SINGLE, good, lengths=np.array([5, 4]), **kw)
        with pytest.raises(ValueError, match="at least one sieve"):
            nn.BandFeatureLayer(words, fr.ISSMode.SINGLE, [], **kw)
        with pytest.raises(TypeError, match="sequence of sieves"):
            nn.iss_band_features(X, words, fr.ISSMode.SINGLE, good[0], **kw)
        with pytest.raises(ValueError, match="258 features.*at most 256"):
            nn.BandFeatureLayer(words, fr.ISSMode.SINGLE, [sv.MPI(list(range(1, 130)), q=(-1, 0, 1))], **kw)
        nn.BandFeatureLayer(words, fr.ISSMode.SINGLE, [sv.MPI(list(range(1, 129)), q=(-1, 0, 1))], **kw)
        unfitted = sv.MPI([-1], q=(-1, 0.5, 1))
        with pytest.raises(RuntimeError, match="not been fitted"):
            nn.iss_band_features(X, words, fr.ISSMode.SINGLE, [unfitted], **kw)
        with pytest.raises(RuntimeError, match="not been fitted"):
            nn.BandFeatureLayer(words, fr.ISSMode.SINGLE, [unfitted], **kw)(X)
        # everything accepted: the next refusal is the host tensor's
        for sieves in (good, [sv.AVG([-1]), sv.STD([3, -1]), sv.MAX([-1]), sv.MIN([-1])],
                       [sv.MPI([-1], inc=i) for i in (0, 8)], [sv.END([-1])]):
            with pytest.raises(TypeError, match="GPU"):
                nn.iss_band_features(X, words, fr.ISSMode.SINGLE, sieves, **kw)
            with pytest.raises(TypeError, match="GPU"):
                nn.BandFeatureLayer(words, fr.ISSMode.SINGLE, sieves, **kw)(X, lengths=np.array([5, 9]))
    # the selecting entries keep their refusals
    with pytest.raises(NotImplementedError, match="MPI.*no selection"):
        nn.iss_features(X, words, fr.ISSMode.SINGLE, [sv.MPI()])
    # the configuration is checked by the check of its adjoint
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.BandFeatureLayer(fr.CosWISS(words, freqs=[0.5]), fr.ISSMode.SINGLE, good)
    with pytest.raises(NotImplementedError, match="argmax"):
        nn.iss_band_features(X, words, fr.ISSMode.SINGLE, good, semiring=fr.semiring.Arctic(argmax=True))


def test_band_head_tables():
    from fruits_amd import _native as nat
    from fruits_amd import nn
    from fruits_amd import sieving as sv
    head = nn._BandHead([sv.MPI([5, -1], q=(-1, 0, 1), inc=3), sv.AVG([-1]), sv.END([1, -1]), sv.MIN([-1])])
    spec, cuts, q = head.host_tables(10)
    assert head.F == 4 + 1 + 2 + 1 and spec.dtype == np.int32 and spec.flags["C_CONTIGUOUS"]
    assert spec.tolist() == [[nat.FR_SIEVE_MPI, 0, 3, 0, 3, 0, 3], [nat.FR_SIEVE_CUR, 3, 2, 3, 2, 4, 2],
                             [nat.FR_SIEVE_END, 5, 3, 5, 0, 5, 0], [nat.FR_SIEVE_MIN, 8, 2, 5, 2, 7, 0]]
    assert cuts.tolist() == [0, 5, 10, 0, 10, 0, 1, 10, 0, 10]
    assert q.tolist() == [-INF, 0.0, INF, -INF, INF, -INF, INF]
    spec, cuts, q = head.host_series_tables(np.array([4, 10]))
    assert (spec[:, 0] & nat.FR_SIEVE_SERIES_CUTS).all() and spec[:, 6].tolist() == [3, 2, 0, 0]
    assert cuts.shape == (2, 10) and cuts[0].tolist() == [0, 4, 4, 0, 4, 0, 1, 4, 0, 4]
    # the selecting head's tables did not change
    assert nn._Head([sv.END([-1])]).host_tables(10)[0].shape == (1, 6)


# ---------------------------------------------------------------- the ABI entries
def test_new_entries_are_exported_and_declared_once():
    from fruits_amd import _native as nat
    L = nat.lib()
    with open(os.path.join(os.path.dirname(HERE), "include", "fruits_hip.h")) as f:
        header = f.read()
    for name in ("fr_sieve_heads", "fr_sieve_heads_adjoint"):
        assert nat.EXPORTS.count(name) == 1 and hasattr(L, name)
        assert header.count(f"int {name}(") == 1
    assert header.count("int fr_sieve_pick(") == 1
    assert L.fr_version() >= 145


def _abi():
    import ctypes as C
    from fruits_amd import _native as nat
    return C, nat, nat.lib(), C.c_void_p(4096), C.c_void_p(0)


def _good(nat):
    MPI, CUR, END, MAX = nat.FR_SIEVE_MPI, nat.FR_SIEVE_CUR, nat.FR_SIEVE_END, nat.FR_SIEVE_MAX
    return [[MPI, 0, 2, 0, 3, 0, 1], [CUR, 2, 3, 0, 3, 2, 2], [END, 0, 2, 0, 0, 6, 0], [MAX, 0, 2, 3, 2, 7, 0]]


def _shared_cases(nat, call, good):
    def changed(s, col, value):
        out = [list(r) for r in good]
        out[s][col] = value
        return out

    return [
        (lambda: call(K=-1), nat.FR_E_ARG, "bad shape"),
        (lambda: call(T=0), nat.FR_E_ARG, "bad shape"),
        (lambda: call(spec=[]), nat.FR_E_ARG, "bad shape"),
        (lambda: call(F=0), nat.FR_E_ARG, "bad shape"),
        (lambda: call(n_cuts=-1), nat.FR_E_ARG, "bad shape"),
        (lambda: call(F=257), nat.FR_E_LIMIT, "at most 256 features per row, not 257"),
        (lambda: call(T=2 ** 31), nat.FR_E_LIMIT, "32-bit, T is not"),
        (lambda: call(host=False), nat.FR_E_ARG, "null host table"),
        (lambda: call(changed(0, 0, nat.FR_SIEVE_NPI)), nat.FR_E_ARG, "sieve 0 is no head (END, MAX, MIN, MPI, CUR)"),
        (lambda: call(changed(1, 0, nat.FR_SIEVE_XPI)), nat.FR_E_ARG, "sieve 1 is no head"),
        (lambda: call(changed(3, 0, nat.FR_SIEVE_PPV)), nat.FR_E_ARG, "sieve 3 is no head"),
        (lambda: call(changed(0, 6, -1)), nat.FR_E_ARG, "sieve 0 has the differencing order -1, not 0 ... 8"),
        (lambda: call(changed(0, 6, 9)), nat.FR_E_ARG, "sieve 0 has the differencing order 9, not 0 ... 8"),
        (lambda: call(changed(1, 6, 1)), nat.FR_E_ARG, "sieve 1 has the differencing order 1, not 2"),
        (lambda: call(changed(2, 6, 1)), nat.FR_E_ARG, "sieve 2 has the differencing order 1, not 0"),
        (lambda: call(changed(3, 6, 2)), nat.FR_E_ARG, "sieve 3 has the differencing order 2, not 0"),
        (lambda: call(changed(0, 2, 1)), nat.FR_E_ARG, "sieve 0 has a cut row outside the cut table"),
        (lambda: call(changed(1, 1, -1)), nat.FR_E_ARG, "sieve 1 has a cut row outside the cut table"),
        (lambda: call(n_cuts=4), nat.FR_E_ARG, "sieve 1 has a cut row outside the cut table"),
        (lambda: call(changed(0, 4, 1)), nat.FR_E_ARG, "sieve 0 has thresholds outside the threshold table"),
        (lambda: call(n_q=4), nat.FR_E_ARG, "sieve 3 has thresholds outside the threshold table"),
        (lambda: call(changed(1, 3, -2)), nat.FR_E_ARG, "sieve 1 has thresholds outside"),
        (lambda: call(changed(2, 5, 5)), nat.FR_E_ARG, "sieve 2 begins at feature 5, not at 6"),
        (lambda: call(F=9), nat.FR_E_ARG, "the sieves have 8 features, not F = 9"),
        (lambda: call(F=7), nat.FR_E_ARG, "the sieves have more than 7 features, not F = 7"),
        (lambda: call(changed(1, 0, nat.FR_SIEVE_CUR | nat.FR_SIEVE_SERIES_CUTS)), nat.FR_E_ARG,
         "sieve 1 and sieve 0 differ in FR_SIEVE_SERIES_CUTS"),
        (lambda: call([[r[0] | nat.FR_SIEVE_SERIES_CUTS] + r[1:] for r in good], n_cuts=16), nat.FR_E_ARG,
         "n_cuts = 16 is no multiple of N = 3"),
        (lambda: call([[r[0] | nat.FR_SIEVE_SERIES_CUTS] + r[1:] for r in good], n_cuts=12), nat.FR_E_ARG,
         "sieve 1 has a cut row outside a series' row of the cut table"),
        (lambda: call(spec_d=False), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(cuts=False), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(q=False), nat.FR_E_ARG, "null device pointer"),
    ]


def test_sieve_heads_checks_before_any_device_call():
    C, nat, L, p, null = _abi()
    i64, i32 = C.c_int64, C.c_int32
    good = _good(nat)

    def call(spec=good, K=2, N=3, T=9, A=True, spec_d=True, cuts=True, n_cuts=5, q=True, n_q=5, F=8, feat=True,
             comp=True, host=True):
        ptr = lambda on: p if on else null          # (never dereferenced: every call fails before a launch)
        sp = np.ascontiguousarray(spec, dtype=np.int32)
        return L.fr_sieve_heads(ptr(A), i64(K), i64(N), i64(T), ptr(spec_d),
                                sp.ctypes.data_as(C.POINTER(C.c_int32)) if host else None, i32(len(spec)),
                                ptr(cuts), i64(n_cuts), ptr(q), i64(n_q), i32(F), ptr(feat), ptr(comp), null)

    cases = _shared_cases(nat, call, good) + [
        (lambda: call(A=False), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(feat=False), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(comp=False), nat.FR_E_ARG, "null device pointer"),
    ]
    for fn, code, text in cases:
        assert fn() == code, text
        assert text in nat.last_error(), (text, nat.last_error())
        assert nat.last_error().startswith("fr_sieve_heads: ")
    # nothing to do: no rows - after the same checks
    assert call(K=0, A=False, feat=False, comp=False) == 0
    assert call(N=0, A=False, feat=False, comp=False) == 0
    assert call(N=0, F=9) == nat.FR_E_ARG


def test_sieve_heads_adjoint_checks_before_any_device_call():
    C, nat, L, p, null = _abi()
    i64, i32 = C.c_int64, C.c_int32
    good = _good(nat)
    rows_at, G_at = C.c_void_p(1 << 20), C.c_void_p(2 << 20)      # (apart: no aliasing)

    def call(spec=good, K=2, N=3, T=9, V=4, rows=True, row_map=(3, 0), map_d=True, spec_d=True, cuts=True, n_cuts=5,
             q=True, n_q=5, F=8, comp=True, g=True, G=G_at, host=True):
        ptr = lambda on: p if on else null
        sp = np.ascontiguousarray(spec, dtype=np.int32)
        rm = None if row_map is None else np.ascontiguousarray(row_map, dtype=np.int32)
        return L.fr_sieve_heads_adjoint(
            rows_at if rows else null, i64(V), ptr(map_d), None if rm is None else rm.ctypes.data_as(C.POINTER(C.c_int32)),
            i64(K), i64(N), i64(T), ptr(spec_d), sp.ctypes.data_as(C.POINTER(C.c_int32)) if host else None,
            i32(len(spec)), ptr(cuts), i64(n_cuts), ptr(q), i64(n_q), i32(F), ptr(comp), ptr(g), null, G, null)

    cases = _shared_cases(nat, call, good) + [
        (lambda: call(V=-1), nat.FR_E_ARG, "bad shape"),
        (lambda: call(map_d=False), nat.FR_E_ARG, "the row map needs its host and its device copy"),
        (lambda: call(row_map=None), nat.FR_E_ARG, "the row map needs its host and its device copy"),
        (lambda: call(row_map=None, map_d=False), nat.FR_E_ARG, "without a row map the buffer holds the K = 2 rows, not V = 4"),
        (lambda: call(row_map=(3, 4)), nat.FR_E_ARG, "row 1 names row 4 of 4"),
        (lambda: call(row_map=(-1, 0)), nat.FR_E_ARG, "row 0 names row -1 of 4"),
        (lambda: call(rows=False), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(comp=False), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(g=False), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(G=null), nat.FR_E_ARG, "null device pointer"),
        (lambda: call(G=C.c_void_p((1 << 20) + 64)), nat.FR_E_ARG, "d_G must not alias"),
        (lambda: call(G=p), nat.FR_E_ARG, "d_G must not alias"),
    ]
    for fn, code, text in cases:
        assert fn() == code, text
        assert text in nat.last_error(), (text, nat.last_error())
        assert nat.last_error().startswith("fr_sieve_heads_adjoint: ")
    assert call(K=0, row_map=(), rows=False, comp=False, g=False, G=null) == 0
    assert call(N=0, rows=False, comp=False, g=False, G=null) == 0
    assert call(N=0, F=9) == nat.FR_E_ARG
