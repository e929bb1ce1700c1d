"""The backward pass of the cosine weighted iterated sums without a GPU: the long-double oracle of
the adjoint recursion against the definition in exact arithmetic, against the unweighted oracle
where the weight is 1, against a central difference of the reference's term-by-term forward pass;
the CosWISS contract of fr_iss_backward, the new fr_plan_info code, and the refusals of
fruits_amd.nn.cos_iss - all raised before any device call."""
import os

import numpy as np
import pytest

import coswiss_grad_ref as cg
import iss_grad_ref as gr

HERE = os.path.dirname(os.path.abspath(__file__))

WORDS = ["[1]", "[1][2]", "[12][1][-2]"]       # one, two and three letters; a product; a division


def exact_input(N, D, T, seed):
    """Integer-valued X from {-2 ... 2}; {+-0.5, +-1, +-2} in dimension 2, which WORDS divides by."""
    rng = np.random.default_rng([seed, N, D, T])
    X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    X[:, 1] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=(N, T))
    return X


def power_tables(F, T, seed):
    """'sin' and 'cos' tables (F, T) of zeros and signed powers of two: every product and sum of
    the recursion is a dyadic rational of few bits, exact in any float format."""
    rng = np.random.default_rng([seed, F, T])
    values = np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0])
    return rng.choice(values, size=(F, T)), rng.choice(values, size=(F, T))


# ---------------------------------------------------------------- the oracles
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_recursion_equals_definition(T, S, total):
    N, D, F = 2, 2, 2
    X = exact_input(N, D, T, seed=1)
    G = np.random.default_rng([2, T, S]).integers(-3, 4, size=(N, len(WORDS) * F, T)).astype(np.float64)
    tables = power_tables(F, T, seed=3)
    want = cg.grad_cos_bruteforce(X, G, WORDS, tables, S, total)
    got = gr.as_fractions(cg.coswiss_grad(X, G, WORDS, None, S, total, tables=tables))
    assert got.shape == want.shape == (N, D, T)
    assert (got == want).all(), (T, S, total)
    if T >= 4:
        assert any(v != 0 for v in want.ravel())
    if T == 5:
        # the weights matter: other tables, another gradient (swapping sin and cos would be none:
        # sin sin + cos cos is symmetric in the two)
        assert (cg.grad_cos_bruteforce(X, G, WORDS, power_tables(F, T, seed=4), S, total) != want).any()
        # ... and so does the weighting of the last letter
        assert (cg.grad_cos_bruteforce(X, G, WORDS, tables, S, not total) != want).any()


def test_magnitude_run_is_the_definition_on_magnitudes():
    """magnitude=True: |X|, |G| and tables of ones - the definition with every weight at its
    largest (no division: its coefficient keeps a sign in the definition)."""
    words, N, D, T, F, S = ["[1]", "[1][2]", "[12][1][2]"], 1, 2, 4, 2, 2
    X = exact_input(N, D, T, seed=4)
    G = np.random.default_rng(5).integers(-3, 4, size=(N, len(words) * F, T)).astype(np.float64)
    ones = (np.ones((F, T)), np.ones((F, T)))
    for total in (False, True):
        mag = gr.as_fractions(cg.coswiss_grad(X, G, words, None, S, total, magnitude=True,
                                              tables=power_tables(F, T, seed=6)))
        assert (mag == cg.grad_cos_bruteforce(np.abs(X), np.abs(G), words, ones, S, total)).all()


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("S", [1, 3])
def test_weight_one_is_the_unweighted_recursion(S, total):
    """sin = 0, cos = 1: q_S = 1 and every other q_m = 0 - the recursion is that of iss_grad_ref,
    bit for bit on integer-valued inputs."""
    N, D, T = 3, 2, 40
    X = exact_input(N, D, T, seed=7)
    G = np.random.default_rng(8).integers(-3, 4, size=(N, len(WORDS), T)).astype(np.float64)
    tables = (np.zeros((1, T)), np.ones((1, T)))
    got = cg.coswiss_grad(X, G, WORDS, None, S, total, tables=tables)
    want = gr.iss_grad(X, G, WORDS, "SINGLE")
    assert np.array_equal(got, want) and np.abs(want).max() > 0
    # the infinite frequency is that case: the angle is exactly 0
    assert np.array_equal(cg.coswiss_grad(X, G, WORDS, [np.inf], S, total), want)
    assert np.array_equal(cg.coswiss_forward(X, WORDS, [np.inf], S, total).astype(np.float64),
                          gr.orc.iss_transform(X, WORDS, "SINGLE").transpose(1, 0, 2))


def coswiss_terms(X, word_strings, freqs, S, total, dtype=gr.HP):
    """The forward pass as the reference evaluates it (fruits/iss/cos.py:11-49), term by term: for
    every combination of one expansion term C(S, m) (sin sin)^(S-m) (cos cos)^m per pair of
    consecutive letters (and one more pair, last letter and output step, with total weighting) an
    ordinary iterated sum over the input times powers of sin and cos, the terms added up with
    their coefficients.  (N, W * F, T) in ``dtype``."""
    from itertools import product
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    N, _, T = X.shape
    sin_t, cos_t = cg.trig_tables(T, freqs, dtype)
    out = []
    for letters in cg.word_letters(word_strings):
        L = len(letters)
        links = L - 1 + (1 if total else 0)
        for f in range(len(freqs)):
            row = np.zeros((N, T), dtype=dtype)
            for ms in product(range(S + 1), repeat=links):
                coef, ps, pc = 1, [0] * (L + 1), [0] * (L + 1)      # powers of sin / cos per position
                for j, m in enumerate(ms):
                    coef *= cg.binomials(S)[m]
                    for at in (j, j + 1):
                        ps[at] += S - m
                        pc[at] += m
                tmp = np.ones((N, T), dtype=dtype)
                for k in range(L):
                    if k > 0:
                        tmp = gr._shift(tmp)
                    tmp = tmp * gr._letter(X, letters[k]) * sin_t[f] ** ps[k] * cos_t[f] ** pc[k]
                    tmp = np.cumsum(tmp, axis=1)
                row = row + coef * (tmp * sin_t[f] ** ps[L] * cos_t[f] ** pc[L])
            out.append(row)
    return np.stack(out, axis=1)


def test_terms_oracle_is_the_reference_oracle_and_the_recursion():
    X = np.random.default_rng(9).uniform(0.5, 1.5, size=(2, 2, 9))
    for S in (1, 2, 3):
        for total in (False, True):
            terms = coswiss_terms(X, WORDS, [0.25, 1.5], S, total)
            ref = gr.orc.coswiss_transform(X, WORDS, [0.25, 1.5], S, total, dtype=gr.HP).transpose(1, 0, 2)
            fac = cg.coswiss_forward(X, WORDS, [0.25, 1.5], S, total)
            scale = np.abs(ref).max()
            assert np.abs(terms - ref).max() <= 1e-15 * scale and np.abs(fac - ref).max() <= 1e-15 * scale


def test_recursion_is_the_gradient_of_the_forward_oracle():
    """A central difference of the term-by-term forward pass agrees with the adjoint recursion:
    the factorisation, the binomials and the shift are tied to the reference's formulation."""
    N, D, T = 2, 2, 7
    rng = np.random.default_rng(10)
    X = rng.uniform(0.5, 1.5, size=(N, D, T))
    freqs = [0.25, 1.5]
    for S in (1, 2, 3):
        for total in (False, True):
            G = rng.standard_normal((N, len(WORDS) * len(freqs), T))

            def loss(Z):
                return float((coswiss_terms(Z, WORDS, freqs, S, total) * G).sum())

            got = cg.coswiss_grad(X, G, WORDS, freqs, S, total).astype(np.float64)
            h = 1e-6
            for at in [(0, 0, 0), (1, 1, 3), (0, 1, 6), (1, 0, 5)]:
                Zp, Zm = X.copy(), X.copy()
                Zp[at] += h
                Zm[at] -= h
                fd = (loss(Zp) - loss(Zm)) / (2 * h)
                assert abs(fd - got[at]) <= 1e-7 * max(1.0, abs(got[at])), (S, total, at, fd, got[at])


def test_n_ops_grad_cos_counts():
    # one letter, non-total: no link, no trig - 9 + 1 + 2 + 0 + 3 + 0 + (1 - 1)
    assert cg.n_ops_grad_cos(["[1]"], 10, [1.0], 2, False, 1) == 15
    # ... total: one link of 4 + S and two q_m of S (1 + 3 ceil(pi) + U) each
    assert cg.n_ops_grad_cos(["[1]"], 10, [1.0], 2, True, 1) == 15 + 6 + 2 * 2 * (1 + 12 + 1)
    # the smallest frequency scales the angle's roundings: pi / 0.25 -> 13
    assert cg._trig_ulps([0.25, 1.5], 2) == 3 * 13 + 2
    n = cg.n_ops_grad_cos(WORDS, 100, [0.25, 1.5], 3, True, 0, E=2)
    assert n == 3 * 99 + 4 + 2 + 3 * 7 + 3 + 1 + (2 * 6 - 1) + 2 * 3 * 3 * (1 + 39)
    assert cg.n_ops_cos(WORDS, 100, [0.25, 1.5], 3, True, 0) == 3 * 99 + 4 + 3 * 7 + 2 * 3 * 3 * (1 + 39)


def test_bound_holds_for_float64_and_can_fail():
    """The float64 run of the recursion on float64 tables lies within the derived bound of the
    long-double one (numpy's sin / cos: 1 ulp); a relative error of 1e-9, or a dropped binomial
    coefficient, lies outside."""
    import iss_bounds as ib
    N, D, T, freqs = 2, 2, 600, [0.25, 1.5]
    rng = np.random.default_rng(11)
    X = rng.uniform(0.5, 1.5, size=(N, D, T))
    G = rng.standard_normal((N, len(WORDS) * len(freqs), T))
    sin64, cos64 = cg.trig_tables(T, freqs, np.float64)
    for S in (1, 3):
        for total in (False, True):
            n = cg.n_ops_grad_cos(WORDS, T, freqs, S, total, U=1)
            hp = cg.coswiss_grad(X, G, WORDS, freqs, S, total)
            A = cg.coswiss_grad(X, G, WORDS, freqs, S, total, magnitude=True)
            f64 = cg.coswiss_grad(X, G, WORDS, freqs, S, total, tables=(sin64, cos64), dtype=np.float64)
            ib.check_bound(f64, hp, A, n, f"float64 recursion S={S} total={total}")
            assert ib.violates(f64 * (1 + 1e-9), hp, A, n) or np.abs(hp).max() < 1e-9 * A.max()
            assert ib.violates(cg.coswiss_grad(X, G, WORDS, freqs, S, not total, dtype=np.float64), hp, A, n)


# ---------------------------------------------------------------- the ABI
def test_header_states_both_contracts():
    from fruits_amd import _native as nat
    L = nat.lib()
    with open(os.path.join(os.path.dirname(HERE), "include", "fruits_hip.h")) as f:
        header = f.read()
    assert header.count("int fr_iss_backward(") == 1
    doc = header[header.index("backward pass"):header.index("int fr_iss_backward(")]
    assert "CosWISS plan" in doc and "FR_INFO_GRAD_ROWS" in doc and "fr_plan_create_coswiss" in doc
    assert "#define FR_INFO_GRAD_ROWS 14" in header and nat.FR_INFO_GRAD_ROWS == 14
    assert L.fr_version() >= 143


def test_info_reports_the_backward_scratch():
    from fruits_amd import _native as nat
    tab = lambda *rows: np.array(rows, dtype=np.int32)
    # two words of 1 + 2 letters, two frequencies: u of the one letter behind a first (x F),
    # dz of the three letters (x F) and 2 F rows for the trig tables
    plan = nat.CosPlan([tab([1]), tab([1, 0], [0, 1])], [0.5, 2.0], 2, True)
    assert plan.rows == 4
    assert nat.coswiss_grad_rows(plan) == (2, 3 * 2 + 2 * 2)
    assert plan.info(nat.FR_INFO_GRAD_ROWS) == (2 << 32) | 10
    assert nat.coswiss_grad_rows(nat.CosPlan([tab([1])], [0.5], 1, False)) == (0, 1 + 2)
    # any other plan has none
    assert nat.Plan([tab([1])], [1]).info(nat.FR_INFO_GRAD_ROWS) == 0


def test_cos_plan_checks_before_any_device_call():
    """fr_iss_backward handed a CosWISS plan validates shapes, pointers, limits and the row map
    on the host, in the order and with the prefix of the trie plans' contract."""
    import ctypes as C
    from fruits_amd import _native as nat
    L = nat.lib()
    i64 = C.c_int64
    p = C.c_void_p(4096)        # never dereferenced: every call below fails before a launch
    null = C.c_void_p(0)
    tab = lambda *rows: np.array(rows, dtype=np.int32)
    rows = np.array([1, 0, 1], dtype=np.int32)        # a row named twice

    def call(plan, X=p, N=2, D=2, T=5, S=C.c_void_p(12288), G=p, K=3, sn=15, sk=5, st=1, rp=rows,
             A=C.c_void_p(16384), dX=None):
        return L.fr_iss_backward(
            plan._h if plan is not None else None, X, i64(N), i64(D), i64(T), S, G, i64(K), i64(sn),
            i64(sk), i64(st), rp.ctypes.data_as(C.POINTER(C.c_int32)) if rp is not None else None,
            A, C.c_void_p(8192) if dX is None else dX, null)

    for total in (False, True):
        cos = nat.CosPlan([tab([1, 0], [0, 1])], [0.5, 2.0], 2, total)
        one_letter = nat.CosPlan([tab([1])], [0.5], 2, total)
        steep = nat.CosPlan([tab([1])], [0.5], 9, total)
        long_word = nat.CosPlan([tab(*[[1]] * 17)], [0.5], 2, total)
        ffn = nat.CosPlan([tab([1])], [0.5], 2, total)
        nat.check(L.fr_coswiss_set_input_stride(ffn._h, i64(40)))
        ragged = nat.CosPlan([tab([1])], [0.5], 2, total)
        nat.check(L.fr_plan_set_grad_lengths(ragged._h, p, i64(2)))
        cases = [
            (lambda: call(cos, N=-1), nat.FR_E_ARG, "bad shape"),
            (lambda: call(cos, D=0), nat.FR_E_ARG, "bad shape"),
            (lambda: call(cos, sk=-1), nat.FR_E_ARG, "bad shape"),
            (lambda: call(cos, rp=None), nat.FR_E_ARG, "null host table"),
            (lambda: call(cos, D=1), nat.FR_E_DIM, "references dimension 2 but the input has only 1"),
            (lambda: call(cos, X=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(cos, G=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(cos, S=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(cos, A=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(cos, dX=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(cos, dX=p), nat.FR_E_ARG, "must not alias"),
            (lambda: call(cos, A=C.c_void_p(12288)), nat.FR_E_ARG, "distinct buffers"),
            (lambda: call(steep, K=1, rp=rows[1:2]), nat.FR_E_LIMIT, "exponents <= 8 and words of <= 16 letters"),
            (lambda: call(long_word, K=1, rp=rows[1:2]), nat.FR_E_LIMIT, "exponents <= 8 and words of <= 16 letters"),
            (lambda: call(cos, T=1024 * 65536), nat.FR_E_LIMIT, "grid too large"),
            (lambda: call(cos, N=1 << 31), nat.FR_E_LIMIT, "grid too large"),
            (lambda: call(ffn, K=1, rp=rows[1:2]), nat.FR_E_ARG, "per-unit input stride (ffn)"),
            (lambda: call(ragged, K=1, rp=rows[1:2]), nat.FR_E_ARG, "fr_plan_set_grad_lengths"),
            (lambda: call(cos, rp=np.array([0, 2, 1], dtype=np.int32)), nat.FR_E_ARG, "row 1 of the gradient names row 2 of 2"),
            (lambda: call(cos, rp=np.array([-1, 0, 1], dtype=np.int32)), nat.FR_E_ARG, "names row -1 of 2"),
        ]
        for fn, code, text in cases:
            assert fn() == code, (text, nat.last_error())
            assert text in nat.last_error(), (text, nat.last_error())
            assert nat.last_error().startswith("fr_iss_backward: ")
        # a plan of one-letter words needs no d_S
        assert call(one_letter, N=0, S=null, K=1, rp=rows[1:2]) == 0
        # nothing to do: no series, or series of no elements - after the same checks
        assert call(cos, N=0, X=null, G=null, S=null, A=null) == 0
        assert call(cos, T=0) == 0
        assert call(cos, K=0, N=0, rp=None) == 0
        assert call(cos, T=0, rp=np.array([0, 1, 7], dtype=np.int32)) == nat.FR_E_ARG
        assert call(cos, N=0, D=1) == nat.FR_E_DIM
        # the other backward entries still refuse a CosWISS plan, word for word
        assert L.fr_iss_backward_max(cos._h, p, i64(2), i64(2), i64(5), p, p, i64(1), i64(5), i64(5), i64(1),
                                     rows.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(12288),
                                     C.c_void_p(8192), null) == nat.FR_E_ARG
        assert "fr_iss_backward_max: a CosWISS plan has no backward pass" in nat.last_error()
    # ... and fr_iss_backward every plan that is neither
    weighted = nat.Plan([tab([1])], [1], [np.array([1.0], dtype=np.float32)], nat.FR_W_TOTAL)
    assert L.fr_iss_backward(weighted._h, p, i64(2), i64(2), i64(5), p, p, i64(1), i64(5), i64(5), i64(1),
                             rows.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(12288), C.c_void_p(8192),
                             null) == nat.FR_E_ARG
    assert "fr_iss_backward: the plan is not an unweighted Reals trie plan" in nat.last_error()


# ---------------------------------------------------------------- fruits_amd.nn
def test_import_stays_lazy():
    """``import fruits_amd`` still imports no torch; fruits_amd.nn brings the new names."""
    import subprocess
    import sys
    code = ("import sys, fruits_amd\n"
            "assert 'torch' not in sys.modules and 'fruits_amd.nn' not in sys.modules\n"
            "import fruits_amd.nn as m\n"
            "assert callable(m.cos_iss) and 'cos_iss' in m.__all__\n"
            "assert 'CosWISSLayer' in m.__all__ and issubclass(m.CosWISSLayer, m.torch.nn.Module)\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(HERE))


def test_refusals_need_no_device(monkeypatch):
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    words = [fr.words.SimpleWord(w) for w in WORDS]
    freqs = [0.25, 1.5]
    X = torch.zeros((2, 2, 5), dtype=torch.float64)
    # a supported configuration on a host tensor: the input checks of nn.iss, the device last
    for total in (False, True):
        with pytest.raises(TypeError, match="GPU"):
            nn.cos_iss(X, words, freqs, 3, total)
        with pytest.raises(TypeError, match="GPU"):
            nn.CosWISSLayer(words, freqs, exponent=8, total_weighting=total)(X)
        with pytest.raises(TypeError, match="GPU"):
            nn.cos_iss(X, fr.CosWISS(words, freqs, total_weighting=total))
    with pytest.raises(TypeError, match="float64"):
        nn.cos_iss(X.float(), words, freqs)
    with pytest.raises(TypeError, match=r"\(N, D, T\)"):
        nn.cos_iss(X[0], words, freqs)
    with pytest.raises(TypeError, match="torch.Tensor"):
        nn.cos_iss(X.numpy(), words, freqs)
    with pytest.raises(IndexError, match="references dimension 2 but the input has only 1"):
        nn.cos_iss(X[:, :1], words, freqs)
    with pytest.raises(TypeError, match="freqs"):
        nn.cos_iss(X, words)
    with pytest.raises(TypeError, match="CosWISS"):
        nn.cos_iss(X, fr.ISS(words))
    # the randomised variants
    for make in (lambda **kw: nn.cos_iss(X, words, freqs, **kw),
                 lambda **kw: nn.cos_iss(X, fr.CosWISS(words, freqs, **kw)),
                 lambda **kw: nn.CosWISSLayer(words, freqs, **kw),
                 lambda **kw: nn.CosWISSLayer(fr.CosWISS(words, freqs, **kw))):
        with pytest.raises(NotImplementedError, match="ffn_size"):
            make(ffn_size=4)
        with pytest.raises(NotImplementedError, match="dropout"):
            make(dropout=0.25)
    # what the factorised kernels do not cover
    with pytest.raises(NotImplementedError, match=r"exponents 1 \.\.\. 8"):
        nn.cos_iss(X, words, freqs, exponent=9)
    with pytest.raises(NotImplementedError, match="at most 16 letters"):
        nn.CosWISSLayer([fr.words.SimpleWord("[1]" * 17)], freqs)
    monkeypatch.setenv("FRUITS_AMD_COSWISS_TERMS", "1")
    with pytest.raises(NotImplementedError, match="FRUITS_AMD_COSWISS_TERMS=1"):
        nn.cos_iss(X, words, freqs)
    monkeypatch.delenv("FRUITS_AMD_COSWISS_TERMS")
    # per-series lengths: the angle is a function of T
    with pytest.raises(NotImplementedError, match="function of T"):
        nn.cos_iss(X, words, freqs, lengths=[5, 4])
    with pytest.raises(NotImplementedError, match="forward CosWISS takes no lengths"):
        nn.CosWISSLayer(words, freqs)(X, lengths=[5, 4])
    # the other three entries keep refusing a CosWISS, and say where it went
    cos = fr.CosWISS(words, freqs)
    for entry in (nn.iss, nn.max_iss, nn.weighted_iss):
        with pytest.raises(NotImplementedError, match=r"CosWISS.*nn\.cos_iss"):
            entry(X, cos)
    from fruits_amd.sieving import END
    with pytest.raises(NotImplementedError, match=r"CosWISS.*nn\.cos_iss"):
        nn.iss_features(X, cos, sieves=[END()])
