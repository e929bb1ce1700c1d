"""The backward pass of the max semirings without a GPU: the adjoint recursion against the
definition in exact arithmetic (ties included), the new ABI entry's host-side refusals, and the
refusals of fruits_amd.nn.max_iss / MaxISSLayer - all raised before any device call."""
import os

import numpy as np
import pytest

import iss_grad_max_ref as gm
import iss_grad_ref as gr

HERE = os.path.dirname(os.path.abspath(__file__))
# a single letter, a chain of 3, siblings under one parent, a multi-dimension letter, a negative
# exponent, and all of them at once (rows that are inner nodes, a fan-out)
WORD_SETS = (["[1]"], ["[1][2][1]"], ["[1][1]", "[1][2]"], ["[12][2]"], ["[1][-2]"], ["[11][2]"],
             ["[1]", "[1][2][1]", "[1][1]", "[1][2]", "[12][2]", "[1][-2]"])


def exact_input(semiring, N, D, T, seed):
    """Arctic: integers from [-2, 2]; Bayesian: powers of two from [1/4, 2].  Few values, many
    exact ties; every sum and product is exact."""
    rng = np.random.default_rng([seed, N, D, T])
    if semiring == "Arctic":
        return rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    return 2.0 ** rng.integers(-2, 2, size=(N, D, T)).astype(np.float64)


@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("words", WORD_SETS, ids=lambda w: "+".join(w))
def test_recursion_equals_definition(words, T, mode, semiring):
    N, D = 3, 2
    X = exact_input(semiring, N, D, T, seed=1)
    K = len(gr.output_prefixes(words, mode))
    G = np.random.default_rng([2, T, K]).integers(-3, 4, size=(N, K, T)).astype(np.float64)
    want = gm.grad_max_bruteforce(X, G, words, mode, semiring)
    got = gr.as_fractions(gm.iss_grad_max(X, G, words, mode, semiring))
    assert got.shape == want.shape == (N, D, T)
    assert (got == want).all(), (words, T, mode, semiring)
    if T >= 4:
        assert any(v != 0 for v in want.ravel())
        # the case has exact ties: the tie rule is what is tested
        assert gm.smallest_gap(X, words, mode, semiring) == 0.0
    # the magnitude run: the same heads, |G|, |e| and |values|
    mag = gr.as_fractions(gm.iss_grad_max(X, G, words, mode, semiring, magnitude=True))
    assert all(m >= abs(g) for m, g in zip(mag.ravel(), got.ravel()))
    if all("-" not in w for w in words) and (G >= 0).all():
        assert (mag == got).all()


def test_first_of_equal_maxima_wins():
    """A constant series: every running maximum is reached at t = 0 and never rises again, so
    the whole gradient lands on the first step - of every letter."""
    X = np.ones((1, 2, 5))
    G = np.ones((1, 1, 5))
    for semiring in gm.SEMIRINGS:
        got = gm.iss_grad_max(X, G, ["[1][2]"], "SINGLE", semiring).astype(np.float64)
        want = np.zeros((1, 2, 5))
        want[0, :, 0] = 5.0
        np.testing.assert_array_equal(got, want)
        assert (gr.as_fractions(got) == gm.grad_max_bruteforce(X, G, ["[1][2]"], "SINGLE", semiring)).all()
    # a rising series: every step is a head, each time step keeps its own gradient
    X = np.arange(1.0, 6.0).reshape(1, 1, 5)
    got = gm.iss_grad_max(X, np.ones((1, 1, 5)), ["[1]"], "SINGLE", "Arctic").astype(np.float64)
    np.testing.assert_array_equal(got, np.ones((1, 1, 5)))


def test_smallest_gap():
    X = np.array([[[0.0, 3.0, 2.5, 7.0]]])
    # z = x, S = 0 3 3 7: gaps |3-0|, |2.5-3|, |7-3|
    assert gm.smallest_gap(X, ["[1]"], "SINGLE", "Arctic") == 0.5
    assert gm.smallest_gap(X[:, :, :1], ["[1]"], "SINGLE", "Arctic") == np.inf
    X[0, 0, 2] = 3.0
    assert gm.smallest_gap(X, ["[1]"], "SINGLE", "Arctic") == 0.0


def test_n_ops_grad_max_counts():
    # one letter, one row: L = W = E = V = 1, C = 0
    assert gm.n_ops_grad_max(["[1]"], 10, "SINGLE", "Arctic") == 9 + 0 + 0 + 1
    assert gm.n_ops_grad_max(["[1]"], 10, "SINGLE", "Bayesian") == 9 + 0 + 0 + 1 + (1 + 2) + (1 + 2)
    # [1][2] SINGLE: L = 2, W = 2, E = 1, C = 1, V = 2
    assert gm.n_ops_grad_max(["[1][2]"], 10, "SINGLE", "Arctic") == 18 + 2 + 1 + 1
    assert gm.n_ops_grad_max(["[1][2]"], 10, "SINGLE", "Bayesian") == 18 + 2 + 1 + 1 + 4 + 4
    # a sibling fan-out of three and a row that is an inner node: L = 2, E = 1, C = 3, V = 4
    words = ["[1]", "[1][1]", "[1][2]", "[1][3]"]
    assert gm.n_ops_grad_max(words, 5, "SINGLE", "Arctic") == 8 + 2 * 3 + 3 + 1
    # the Arctic count never exceeds the Reals one of the same words
    for ws in (["[1]"], ["[1][2]"], words):
        assert gm.n_ops_grad_max(ws, 7, "EXTENDED", "Bayesian") <= gr.n_ops_grad(ws, 7, "EXTENDED") + 1


def test_bound_holds_for_float64_and_can_fail():
    """The float64 run of the recursion lies within the derived bound of the long-double one, and
    a relative error of 1e-10 on a positive case lies outside - the bound is no formality."""
    import iss_bounds as ib
    words, T = ["[1][2][3]", "[11][2]", "[12][2][3][1]"], 700
    rng = np.random.default_rng(4)
    X = 0.25 + 0.75 * rng.random((2, 3, T))
    G = rng.random((2, len(gr.output_prefixes(words, "EXTENDED")), T))
    for semiring in gm.SEMIRINGS:
        hp = gm.iss_grad_max(X, G, words, "EXTENDED", semiring)
        A = gm.iss_grad_max(X, G, words, "EXTENDED", semiring, magnitude=True)
        n = gm.n_ops_grad_max(words, T, "EXTENDED", semiring)
        f64 = gm.iss_grad_max(X, G, words, "EXTENDED", semiring, dtype=np.float64)
        ib.check_bound(f64, hp, A, n, f"float64 recursion {semiring}")
        np.testing.assert_array_equal(A, hp)          # positive everything: no cancellation
        assert ib.violates(f64 * (1 + 1e-10), hp, A, n)


# ---------------------------------------------------------------- the C ABI
def test_new_entry_is_exported():
    from fruits_amd import _native as nat
    L = nat.lib()
    assert "fr_iss_backward_max" in nat.EXPORTS and hasattr(L, "fr_iss_backward_max")
    with open(os.path.join(os.path.dirname(HERE), "include", "fruits_hip.h")) as f:
        header = f.read()
    assert header.count("int fr_iss_backward_max(") == 1 and header.count("int fr_iss_backward(") == 1
    assert "fruits/iss/semiring.py:282-309" in header and "fruits/iss/semiring.py:461-493" in header
    assert L.fr_version() >= 139


def test_backward_max_entry_checks_before_any_device_call():
    """fr_iss_backward_max validates the plan, the row map and the pointers on the host."""
    import ctypes as C
    from fruits_amd import _native as nat
    L = nat.lib()
    i64 = C.c_int64
    p = C.c_void_p(4096)        # never dereferenced: every call below fails before a launch
    null = C.c_void_p(0)
    tab = lambda *rows: np.array(rows, dtype=np.int32)
    rows = np.array([1], dtype=np.int32)
    for flag in ("arctic", "bayesian"):
        prefix = nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1], **{flag: True})

        def call(plan=prefix, X=p, N=2, D=2, T=5, S=p, G=p, K=1, sn=5, sk=5, st=1, rp=rows, A=p, dX=None):
            return L.fr_iss_backward_max(plan._h if plan is not None else None, X, i64(N), i64(D), i64(T),
                                         S, G, i64(K), i64(sn), i64(sk), i64(st),
                                         rp.ctypes.data_as(C.POINTER(C.c_int32)) if rp is not None else None,
                                         A, C.c_void_p(8192) if dX is None else dX, null)

        not_prefix = nat.Plan([tab([1, 0], [0, 1])], [1], **{flag: True})   # the inner node emits no row
        weighted = nat.Plan([tab([1])], [1], [np.ones(1, np.float32)], nat.FR_W_NONTOTAL, **{flag: True})
        total = nat.Plan([tab([1])], [1], [np.ones(1, np.float32)], nat.FR_W_TOTAL, **{flag: True})
        reals = nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1])
        letter_sum = nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1], arctic=True, letter_sum=True)
        cos = nat.CosPlan([tab([1])], [0.5], 2, False)
        cases = [
            (lambda: call(plan=None), nat.FR_E_ARG, "null plan"),
            (lambda: call(N=-1), nat.FR_E_ARG, "bad shape"),
            (lambda: call(D=0), nat.FR_E_ARG, "bad shape"),
            (lambda: call(st=-1), nat.FR_E_ARG, "bad shape"),
            (lambda: call(rp=None), nat.FR_E_ARG, "null host table"),
            (lambda: call(D=1), nat.FR_E_DIM, "references dimension 2 but the input has only 1"),
            (lambda: call(X=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(S=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(A=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(G=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(dX=p), nat.FR_E_ARG, "must not alias"),
            (lambda: call(plan=not_prefix), nat.FR_E_ARG, "not a prefix plan"),
            (lambda: call(plan=weighted), nat.FR_E_ARG, "a weighted plan"),
            (lambda: call(plan=total), nat.FR_E_ARG, "a weighted plan"),
            (lambda: call(plan=reals), nat.FR_E_ARG, "a Reals plan - its backward pass is fr_iss_backward"),
            (lambda: call(plan=letter_sum), nat.FR_E_ARG, "a letter-sum plan"),
            (lambda: call(plan=cos, D=1), nat.FR_E_ARG, "a CosWISS plan"),
            (lambda: call(rp=np.array([2], dtype=np.int32)), nat.FR_E_ARG, "names prefix 2 of 2"),
            (lambda: call(rp=np.array([-1], dtype=np.int32)), nat.FR_E_ARG, "names prefix -1 of 2"),
        ]
        for fn, code, text in cases:
            assert fn() == code, (flag, text, nat.last_error())
            assert text in nat.last_error(), (flag, text, nat.last_error())
            assert nat.last_error().startswith("fr_iss_backward_max: ")
        # nothing to do: no series, or series of no elements - after the same checks
        assert call(N=0, X=null, S=null, G=null, A=null) == 0
        assert call(T=0) == 0
        # the Reals entry still refuses these plans, in its own words
        assert L.fr_iss_backward(prefix._h, p, i64(2), i64(2), i64(5), p, p, i64(1), i64(5), i64(5), i64(1),
                                 rows.ctypes.data_as(C.POINTER(C.c_int32)), p, C.c_void_p(8192),
                                 null) == nat.FR_E_ARG
        assert "fr_iss_backward: the plan is not an unweighted Reals trie plan" in nat.last_error()


# ---------------------------------------------------------------- fruits_amd.nn
def test_import_stays_lazy():
    import subprocess
    import sys
    code = ("import sys, fruits_amd\n"
            "assert 'torch' not in sys.modules and 'fruits_amd.nn' not in sys.modules\n"
            "import fruits_amd.nn as m\n"
            "assert callable(m.max_iss) and issubclass(m.MaxISSLayer, sys.modules['torch'].nn.Module)\n"
            "assert {'max_iss', 'MaxISSLayer', 'iss', 'ISSLayer'} <= set(m.__all__)\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(HERE))


def test_refusals_need_no_device():
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    from fruits_amd.iss.weighting import Indices
    Arctic, Bayesian, Reals = fr.semiring.Arctic, fr.semiring.Bayesian, fr.semiring.Reals
    words = [fr.words.SimpleWord("[1][2]")]
    X = torch.zeros((2, 2, 5), dtype=torch.float64)
    for sr in (Arctic, Bayesian):
        with pytest.raises(TypeError, match="GPU"):
            nn.max_iss(X, words, semiring=sr())
        with pytest.raises(TypeError, match="GPU"):
            nn.MaxISSLayer(words, fr.ISSMode.EXTENDED, semiring=sr())(X)
        with pytest.raises(TypeError, match="GPU"):
            nn.max_iss(X, fr.ISS(words, semiring=sr()))
        with pytest.raises(TypeError, match="float64"):
            nn.max_iss(X.float(), words, semiring=sr())
        with pytest.raises(TypeError, match=r"\(N, D, T\)"):
            nn.max_iss(X[0], words, semiring=sr())
        with pytest.raises(TypeError, match="torch.Tensor"):
            nn.max_iss(X.numpy(), words, semiring=sr())
        with pytest.raises(IndexError, match="references dimension 2 but the input has only 1"):
            nn.max_iss(X[:, :1], words, semiring=sr())
        with pytest.raises(IndexError, match="references dimension 2"):
            nn.MaxISSLayer(words, semiring=sr())(X[:, :1])
        weighted = fr.ISS(words, semiring=sr(), weighting=Indices())
        with pytest.raises(NotImplementedError, match="weighting"):
            nn.max_iss(X, weighted)
        with pytest.raises(NotImplementedError, match="weighting"):
            nn.MaxISSLayer(weighted)
        generic = fr.words.Word("[DIM(1)][ABS(2)]")
        with pytest.raises(NotImplementedError, match="generic"):
            nn.max_iss(X, [words[0], generic], semiring=sr())
        with pytest.raises(NotImplementedError, match="generic"):
            nn.MaxISSLayer([generic], semiring=sr())
    # Reals: pointed to nn.iss
    with pytest.raises(NotImplementedError, match=r"nn\.iss"):
        nn.max_iss(X, words, semiring=Reals())
    with pytest.raises(NotImplementedError, match=r"nn\.iss"):
        nn.MaxISSLayer(fr.ISS(words))
    with pytest.raises(TypeError, match="semiring="):
        nn.max_iss(X, words)
    with pytest.raises(TypeError, match="semiring="):
        nn.MaxISSLayer(words)
    with pytest.raises(TypeError, match="carries Arctic, not Bayesian"):
        nn.max_iss(X, fr.ISS(words, semiring=Arctic()), semiring=Bayesian())
    with pytest.raises(NotImplementedError, match="argmax"):
        nn.max_iss(X, words, fr.ISSMode.EXTENDED, semiring=Arctic(argmax=True))
    with pytest.raises(NotImplementedError, match="argmax"):
        nn.MaxISSLayer(words, fr.ISSMode.EXTENDED, semiring=Arctic(argmax=True))
    cos = fr.CosWISS(words, freqs=[0.5])
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.max_iss(X, cos)
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.MaxISSLayer(cos)
    # the Reals names keep their refusals
    with pytest.raises(NotImplementedError, match="semiring"):
        nn.iss(X, words, semiring=Arctic())


def test_layer_is_a_plain_module():
    """No parameters; copies and pickles without its device programs."""
    import copy
    import pickle
    import fruits_amd as fr
    from fruits_amd import nn
    words = fr.words.of_weight(2, dim=2)
    for sr in (fr.semiring.Arctic, fr.semiring.Bayesian):
        layer = nn.MaxISSLayer(words, fr.ISSMode.EXTENDED, semiring=sr())
        assert list(layer.parameters()) == [] and list(layer.buffers()) == []
        assert sr.__name__ in repr(layer)
        for dup in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
            assert isinstance(dup, nn.MaxISSLayer) and dup.mode == fr.ISSMode.EXTENDED
            assert type(dup.semiring) is sr
            assert [str(w) for w in dup.words] == [str(w) for w in words]
            assert dup.op._plans == {}
