"""The backward pass of the Reals iterated sums without a GPU: the long-double oracle of the
adjoint recursion against the definition in exact arithmetic, the new ABI entry, and the
refusals of fruits_amd.nn - all raised before any device call."""
import os

import numpy as np
import pytest

import iss_grad_ref as gr

HERE = os.path.dirname(os.path.abspath(__file__))
WORD_SETS = (["[1]"], ["[1][2]"], ["[11][2]"], ["[1][-2]"], ["[12][2][1]"],
             ["[1]", "[1][2]", "[11][2]", "[1][-2]", "[12][2][1]"])


def exact_input(word_strings, N, D, T, seed):
    """Integer-valued X from {-2 ... 2}, from {+-0.5, +-1, +-2} in the dimensions some word
    divides by (zeros wherever every exponent is positive)."""
    rng = np.random.default_rng([seed, N, D, T])
    X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    divided = {d for s in word_strings for row in gr.orc.parse_word(s)
               for d, e in enumerate(row) if e < 0}
    for d in divided:
        X[:, d] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=(N, T))
    return X


@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("T", [1, 2, 5, 7])
@pytest.mark.parametrize("words", WORD_SETS, ids=lambda w: "+".join(w))
def test_oracle_equals_definition(words, T, mode):
    N, D = 2, 2
    X = exact_input(words, N, D, T, seed=1)
    K = len(gr.output_prefixes(words, mode))
    G = np.random.default_rng([2, T, K]).integers(-3, 4, size=(N, K, T)).astype(np.float64)
    want = gr.grad_bruteforce(X, G, words, mode)
    got = gr.as_fractions(gr.iss_grad(X, G, words, mode))
    assert got.shape == want.shape == (N, D, T)
    assert (got == want).all(), (words, T, mode)
    if T >= 5:
        assert any(v != 0 for v in want.ravel())
    # the magnitude run is the same recursion on |X|, |G|, |e|: the definition on those, with
    # the sign of a negative exponent's coefficient dropped
    if all("-" not in w for w in words):
        mag = gr.as_fractions(gr.iss_grad(X, G, words, mode, magnitude=True))
        assert (mag == gr.grad_bruteforce(np.abs(X), np.abs(G), words, mode)).all()


def test_zero_input_has_a_finite_gradient():
    """x = 0 under a positive exponent: x^(e-1) by multiplication, never m / x."""
    X = np.zeros((1, 2, 4))
    X[0, 1] = [1.0, 2.0, 0.0, 1.0]
    G = np.ones((1, 1, 4))
    for words in (["[1][2]"], ["[11][2]"], ["[12]"]):
        got = gr.iss_grad(X, G, words)
        assert np.isfinite(got).all()
        assert (gr.as_fractions(got) == gr.grad_bruteforce(X, G, words)).all()


def test_n_ops_grad_counts():
    # one letter, one row: L = W = E = V = 1, C = 0
    assert gr.n_ops_grad(["[1]"], 10) == 9 + 1 + 2 + 1 + 2 + 0 + 0
    # [1][2] SINGLE: L = 2, W = 2, E = 1, C = 1, V = 2
    assert gr.n_ops_grad(["[1][2]"], 10) == 18 + 2 + 2 + 2 + 2 + 2 + 1
    # a sibling fan-out of three and a row that is an inner node
    words = ["[1]", "[1][1]", "[1][2]", "[1][3]"]
    assert gr.n_ops_grad(words, 5, "SINGLE") == 8 + 2 + 2 + 2 + 2 + 2 * 3 + 3
    assert gr.n_ops_grad(["[1]", "[1]"], 3) == 2 + 1 + 2 + 1 + 2 + 1 + 0      # E = 2


def test_bound_holds_for_float64_and_can_fail():
    """The float64 run of the recursion lies within the derived bound of the long-double one; on
    positive inputs (no cancellation: the magnitude run is the value) a relative error of 1e-10
    lies outside - the bound is no formality."""
    import iss_bounds as ib
    words, T = ib.WORDS, 700
    rng = np.random.default_rng(4)
    X = rng.random((2, 3, T)) + 0.25
    G = rng.random((2, len(gr.output_prefixes(words, "EXTENDED")), T))
    hp = gr.iss_grad(X, G, words, "EXTENDED")
    A = gr.iss_grad(X, G, words, "EXTENDED", magnitude=True)
    n = gr.n_ops_grad(words, T, "EXTENDED")
    f64 = gr.iss_grad(X, G, words, "EXTENDED", dtype=np.float64)
    ib.check_bound(f64, hp, A, n, "float64 recursion")
    # the only negative terms are those of the division's derivative: A is |hp| but for them
    assert ib.violates(f64 * (1 + 1e-10), hp, A, n)


def test_new_entry_is_exported():
    from fruits_amd import _native as nat
    L = nat.lib()
    assert "fr_iss_backward" in nat.EXPORTS and hasattr(L, "fr_iss_backward")
    with open(os.path.join(os.path.dirname(HERE), "include", "fruits_hip.h")) as f:
        header = f.read()
    assert header.count("int fr_iss_backward(") == 1
    assert "fruits/iss/semiring.py:98-125" in header
    assert L.fr_version() >= 138


def test_backward_entry_checks_before_any_device_call():
    """fr_iss_backward validates the plan, the row map and the pointers on the host."""
    import ctypes as C
    from fruits_amd import _native as nat
    L = nat.lib()
    i64 = C.c_int64
    p = C.c_void_p(4096)        # never dereferenced: every call below fails before a launch
    null = C.c_void_p(0)
    tab = lambda *rows: np.array(rows, dtype=np.int32)
    prefix = nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1])
    rows = np.array([1], dtype=np.int32)

    def call(plan=prefix, X=p, N=2, D=2, T=5, S=p, G=p, K=1, sn=5, sk=5, st=1, rp=rows, A=p, dX=None):
        return L.fr_iss_backward(plan._h if plan is not None else None, X, i64(N), i64(D), i64(T), S, G,
                                 i64(K), i64(sn), i64(sk), i64(st),
                                 rp.ctypes.data_as(C.POINTER(C.c_int32)) if rp is not None else None,
                                 A, C.c_void_p(8192) if dX is None else dX, null)

    not_prefix = nat.Plan([tab([1, 0], [0, 1])], [1])           # the inner node emits no row
    weighted = nat.Plan([tab([1])], [1], [np.ones(1, np.float32)], nat.FR_W_NONTOTAL)
    arctic = nat.Plan([tab([1])], [1], arctic=True)
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
        (lambda: call(plan=weighted), nat.FR_E_ARG, "not an unweighted Reals trie plan"),
        (lambda: call(plan=arctic), nat.FR_E_ARG, "not an unweighted Reals trie plan"),
        (lambda: call(rp=np.array([2], dtype=np.int32)), nat.FR_E_ARG, "names prefix 2 of 2"),
        (lambda: call(rp=np.array([-1], dtype=np.int32)), nat.FR_E_ARG, "names prefix -1 of 2"),
    ]
    for fn, code, text in cases:
        assert fn() == code, text
        assert text in nat.last_error(), (text, nat.last_error())
    # nothing to do: no series, or series of no elements - after the same checks
    assert call(N=0, X=null, S=null, G=null, A=null) == 0
    assert call(T=0) == 0


# ---------------------------------------------------------------- fruits_amd.nn
def test_nn_is_loaded_lazily():
    import subprocess
    import sys
    code = ("import sys, fruits_amd\n"
            "assert 'fruits_amd.nn' not in sys.modules and 'torch.nn' not in sys.modules\n"
            "import fruits_amd.nn as m\n"
            "assert fruits_amd.nn is m and callable(m.iss) and 'torch.nn' in sys.modules\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(HERE))


def test_refusals_need_no_device():
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    from fruits_amd.iss.weighting import Indices
    words = [fr.words.SimpleWord("[1][2]")]
    X = torch.zeros((2, 2, 5), dtype=torch.float64)
    with pytest.raises(TypeError, match="GPU"):
        nn.iss(X, words)
    with pytest.raises(TypeError, match="GPU"):
        nn.ISSLayer(words, fr.ISSMode.EXTENDED)(X)
    with pytest.raises(TypeError, match="float64"):
        nn.iss(X.float(), words)
    with pytest.raises(TypeError, match=r"\(N, D, T\)"):
        nn.iss(X[0], words)
    with pytest.raises(TypeError, match="torch.Tensor"):
        nn.iss(X.numpy(), words)
    with pytest.raises(IndexError, match="references dimension 2 but the input has only 1"):
        nn.iss(X[:, :1], words)
    with pytest.raises(IndexError, match="references dimension 2"):
        nn.ISSLayer(words)(X[:, :1])
    with pytest.raises(NotImplementedError, match="weighting"):
        nn.iss(X, words, weighting=Indices())
    with pytest.raises(NotImplementedError, match="weighting"):
        nn.ISSLayer(words, weighting=Indices())
    for semiring in (fr.semiring.Arctic(), fr.semiring.Bayesian()):
        with pytest.raises(NotImplementedError, match="semiring"):
            nn.iss(X, words, semiring=semiring)
        with pytest.raises(NotImplementedError, match="semiring"):
            nn.ISSLayer(words, semiring=semiring)
    generic = fr.words.Word("[DIM(1)][ABS(2)]")
    with pytest.raises(NotImplementedError, match="generic"):
        nn.iss(X, [words[0], generic])
    with pytest.raises(NotImplementedError, match="generic"):
        nn.ISSLayer([generic])
    cos = fr.CosWISS(words, freqs=[0.5])
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.iss(X, cos)
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.ISSLayer(cos)


def test_layer_is_a_plain_module():
    """No parameters; copies and pickles without its device programs."""
    import copy
    import pickle
    import fruits_amd as fr
    from fruits_amd import nn
    words = fr.words.of_weight(2, dim=2)
    layer = nn.ISSLayer(words, fr.ISSMode.EXTENDED)
    assert list(layer.parameters()) == [] and list(layer.buffers()) == []
    for dup in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
        assert isinstance(dup, nn.ISSLayer) and dup.mode == fr.ISSMode.EXTENDED
        assert [str(w) for w in dup.words] == [str(w) for w in words]
        assert dup.op._plans == {}
