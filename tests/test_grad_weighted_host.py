"""The backward pass of the weighted Reals iterated sums without a GPU: the long-double oracle of
the adjoint recursion against the definition in exact arithmetic, against the unweighted oracle at
alpha = 0, the new ABI entry, and the refusals of fruits_amd.nn.weighted_iss - all raised before
any device call."""
import os

import numpy as np
import pytest

import iss_grad_ref as gr
import iss_grad_weighted_ref as gw

HERE = os.path.dirname(os.path.abspath(__file__))

# (words, alphas): a word that is a proper prefix of another with DIFFERENT alphas (two nodes
# [1] of depth 1); a node that is an output row and a parent ([1][2] with the alphas (1, 2) in
# the last set, [1] in the second); equal words with other alphas; a squared letter, a division
WORD_SETS = {
    "one_letter": (["[1]"], [[1.0]]),
    "two_letters": (["[1][2]"], [[1.0, 2.0]]),
    "prefix_other_alpha": (["[1]", "[1][2]"], [[1.0], [2.0, 1.0]]),
    "row_and_parent": (["[1]", "[1][2]", "[1][1]"], [[2.0], [2.0, 1.0], [2.0, 2.0]]),
    "twins": (["[1][2]", "[1][2]", "[11][2]"], [[1.0, 1.0], [2.0, 1.0], [1.0, 2.0]]),
    "three_letters": (["[1][2]", "[1][2][1]", "[12][2][1]", "[1][-2]"],
                      [[1.0, 2.0], [1.0, 2.0, 1.0], [2.0, 1.0, 1.0], [1.0, 1.0]]),
}


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


def power_tables(T, seed):
    """Exp tables of exact powers of two, E+_a[t] = 2^(a j(t)) and E-_a[t] = 2^(-a j(t)) with a
    non-decreasing integer j - a lookup 'g = j ln 2' - for the alphas 1 and 2: every product and
    sum of the recursion is a dyadic rational of few bits, exact in any float format."""
    j = np.cumsum(np.random.default_rng([seed, T]).integers(0, 2, size=T)).astype(np.float64)
    return ({a: 2.0 ** (a * j) for a in (1.0, 2.0)}, {a: 2.0 ** (-a * j) for a in (1.0, 2.0)})


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("name", list(WORD_SETS))
def test_oracle_equals_definition(name, T, mode, total):
    words, alphas = WORD_SETS[name]
    N, D = 2, 2
    X = exact_input(words, N, D, T, seed=1)
    K = len(gw.output_nodes(words, alphas, mode))
    G = np.random.default_rng([2, T, K]).integers(-3, 4, size=(N, K, T)).astype(np.float64)
    Ep, Em = power_tables(T, seed=3)
    want = gw.grad_weighted_bruteforce(X, G, words, alphas, Ep, Em, total, mode)
    got = gr.as_fractions(gw.iss_grad_weighted(X, G, words, alphas, None, total, mode, tables=(Ep, Em)))
    assert got.shape == want.shape == (N, D, T)
    assert (got == want).all(), (name, T, mode, total)
    if T >= 5:
        assert any(v != 0 for v in want.ravel())
    if T == 6 and len(words) > 1:
        # the weights matter: with the tables swapped, another gradient
        assert (gw.grad_weighted_bruteforce(X, G, words, alphas, Em, Ep, total, mode) != want).any()
    # the magnitude run: the definition on |X|, |G| (no division: its coefficient keeps a sign)
    if all("-" not in w for w in words):
        mag = gr.as_fractions(gw.iss_grad_weighted(X, G, words, alphas, None, total, mode,
                                                   magnitude=True, tables=(Ep, Em)))
        assert (mag == gw.grad_weighted_bruteforce(np.abs(X), np.abs(G), words, alphas, Ep, Em,
                                                   total, mode)).all()


def test_the_trie_is_keyed_by_letters_and_alphas():
    words, alphas = WORD_SETS["prefix_other_alpha"]
    # [1] with alpha 1 is a row; [1] with alpha 2 is the inner node of [1][2]: two nodes
    rows = gw.output_nodes(words, alphas, "EXTENDED")
    one, two = (1,), (0, 1)
    assert rows == [((one, 1.0),), ((one, 2.0), (two, 1.0))]
    assert len(gw.trie_nodes(rows)) == 3
    words, alphas = WORD_SETS["row_and_parent"]
    rows = gw.output_nodes(words, alphas, "SINGLE")
    nodes = gw.trie_nodes(rows)
    assert len(nodes) == 3 and rows[0] == nodes[0] and all(r[:1] == nodes[0] for r in rows[1:])


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
def test_alpha_zero_is_the_unweighted_recursion(mode, total):
    """exp(+-g * 0) = 1.0 exactly: the weighted recursion is that of iss_grad_ref, bit for bit."""
    words = ["[1]", "[1][2]", "[1][2][1]", "[2]", "[1][2]", "[11][2]", "[1][-2]"]
    alphas = [np.zeros(len(gr.orc.parse_word(w)), dtype=np.float32) for w in words]
    N, D, T = 3, 2, 40
    X = exact_input(words, N, D, T, seed=5)
    K = len(gr.output_prefixes(words, mode))
    G = np.random.default_rng(6).integers(-3, 4, size=(N, K, T)).astype(np.float64)
    lookup = np.linspace(0.0, 50.0, T)[None, :]
    got = gw.iss_grad_weighted(X, G, words, alphas, lookup, total, mode)
    want = gr.iss_grad(X, G, words, mode)
    assert np.array_equal(got, want) and np.abs(want).max() > 0


def test_recursion_is_the_gradient_of_the_forward_oracle():
    """A central difference of the weighted forward oracle (oracle/ref_numpy.py) agrees with the
    recursion: the two bodies are tied to the reference's code, not only to the definition."""
    words = ["[1][2]", "[11][2][1]", "[2]"]
    alphas = [np.array(a, dtype=np.float32) for a in ([0.5, 1.5], [1.25, 0.25, 2.0], [0.75])]
    N, D, T = 2, 2, 7
    rng = np.random.default_rng(8)
    X = rng.standard_normal((N, D, T))
    lookup = np.broadcast_to(gr.orc.lookup_indices(1, T, scale=2.0), (N, T))
    for mode in ("SINGLE", "EXTENDED"):
        for total in (False, True):
            K = len(gw.output_nodes(words, alphas, mode))
            G = rng.standard_normal((N, K, T))

            def loss(Z):
                Y = gr.orc.iss_transform(Z, words, mode, alphas, lookup, total, dtype=gr.HP)
                return float((Y.transpose(1, 0, 2) * G).sum())

            got = gw.iss_grad_weighted(X, G, words, alphas, lookup, total, mode).astype(np.float64)
            h = 1e-6
            for at in [(0, 0, 0), (1, 1, 3), (0, 1, 6), (1, 0, 5)]:
                Zp, Zm = X.copy(), X.copy()
                Zp[at] += h
                Zm[at] -= h
                fd = (loss(Zp) - loss(Zm)) / (2 * h)
                assert abs(fd - got[at]) <= 1e-7 * max(1.0, abs(got[at])), (mode, total, at, fd, got[at])


def test_n_ops_grad_weighted_counts():
    lookup = np.array([[0.0, 1.5]])
    # one letter, alpha 1: n_ops_grad = 9 + 1 + 2 + 1 + 2 + 0 + 0, then 4 (3 + 2) + 1
    assert gr.n_ops_grad(["[1]"], 10) == 15
    assert gw.n_ops_grad_weighted(["[1]"], [[1.0]], lookup, 10) == 15 + 4 * (3 + 2) + 1
    # alpha_max g_max = 2 * 1.5 = 3: 4 L (3 + 3) + L with L = 2
    assert gw.n_ops_grad_weighted(["[1][2]"], [[1.0, 2.0]], lookup, 10) == \
        gr.n_ops_grad(["[1][2]"], 10) + 8 * 6 + 2
    # equal letters, other alphas: two nodes where the unweighted trie has one (V: 2 -> 3, E: 2 -> 1)
    words, alphas = ["[1][2]", "[1][2]"], [[1.0, 1.0], [1.0, 2.0]]
    assert gr.n_ops_grad(words, 5) == 8 + 2 + 2 + 2 + 2 + 2 * 2 + 1
    assert gw.n_ops_grad_weighted(words, alphas, lookup, 5) == (8 + 2 + 2 + 2 + 2 + 2 * 2 + 2) + 8 * 6 + 2
    # with equal alphas throughout the trie is the unweighted one
    assert gw.n_ops_grad_weighted(words, [[1.0, 1.0]] * 2, lookup, 5) == gr.n_ops_grad(words, 5) + 8 * 5 + 2


def test_bound_holds_for_float64_and_can_fail():
    """The float64 run of the recursion lies within the derived bound of the long-double one; a
    relative error of 1e-10 on positive inputs, or a dropped exp factor, lies outside."""
    import iss_bounds as ib
    words, T = ib.WORDS, 700
    rng = np.random.default_rng(4)
    alphas = [rng.uniform(0.25, 2.0, len(gr.orc.parse_word(w))).astype(np.float32) for w in words]
    X = rng.random((2, 3, T)) + 0.25
    lookup = gr.orc.lookup_indices(1, T, scale=5.0)
    K = len(gw.output_nodes(words, alphas, "EXTENDED"))
    G = rng.random((2, K, T))
    n = gw.n_ops_grad_weighted(words, alphas, lookup, T, "EXTENDED")
    for total in (False, True):
        hp = gw.iss_grad_weighted(X, G, words, alphas, lookup, total, "EXTENDED")
        A = gw.iss_grad_weighted(X, G, words, alphas, lookup, total, "EXTENDED", magnitude=True)
        f64 = gw.iss_grad_weighted(X, G, words, alphas, lookup, total, "EXTENDED", dtype=np.float64)
        ib.check_bound(f64, hp, A, n, f"float64 recursion total={total}")
        assert ib.violates(f64 * (1 + 1e-10), hp, A, n)
        # the other body's gradient is far outside: a misplaced factor does not hide in the bound
        assert ib.violates(gw.iss_grad_weighted(X, G, words, alphas, lookup, not total, "EXTENDED",
                                                dtype=np.float64), hp, A, n)


# ---------------------------------------------------------------- the ABI entry
def test_new_entry_is_exported():
    from fruits_amd import _native as nat
    L = nat.lib()
    assert "fr_iss_backward_weighted" in nat.EXPORTS and hasattr(L, "fr_iss_backward_weighted")
    with open(os.path.join(os.path.dirname(HERE), "include", "fruits_hip.h")) as f:
        header = f.read()
    assert header.count("int fr_iss_backward_weighted(") == 1
    assert header.count("int fr_iss_backward(") == 1 and header.count("int fr_iss_backward_max(") == 1
    assert "fruits/iss/semiring.py:98-158" in header
    assert L.fr_version() >= 140


def test_weighted_entry_checks_before_any_device_call():
    """fr_iss_backward_weighted validates the plan, the row map and the pointers on the host."""
    import ctypes as C
    from fruits_amd import _native as nat
    L = nat.lib()
    i64 = C.c_int64
    p = C.c_void_p(4096)        # never dereferenced: every call below fails before a launch
    null = C.c_void_p(0)
    tab = lambda *rows: np.array(rows, dtype=np.int32)
    f32 = lambda *v: np.array(v, dtype=np.float32)
    plans = {w: nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1], [f32(1.0), f32(1.0, 0.5)], w)
             for w in (nat.FR_W_NONTOTAL, nat.FR_W_TOTAL)}
    rows = np.array([1], dtype=np.int32)

    def call(plan, X=p, N=2, D=2, T=5, lk=p, lr=1, G=p, K=1, sn=5, sk=5, st=1, rp=rows,
             Cs=C.c_void_p(12288), A=C.c_void_p(16384), aux=C.c_void_p(20480), dX=None):
        return L.fr_iss_backward_weighted(
            plan._h if plan is not None else None, X, i64(N), i64(D), i64(T), lk, i64(lr), G, i64(K),
            i64(sn), i64(sk), i64(st),
            rp.ctypes.data_as(C.POINTER(C.c_int32)) if rp is not None else None,
            Cs, A, aux, C.c_void_p(8192) if dX is None else dX, null)

    for wmode, prefix in plans.items():
        assert prefix.nodes == 2 and prefix.info(nat.FR_INFO_ALPHAS) == 2
        not_prefix = nat.Plan([tab([1, 0], [0, 1])], [1], [f32(1.0, 0.5)], wmode)
        unweighted = nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1])
        arctic = nat.Plan([tab([1])], [1], [f32(1.0)], wmode, arctic=True)
        bayesian = nat.Plan([tab([1])], [1], [f32(1.0)], wmode, bayesian=True)
        cos = nat.CosPlan([tab([1])], [0.5], 1, False)
        cases = [
            (lambda: call(None), nat.FR_E_ARG, "null plan"),
            (lambda: call(prefix, N=-1), nat.FR_E_ARG, "bad shape"),
            (lambda: call(prefix, D=0), nat.FR_E_ARG, "bad shape"),
            (lambda: call(prefix, sk=-1), nat.FR_E_ARG, "bad shape"),
            (lambda: call(prefix, lr=3), nat.FR_E_ARG, "1 or N rows, not 3"),
            (lambda: call(prefix, rp=None), nat.FR_E_ARG, "null host table"),
            (lambda: call(prefix, D=1), nat.FR_E_DIM, "references dimension 2 but the input has only 1"),
            (lambda: call(prefix, X=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, lk=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, Cs=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, A=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, aux=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, G=null), nat.FR_E_ARG, "null device pointer"),
            (lambda: call(prefix, dX=p), nat.FR_E_ARG, "must not alias"),
            (lambda: call(prefix, A=C.c_void_p(12288)), nat.FR_E_ARG, "distinct buffers"),
            (lambda: call(not_prefix), nat.FR_E_ARG, "not a prefix plan"),
            (lambda: call(unweighted), nat.FR_E_ARG, "an unweighted Reals plan - its backward pass is fr_iss_backward"),
            (lambda: call(arctic), nat.FR_E_ARG, "fr_iss_backward_max differentiates the unweighted ones"),
            (lambda: call(bayesian), nat.FR_E_ARG, "fr_iss_backward_max differentiates the unweighted ones"),
            (lambda: call(cos), nat.FR_E_ARG, "a CosWISS plan has no backward pass"),
            (lambda: call(prefix, rp=np.array([2], dtype=np.int32)), nat.FR_E_ARG, "names prefix 2 of 2"),
            (lambda: call(prefix, rp=np.array([-1], dtype=np.int32)), nat.FR_E_ARG, "names prefix -1 of 2"),
        ]
        for fn, code, text in cases:
            assert fn() == code, text
            assert text in nat.last_error(), (text, nat.last_error())
            assert nat.last_error().startswith("fr_iss_backward_weighted: ")
        # nothing to do: no series, or series of no elements - after the same checks
        assert call(prefix, N=0, lr=0, X=null, lk=null, G=null, Cs=null, A=null, aux=null) == 0
        assert call(prefix, N=0, X=null, lk=null, G=null, Cs=null, A=null, aux=null) == 0
        assert call(prefix, T=0) == 0
        assert call(prefix, T=0, rp=np.array([7], dtype=np.int32)) == nat.FR_E_ARG
        # the old entries still refuse a weighted plan, with their own messages
        assert L.fr_iss_backward(prefix._h, p, i64(2), i64(2), i64(5), p, p, i64(1), i64(5), i64(5), i64(1),
                                 rows.ctypes.data_as(C.POINTER(C.c_int32)), p, C.c_void_p(8192), null) == nat.FR_E_ARG
        assert "fr_iss_backward: the plan is not an unweighted Reals trie plan" in nat.last_error()


# ---------------------------------------------------------------- fruits_amd.nn
def test_import_stays_lazy():
    """``import fruits_amd`` still imports no torch; fruits_amd.nn brings the new names."""
    import subprocess
    import sys
    code = ("import sys, fruits_amd\n"
            "assert 'torch' not in sys.modules and 'fruits_amd.nn' not in sys.modules\n"
            "import fruits_amd.nn as m\n"
            "assert callable(m.weighted_iss) and 'weighted_iss' in m.__all__\n"
            "assert 'WeightedISSLayer' in m.__all__ and 'torch.nn' in sys.modules\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(HERE))


def test_refusals_need_no_device():
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    from fruits_amd.iss.weighting import L1, L2, Custom, Indices, Plateaus
    words = [fr.words.SimpleWord("[1][2]")]
    X = torch.zeros((2, 2, 5), dtype=torch.float64)
    for w in (Indices(), Indices(total=True), Plateaus(3), Plateaus(3, total=True)):
        # a supported configuration on a host tensor: the input checks of nn.iss, the device last
        with pytest.raises(TypeError, match="GPU"):
            nn.weighted_iss(X, words, weighting=w)
        with pytest.raises(TypeError, match="GPU"):
            nn.WeightedISSLayer(words, fr.ISSMode.EXTENDED, weighting=w)(X)
        with pytest.raises(TypeError, match="GPU"):
            nn.weighted_iss(X, fr.ISS(words, weighting=w))
        with pytest.raises(TypeError, match="float64"):
            nn.weighted_iss(X.float(), words, weighting=w)
        with pytest.raises(TypeError, match=r"\(N, D, T\)"):
            nn.weighted_iss(X[0], words, weighting=w)
        with pytest.raises(TypeError, match="torch.Tensor"):
            nn.weighted_iss(X.numpy(), words, weighting=w)
        with pytest.raises(IndexError, match="references dimension 2 but the input has only 1"):
            nn.weighted_iss(X[:, :1], words, weighting=w)
        with pytest.raises(IndexError, match="references dimension 2"):
            nn.WeightedISSLayer(words, weighting=w)(X[:, :1])
    # no weighting: the unweighted functions
    with pytest.raises(NotImplementedError, match=r"nn\.iss"):
        nn.weighted_iss(X, words)
    with pytest.raises(NotImplementedError, match=r"nn\.iss"):
        nn.WeightedISSLayer(words, weighting=None)
    with pytest.raises(NotImplementedError, match=r"nn\.iss"):
        nn.weighted_iss(X, fr.ISS(words))
    # a lookup that is a function of the input
    for w in (L1(), L2(total=True), Custom(lambda Z: Z[:, 0, :])):
        with pytest.raises(NotImplementedError, match="depends on the input"):
            nn.weighted_iss(X, words, weighting=w)
        with pytest.raises(NotImplementedError, match="depends on the input"):
            nn.WeightedISSLayer(words, weighting=w)
    for semiring in (fr.semiring.Arctic(), fr.semiring.Bayesian()):
        op = fr.ISS(words, semiring=semiring, weighting=Indices())
        with pytest.raises(NotImplementedError, match="semiring"):
            nn.weighted_iss(X, op)
        with pytest.raises(NotImplementedError, match="semiring"):
            nn.WeightedISSLayer(op)
    generic = fr.words.Word("[DIM(1)][ABS(2)]")
    with pytest.raises(NotImplementedError, match="generic"):
        nn.weighted_iss(X, [words[0], generic], weighting=Indices())
    with pytest.raises(NotImplementedError, match="generic"):
        nn.WeightedISSLayer([generic], weighting=Indices())
    cos = fr.CosWISS(words, freqs=[0.5])
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.weighted_iss(X, cos)
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.WeightedISSLayer(cos)
    # an ISS brings its own weighting
    with pytest.raises(TypeError, match="its own weighting"):
        nn.weighted_iss(X, fr.ISS(words, weighting=Indices()), weighting=Plateaus(3))
    # the unweighted functions still refuse a weighting, and say where to go
    with pytest.raises(NotImplementedError, match="weighting"):
        nn.iss(X, words, weighting=Indices())
    with pytest.raises(NotImplementedError, match="weighted_iss"):
        nn.ISSLayer(words, weighting=Indices())


def test_prefix_program_keys_nodes_by_letters_and_alphas():
    """The weighted prefix plan: equal letters with other alphas are other nodes; in EXTENDED mode
    a row maps to the prefix with the alphas of the word that emits it."""
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    from fruits_amd.iss.weighting import Indices
    words = [fr.words.SimpleWord(s) for s in ("[1]", "[1][2]", "[1][2]", "[1][2][1]")]
    for w, a in zip(words, ([1.0], [2.0, 1.0], [2.0, 0.5], [2.0, 1.0, 3.0])):
        w.alpha = a
    for total in (False, True):
        op = fr.ISS(words, mode=fr.ISSMode.EXTENDED, weighting=Indices(total=total))
        plan, rows = nn._weighted_prefix_program(op)
        # EXTENDED rows: [1] of word 0; [1][2] of word 1 (its [1] is out already, but with another
        # alpha: an inner node of its own); word 2 is a twin by letters - no rows, no work;
        # [1][2][1] of word 3.  Prefixes: [1]a1 | [1]a2, [1]a2[2]a1 | [1]a2[2]a1[1]a3
        assert plan.nodes == plan.rows == 4 and plan.info(nat.FR_INFO_ALPHAS) == 3
        assert plan.weighting == (nat.FR_W_TOTAL if total else nat.FR_W_NONTOTAL)
        assert rows.tolist() == [0, 2, 3]
        assert nn._weighted_prefix_program(op)[0] is plan
        # SINGLE: the twin is a row, and with its other alpha a node: [1]a2[2]a.5
        single = fr.ISS(words, mode=fr.ISSMode.SINGLE, weighting=Indices(total=total))
        plan, rows = nn._weighted_prefix_program(single)
        assert plan.nodes == 5 and plan.info(nat.FR_INFO_ALPHAS) == 4 and rows.tolist() == [0, 2, 3, 4]
        # other alphas, another program
        words[2].alpha = [2.0, 1.0]
        assert nn._weighted_prefix_program(single)[1].tolist() == [0, 2, 2, 3]
        words[2].alpha = [2.0, 0.5]


def test_layer_is_a_plain_module():
    """No parameters; copies and pickles without its device programs."""
    import copy
    import pickle
    import fruits_amd as fr
    from fruits_amd import nn
    from fruits_amd.iss.weighting import Plateaus
    words = fr.words.of_weight(2, dim=2)
    layer = nn.WeightedISSLayer(words, fr.ISSMode.EXTENDED, weighting=Plateaus(4, total=True))
    assert list(layer.parameters()) == [] and list(layer.buffers()) == []
    assert "Plateaus total" in repr(layer)
    nn._weighted_prefix_program(layer.op)
    for dup in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
        assert isinstance(dup, nn.WeightedISSLayer) and dup.mode == fr.ISSMode.EXTENDED
        assert [str(w) for w in dup.words] == [str(w) for w in words]
        assert isinstance(dup.weighting, Plateaus) and dup.weighting.total
        assert dup.op._plans == {}
