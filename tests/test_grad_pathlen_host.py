"""The gradient through the path-length lookup (L1 / L2) without a GPU: the long-double recursion
against a central difference of the forward oracle, its exact cases, the derived bound and what
falls outside it, the stream-less setter and its refusals, and the refusals of
fruits_amd.nn.pathlen_iss - all raised before any device call."""
import os
import re

import numpy as np
import pytest

import iss_bounds as ib
import iss_grad_pathlen_ref as gp
import iss_grad_ref as gr
import iss_grad_weighted_ref as gw

HERE = os.path.dirname(os.path.abspath(__file__))
orc = gr.orc

WORDS = ["[1][2]", "[11][2][1]", "[2]"]
ALPHAS = [np.array(a, dtype=np.float32) for a in ([0.5, 1.5], [1.25, 0.25, 2.0], [0.75])]


def moving_input(N, D, T, seed):
    """Standard normal X whose dimension 0 moves by at least 0.25 in every step: no kink of |dx|
    within a difference step."""
    rng = np.random.default_rng([seed, N, D, T])
    X = rng.standard_normal((N, D, T))
    steps = rng.uniform(0.25, 1.0, (N, T)) * rng.choice([-1.0, 1.0], (N, T))
    X[:, 0] = np.cumsum(steps, axis=1)
    return X


def lookup_of(norm):
    return orc.lookup_l1 if norm == 1 else orc.lookup_l2


@pytest.mark.parametrize("relative", [False, True], ids=["absolute", "relative"])
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("norm", [1, 2], ids=["l1", "l2"])
def test_recursion_is_the_gradient_of_the_forward_oracle(norm, total, mode, relative):
    """A central difference of ``orc.iss_transform`` composed with ``orc.lookup_l1`` / ``lookup_l2``
    agrees with input part + lookup part, ``relative`` either way: the + 1e-5 cancels."""
    N, D, T = 2, 2, 7
    X = moving_input(N, D, T, seed=8)
    assert np.abs(np.diff(X[:, 0], axis=1)).min() >= 0.25
    rng = np.random.default_rng([9, norm, total, relative])
    K = len(gw.output_nodes(WORDS, ALPHAS, mode))
    G = rng.standard_normal((N, K, T))
    look = lookup_of(norm)

    def loss(Z):
        Y = orc.iss_transform(Z, WORDS, mode, ALPHAS, look(Z, relative, 2.0), total, dtype=gr.HP)
        return float((Y.transpose(1, 0, 2) * G).sum())

    g = look(X, relative, 2.0)
    inp, lk = gp.iss_grad_pathlen(X, G, WORDS, ALPHAS, g, total, norm, 2.0, mode, parts=True)
    got = gp.iss_grad_pathlen(X, G, WORDS, ALPHAS, g, total, norm, 2.0, mode).astype(np.float64)
    assert np.abs(lk).max() > 1e-3 and np.array_equal(got[:, 1], inp[:, 1].astype(np.float64))
    h = 1e-6
    for at in [(0, 0, 0), (1, 0, 3), (0, 0, 6), (1, 0, 5), (0, 1, 2), (1, 0, 1), (0, 0, 4)]:
        Zp, Zm = X.copy(), X.copy()
        Zp[at] += h
        Zm[at] -= h
        fd = (loss(Zp) - loss(Zm)) / (2 * h)
        assert abs(fd - got[at]) <= 1e-7 * max(1.0, abs(got[at])), (at, fd, got[at])
        # without the lookup part the first dimension is elsewhere
        if at[1] == 0:
            assert abs(fd - float(inp[at])) > 1e-5 * max(1.0, abs(got[at])), (at, fd, float(inp[at]))


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("norm", [1, 2], ids=["l1", "l2"])
def test_alpha_zero_is_the_unweighted_recursion(norm, total):
    words = ["[1]", "[1][2]", "[1][2][1]", "[2]", "[11][2]"]
    alphas = [np.zeros(len(orc.parse_word(w)), dtype=np.float32) for w in words]
    N, D, T = 3, 2, 40
    X = np.random.default_rng(5).integers(-2, 3, size=(N, D, T)).astype(np.float64)
    K = len(gr.output_prefixes(words, "EXTENDED"))
    G = np.random.default_rng(6).integers(-3, 4, size=(N, K, T)).astype(np.float64)
    g = lookup_of(norm)(X, False, 5.0)
    assert g.max() == 5.0
    got = gp.iss_grad_pathlen(X, G, words, alphas, g, total, norm, 5.0, "EXTENDED")
    want = gr.iss_grad(X, G, words, "EXTENDED")
    assert np.array_equal(got, want) and np.abs(want).max() > 0
    assert not gp.iss_grad_lookup(X, G, words, alphas, g, total, "EXTENDED").any()


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("norm", [1, 2], ids=["l1", "l2"])
def test_constant_first_dimension_gets_no_lookup_part(norm, total):
    """r_L = 0: g = 0 and every exp factor 1.0 - the unweighted gradient exactly, finite; T = 1 too."""
    for T in (1, 9):
        X = np.random.default_rng([7, T]).integers(-2, 3, size=(2, 2, T)).astype(np.float64)
        X[:, 0] = 3.0
        K = len(gr.output_prefixes(WORDS, "SINGLE"))
        G = np.random.default_rng(8).integers(-3, 4, size=(2, K, T)).astype(np.float64)
        g = lookup_of(norm)(X, False, 5.0)
        assert not g.any()
        got = gp.iss_grad_pathlen(X, G, WORDS, ALPHAS, g, total, norm, 5.0)
        assert np.isfinite(got.astype(np.float64)).all()
        assert np.array_equal(got, gr.iss_grad(X, G, WORDS, "SINGLE"))


def test_a_flat_stretch_contributes_nothing_for_l1():
    """sign(0) = 0: inside a stretch where dimension 0 does not move the lookup part is exactly 0
    (both neighbouring increments vanish), while the series as a whole has one."""
    N, T = 2, 12
    X = moving_input(N, 2, T, seed=3)
    X[:, 0, 4:9] = X[:, 0, 4:5]
    dg = np.random.default_rng(4).standard_normal((N, T))
    g = orc.lookup_l1(X, False, 5.0)
    out = gp.pathlen_grad(X, dg, g, 1, 5.0)
    assert not out[:, 5:8].any() and np.abs(out[:, :4]).min() > 0 and np.isfinite(out.astype(np.float64)).all()
    # L2: 2 dx = 0 there as well
    assert not gp.pathlen_grad(X, dg, orc.lookup_l2(X, False, 5.0), 2, 5.0)[:, 5:8].any()


def test_n_ops_grad_pathlen_counts():
    lookup = np.array([[0.0, 1.5]])
    base = gw.n_ops_grad_weighted(["[1][2]"], [[1.0, 2.0]], lookup, 10)
    # W = 2, V = 2: + W + 6 + 2 V for one term of dg, + 3 T + 8 through the path length
    assert gp.n_ops_grad_lookup(["[1][2]"], [[1.0, 2.0]], lookup, 10) == base + 2 + 6 + 4
    assert gp.n_ops_grad_pathlen(["[1][2]"], [[1.0, 2.0]], lookup, 10) == base + 2 + 6 + 4 + 30 + 8


@pytest.mark.parametrize("norm", [1, 2], ids=["l1", "l2"])
def test_bound_holds_for_float64_and_can_fail(norm):
    """The float64 run of the recursion lies within the derived bound of the long-double one; a
    relative error of 1e-10, a dropped lookup part and the other body lie outside."""
    words, T = ib.WORDS, 700
    rng = np.random.default_rng(4)
    alphas = [rng.uniform(0.25, 2.0, len(orc.parse_word(w))).astype(np.float32) for w in words]
    X = rng.random((2, 3, T)) + 0.25
    g = lookup_of(norm)(X, False, 5.0)
    K = len(gw.output_nodes(words, alphas, "EXTENDED"))
    G = rng.random((2, K, T))
    n = gp.n_ops_grad_pathlen(words, alphas, g, T, "EXTENDED")
    for total in (False, True):
        args = (X, G, words, alphas, g, total, norm, 5.0, "EXTENDED")
        hp = gp.iss_grad_pathlen(*args)
        A = gp.iss_grad_pathlen(*args, magnitude=True)
        f64 = gp.iss_grad_pathlen(*args, dtype=np.float64)
        ib.check_bound(f64, hp, A, n, f"float64 recursion norm={norm} total={total}")
        assert ib.violates(f64 * (1 + 1e-10), hp, A, n)
        inp, _ = gp.iss_grad_pathlen(*args, dtype=np.float64, parts=True)
        assert ib.violates(inp, hp, A, n)
        other = gp.iss_grad_pathlen(X, G, words, alphas, g, not total, norm, 5.0, "EXTENDED", dtype=np.float64)
        assert ib.violates(other, hp, A, n)
        # dg alone, with its own count
        dg_hp = gp.iss_grad_lookup(X, G, words, alphas, g, total, "EXTENDED")
        dg_A = gp.iss_grad_lookup(X, G, words, alphas, g, total, "EXTENDED", magnitude=True)
        dg_64 = gp.iss_grad_lookup(X, G, words, alphas, g, total, "EXTENDED", dtype=np.float64)
        ib.check_bound(dg_64, dg_hp, dg_A, gp.n_ops_grad_lookup(words, alphas, g, T, "EXTENDED"), "float64 dg")


# ---------------------------------------------------------------- the setter
def header():
    with open(os.path.join(os.path.dirname(HERE), "include", "fruits_hip.h")) as f:
        return f.read()


def test_setter_is_exported_and_takes_no_stream():
    from fruits_amd import _native as nat
    L = nat.lib()
    assert "fr_plan_set_grad_pathlen" in nat.EXPORTS and hasattr(L, "fr_plan_set_grad_pathlen")
    text = header()
    assert text.count("int fr_plan_set_grad_pathlen(") == 1
    decl = re.search(r"int fr_plan_set_grad_pathlen\(([^;]*)\);", text).group(1)
    assert "stream" not in decl and "void *" not in decl
    assert L.fr_version() >= 144


def test_setter_and_armed_entry_check_before_any_device_call():
    """Every FR_E_ARG of fr_plan_set_grad_pathlen and of the armed entries is returned on the host:
    no pointer below is ever dereferenced."""
    import ctypes as C
    from fruits_amd import _native as nat
    L = nat.lib()
    i64, i32, f64 = C.c_int64, C.c_int32, C.c_double
    p = C.c_void_p(4096)
    null = C.c_void_p(0)
    DG, R = C.c_void_p(24576), C.c_void_p(28672)
    tab = lambda *rows: np.array(rows, dtype=np.int32)
    f32 = lambda *v: np.array(v, dtype=np.float32)
    rows = np.array([1], dtype=np.int32)
    rp = rows.ctypes.data_as(C.POINTER(C.c_int32))
    who = "fr_plan_set_grad_pathlen: "

    def arm(plan, N=2, norm=1, scale=5.0, dg=DG, r=R):
        return L.fr_plan_set_grad_pathlen(plan._h if plan is not None else None, i64(N), i32(norm),
                                          f64(scale), dg, r)

    def weighted(plan, N=2, lr=2, X=p, Cs=C.c_void_p(12288), A=C.c_void_p(16384)):
        return L.fr_iss_backward_weighted(plan._h, X, i64(N), i64(2), i64(5), p, i64(lr), p, i64(1), i64(5),
                                          i64(5), i64(1), rp, Cs, A, C.c_void_p(20480), C.c_void_p(8192), null)

    def picked(plan):
        return L.fr_iss_backward_picked(plan._h, p, i64(2), i64(2), i64(5), null, p, i64(2), p, p, i64(1),
                                        i32(1), rp, C.c_void_p(12288), C.c_void_p(16384), C.c_void_p(20480),
                                        C.c_void_p(8192), null)

    assert arm(None) == nat.FR_E_ARG and nat.last_error() == who + "null plan"
    for wmode in (nat.FR_W_NONTOTAL, nat.FR_W_TOTAL):
        prefix = nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1], [f32(1.0), f32(1.0, 0.5)], wmode)
        unweighted = nat.Plan([tab([1]), tab([1, 0], [0, 1])], [1, 1])
        arctic = nat.Plan([tab([1])], [1], [f32(1.0)], wmode, arctic=True)
        cos = nat.CosPlan([tab([1])], [0.5], 1, False)
        cases = [
            (lambda: arm(prefix, N=-1), "bad shape"),
            (lambda: arm(prefix, norm=0), "the norm has to be 1 (L1) or 2 (L2), not 0"),
            (lambda: arm(prefix, norm=3), "not 3"),
            (lambda: arm(prefix, scale=float("inf")), "the scale has to be finite"),
            (lambda: arm(prefix, scale=float("nan")), "the scale has to be finite"),
            (lambda: arm(unweighted), "not a weighted Reals trie plan"),
            (lambda: arm(arctic), "not a weighted Reals trie plan"),
            (lambda: arm(cos), "not a weighted Reals trie plan"),
            (lambda: arm(prefix, r=DG), "distinct buffers"),
        ]
        if wmode == nat.FR_W_NONTOTAL:
            cases.append((lambda: arm(prefix, r=null), "a non-total plan needs the scratch d_R"))
        for fn, text in cases:
            assert fn() == nat.FR_E_ARG, text
            assert nat.last_error().startswith(who) and text in nat.last_error(), (text, nat.last_error())
        # a refused setter arms nothing: the entry goes on to its own checks (a null input here)
        assert weighted(prefix, X=null) == nat.FR_E_ARG and "null device pointer" in nat.last_error()
        if wmode == nat.FR_W_TOTAL:
            assert arm(prefix, r=null) == 0          # (a total plan keeps no R)
        assert arm(prefix) == 0
        armed = [
            (lambda: weighted(prefix, N=3, lr=3), "was set for 2 series (fr_plan_set_grad_pathlen), the call brings 3"),
            (lambda: weighted(prefix, lr=1), "the lookup has to have N rows, one per series, not 1"),
            (lambda: weighted(prefix, A=DG), "must be distinct from the call's buffers"),
            (lambda: weighted(prefix, X=null), "null device pointer"),
        ]
        if wmode == nat.FR_W_NONTOTAL:
            armed.append((lambda: weighted(prefix, Cs=R), "must be distinct from the call's buffers"))
        for fn, text in armed:
            assert fn() == nat.FR_E_ARG, text
            assert nat.last_error().startswith("fr_iss_backward_weighted: ") and text in nat.last_error(), \
                (text, nat.last_error())
        assert picked(prefix) == nat.FR_E_ARG
        assert nat.last_error().startswith("fr_iss_backward_picked: ")
        assert "only fr_iss_backward_weighted carries a gradient through it" in nat.last_error()
        # armed with lengths too
        assert L.fr_plan_set_grad_lengths(prefix._h, p, i64(2)) == 0
        assert weighted(prefix) == nat.FR_E_ARG
        assert "fr_plan_set_grad_lengths" in nat.last_error() and "fr_plan_set_grad_pathlen" in nat.last_error()
        assert L.fr_plan_set_grad_lengths(prefix._h, None, i64(0)) == 0
        # nothing to do, after the same checks; then cleared: the plain entry's answers again
        assert weighted(prefix, N=0, lr=0) == nat.FR_E_ARG and "was set for 2 series" in nat.last_error()
        assert arm(prefix, N=0) == 0 and weighted(prefix, N=0, lr=0) == 0
        assert arm(prefix, dg=null, r=null) == 0
        assert weighted(prefix, lr=3) == nat.FR_E_ARG and "1 or N rows, not 3" in nat.last_error()


# ---------------------------------------------------------------- fruits_amd.nn
def test_import_stays_lazy():
    import subprocess
    import sys
    code = ("import sys, fruits_amd\n"
            "assert 'torch' not in sys.modules and 'fruits_amd.nn' not in sys.modules\n"
            "import fruits_amd.nn as m\n"
            "assert callable(m.pathlen_iss) and 'pathlen_iss' in m.__all__\n"
            "assert 'PathLengthISSLayer' in m.__all__ and 'torch.nn' in sys.modules\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(HERE))


def test_refusals_need_no_device():
    import torch
    import fruits_amd as fr
    from fruits_amd import nn
    from fruits_amd.iss.weighting import L1, L2, Custom, Indices, Plateaus
    words = [fr.words.SimpleWord("[1][2]")]
    X = torch.zeros((2, 2, 5), dtype=torch.float64)
    for w in (L1(), L1(total=True), L2(relative=True), L2(scale=3, total=True), L1(on_prepared=True)):
        # a supported configuration on a host tensor: the input checks, the device last
        with pytest.raises(TypeError, match="GPU"):
            nn.pathlen_iss(X, words, weighting=w)
        with pytest.raises(TypeError, match="GPU"):
            nn.PathLengthISSLayer(words, fr.ISSMode.EXTENDED, weighting=w)(X)
        with pytest.raises(TypeError, match="GPU"):
            nn.pathlen_iss(X, fr.ISS(words, weighting=w))
        with pytest.raises(TypeError, match="float64"):
            nn.pathlen_iss(X.float(), words, weighting=w)
        with pytest.raises(TypeError, match=r"\(N, D, T\)"):
            nn.pathlen_iss(X[0], words, weighting=w)
        with pytest.raises(TypeError, match="torch.Tensor"):
            nn.pathlen_iss(X.numpy(), words, weighting=w)
        with pytest.raises(IndexError, match="references dimension 2 but the input has only 1"):
            nn.pathlen_iss(X[:, :1], words, weighting=w)
        with pytest.raises(NotImplementedError, match="lengths"):
            nn.pathlen_iss(X, words, weighting=w, lengths=[5, 4])
        with pytest.raises(NotImplementedError, match="lengths"):
            nn.PathLengthISSLayer(words, weighting=w)(X, lengths=[5, 4])
    with pytest.raises(NotImplementedError, match=r"nn\.iss"):
        nn.pathlen_iss(X, words)
    with pytest.raises(NotImplementedError, match=r"nn\.iss"):
        nn.PathLengthISSLayer(words, weighting=None)
    for w in (Indices(), Plateaus(3, total=True)):
        with pytest.raises(NotImplementedError, match=r"nn\.weighted_iss"):
            nn.pathlen_iss(X, words, weighting=w)
        with pytest.raises(NotImplementedError, match=r"nn\.weighted_iss"):
            nn.PathLengthISSLayer(words, weighting=w)
    with pytest.raises(NotImplementedError, match="arbitrary callable"):
        nn.pathlen_iss(X, words, weighting=Custom(lambda Z: Z[:, 0, :]))
    for w in (L1(transform=np.sqrt), L2(transform=np.sqrt, total=True)):
        with pytest.raises(NotImplementedError, match="transform"):
            nn.pathlen_iss(X, words, weighting=w)
        with pytest.raises(NotImplementedError, match="transform"):
            nn.PathLengthISSLayer(words, weighting=w)
    for semiring in (fr.semiring.Arctic(), fr.semiring.Bayesian()):
        op = fr.ISS(words, semiring=semiring, weighting=L1())
        with pytest.raises(NotImplementedError, match="semiring"):
            nn.pathlen_iss(X, op)
        with pytest.raises(NotImplementedError, match="semiring"):
            nn.PathLengthISSLayer(op)
    generic = fr.words.Word("[DIM(1)][ABS(2)]")
    with pytest.raises(NotImplementedError, match="generic"):
        nn.pathlen_iss(X, [words[0], generic], weighting=L1())
    with pytest.raises(NotImplementedError, match="generic"):
        nn.PathLengthISSLayer([generic], weighting=L2())
    cos = fr.CosWISS(words, freqs=[0.5])
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.pathlen_iss(X, cos)
    with pytest.raises(NotImplementedError, match="CosWISS"):
        nn.PathLengthISSLayer(cos)
    with pytest.raises(TypeError, match="its own weighting"):
        nn.pathlen_iss(X, fr.ISS(words, weighting=L1()), weighting=L2())
    # the other entries keep their refusals of L1 / L2
    with pytest.raises(NotImplementedError, match="depends on the input"):
        nn.weighted_iss(X, words, weighting=L1())
    with pytest.raises(NotImplementedError):
        nn.FeatureLayer(words, sieves=[fr.sieving.END()], weighting=L1())


def test_layer_is_a_plain_module():
    import copy
    import pickle
    import fruits_amd as fr
    from fruits_amd import nn
    from fruits_amd.iss.weighting import L2
    words = fr.words.of_weight(2, dim=2)
    layer = nn.PathLengthISSLayer(words, fr.ISSMode.EXTENDED, weighting=L2(scale=3, total=True))
    assert list(layer.parameters()) == [] and list(layer.buffers()) == []
    assert "L2 total" in repr(layer)
    nn._prefix_program(layer.op)
    for dup in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
        assert isinstance(dup, nn.PathLengthISSLayer) and dup.mode == fr.ISSMode.EXTENDED
        assert [str(w) for w in dup.words] == [str(w) for w in words]
        assert isinstance(dup.weighting, L2) and dup.weighting.total and dup.weighting._scale == 3
        assert dup.op._plans == {}
