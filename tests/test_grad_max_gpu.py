"""GPU tests of the differentiable max semirings (fruits_amd.nn.max_iss, fr_iss_backward_max): the
forward bits, the gradient against the oracle of the adjoint recursion - bit for bit on inputs
where every sum and product is exact, ties included, within the derived rounding bound on
real-valued ones -, the positions of Arctic(argmax=True), repeatability and the autograd wiring."""
import os

import numpy as np
import pytest

import iss_bounds as ib
import iss_grad_max_ref as gm
import iss_grad_ref as gr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 1024       # time steps the suffix kernels scan at once (csrc/kernels.h, kGradChunk)
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
N = 3
# (D, words): a single letter; a chain of 3; siblings under one parent (one of them a row that is
# an inner node too); a multi-dimension letter; a negative exponent; a squared letter
WORD_SETS = {
    "one_letter": (1, ["[1]"]),
    "chain3": (2, ["[1][2][1]"]),
    "siblings": (3, ["[1]", "[1][1]", "[1][2]", "[1][3]"]),
    "multidim": (2, ["[12][2]"]),
    "negative": (2, ["[1][-2]"]),
    "square": (2, ["[11][2]"]),
}


@pytest.fixture(scope="module")
def env():
    import torch
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    nat.require_device()
    yield fr, nn, torch
    ib.print_ratios()


def words_of(fr, strings):
    return [fr.words.SimpleWord(s) for s in strings]


def mode_of(fr, mode):
    return fr.ISSMode.EXTENDED if mode == "EXTENDED" else fr.ISSMode.SINGLE


def semiring_of(fr, semiring):
    return fr.semiring.Arctic() if semiring == "Arctic" else fr.semiring.Bayesian()


def exact_input(semiring, D, T, seed=0):
    """(N, D, T) on which every sum and product of the forward and the backward pass is exact.
    Arctic: small integers from [-2, 2], ties everywhere - series 0 as they are (the running
    maxima saturate: heads in front only, one open segment across every chunk behind), series 1
    on a slow staircase t // 5 (heads and ties all along), series 2 on a falling one.  Bayesian:
    powers of two from [1/4, 2]."""
    rng = np.random.default_rng([seed, D, T])
    if semiring == "Bayesian":
        return 2.0 ** rng.integers(-2, 2, size=(N, D, T)).astype(np.float64)
    X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    X[1] += np.arange(T) // 5
    X[2] -= np.arange(T) // 5
    return X


def shaped_input(semiring, shape, T):
    """(N, 2, T) series of one shape: ``decreasing`` - a single head, at t = 0, and one segment
    across every lane, wave and chunk edge; ``increasing`` - a head at every step; ``staircase``
    - a head every third step, ties between.  Arctic: integers; Bayesian: 1 + k / 4096 (13
    bits: the products of the words used with it stay exact), dimension d scaled by 2^d."""
    t = np.arange(T, dtype=np.float64)
    f = {"decreasing": T - 1 - t, "increasing": t, "staircase": np.floor(t / 3)}[shape]
    X = np.empty((N, 2, T))
    for n in range(N):
        for d in range(2):
            X[n, d] = f + n + d if semiring == "Arctic" else (1 + (f + n) / 4096) * 2.0 ** d
    return X


def device_grad(env, X, G, strings, mode, semiring):
    """X.grad of ``(nn.max_iss(X) * G).sum()`` as a host array, and the forward result."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)       # (copies: the shared cases are read-only)
    Y = nn.max_iss(Xd, words_of(fr, strings), mode_of(fr, mode), semiring=semiring_of(fr, semiring))
    Y.backward(torch.tensor(G, device="cuda"))
    return Xd.grad.cpu().numpy(), Y.detach().cpu().numpy()


def int_gradient(strings, mode, T, seed):
    K = len(gr.output_prefixes(strings, mode))
    return np.random.default_rng([seed, T, K]).integers(-3, 4, size=(N, K, T)).astype(np.float64)


def oracle_rows(X, strings, mode, semiring):
    """The oracle's iterated sums in the layout of nn.max_iss, (N, K, T)."""
    return gr.orc.iss_transform(X, strings, mode, semiring=semiring).transpose(1, 0, 2)


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
def test_forward_bits(env, mode, semiring):
    fr, nn, torch = env
    strings = ["[1][2][3]", "[11][2]", "[1][-2]", "[12][2][3][1]"] + gr.orc.of_weight_strings(2, 3)
    words = words_of(fr, strings)
    rng = np.random.default_rng(3)
    X = rng.standard_normal((N, 3, 300)) if semiring == "Arctic" else 0.25 + 0.75 * rng.random((N, 3, 300))
    op = fr.ISS(words, mode=mode_of(fr, mode), semiring=semiring_of(fr, semiring))
    Xd = torch.from_numpy(X).cuda()
    want = op.transform_device(Xd).cpu().numpy()                       # (K, N, T)
    Y = nn.max_iss(Xd, words, mode_of(fr, mode), semiring=semiring_of(fr, semiring))
    assert Y.shape == (N, want.shape[0], 300) and Y.device == Xd.device and not Y.requires_grad
    # a permuted view of the walk's (K, N, T) buffer, not a copy
    assert not Y.is_contiguous() and Y.permute(1, 0, 2).is_contiguous()
    np.testing.assert_array_equal(Y.cpu().numpy(), want.transpose(1, 0, 2))
    np.testing.assert_array_equal(Y.cpu().numpy(), oracle_rows(X, strings, mode, semiring))
    # the layer, an ISS that carries the semiring, and an input that is not contiguous
    Xt = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).cuda().transpose(1, 2)
    assert not Xt.is_contiguous()
    layer = nn.MaxISSLayer(words, mode_of(fr, mode), semiring=semiring_of(fr, semiring))
    np.testing.assert_array_equal(layer(Xt).cpu().numpy(), want.transpose(1, 0, 2))
    np.testing.assert_array_equal(nn.max_iss(Xd, op).cpu().numpy(), want.transpose(1, 0, 2))


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("name", list(WORD_SETS))
def test_gradient_exact(env, name, T, mode, semiring):
    D, strings = WORD_SETS[name]
    X = exact_input(semiring, D, T)
    G = int_gradient(strings, mode, T, seed=5)
    got, Y = device_grad(env, X, G, strings, mode, semiring)
    # the precondition for shared heads: the forward bits are the oracle's
    np.testing.assert_array_equal(Y, oracle_rows(X, strings, mode, semiring))
    want = gm.iss_grad_max(X, G, strings, mode, semiring)
    assert np.abs(want).max() < 2.0 ** 50 and (want == want.astype(np.float64)).all()
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=f"{semiring} {name} T={T} {mode}")
    if T >= 63:
        assert gm.smallest_gap(X, strings, mode, semiring) == 0.0        # ties included
        assert np.abs(want).max() > 0


@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("shape", ["decreasing", "increasing", "staircase"])
def test_gradient_exact_shapes(env, shape, T, semiring):
    """One head at t = 0, a head at every step, a head every third step: segments across - and
    heads on - every lane, wave and chunk edge."""
    strings, mode = ["[1]", "[1][2]"], "EXTENDED"
    X = shaped_input(semiring, shape, T)
    G = int_gradient(strings, mode, T, seed=6)
    got, Y = device_grad(env, X, G, strings, mode, semiring)
    np.testing.assert_array_equal(Y, oracle_rows(X, strings, mode, semiring))
    want = gm.iss_grad_max(X, G, strings, mode, semiring)
    assert np.abs(want).max() < 2.0 ** 50 and (want == want.astype(np.float64)).all()
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=f"{semiring} {shape} T={T}")
    # the shape is what it says: where the gradient of dimension 1 may be non-zero
    heads = (got[:, 0] != 0).sum(axis=1)
    if shape == "decreasing":
        assert (got[:, :, 1:] == 0).all()
    elif shape == "staircase":
        assert (heads <= -(-T // 3)).all() and (got[:, 0, np.arange(T) % 3 != 0] == 0).all()


# ---------------------------------------------------------------- the derived bound
WORDS = ["[1][2][3]", "[11][2]", "[1][-2]", "[12][2][3][1]"]
BOUND_CASES = {
    # (D, T, words, mode, trend): `trend` tilts an Arctic input upwards - the running maxima
    # then rise all along the series, not only at its rare records
    "words_700": (3, 700, WORDS, "EXTENDED", 0.0),
    "words_2051": (3, 2 * CHUNK + 3, WORDS, "EXTENDED", 0.02),
    "words_1025_single": (3, CHUNK + 1, WORDS, "SINGLE", 0.02),
    "of_weight32_1024": (2, CHUNK, gr.orc.of_weight_strings(3, 2), "EXTENDED", 0.05),
}
_REAL = {}


def real_case(name, semiring):
    """(X, G, hp, A, n) of a bound case: computed once, shared, never changed.  Arctic: standard
    normal plus the trend; Bayesian: uniform in [0.25, 1]."""
    if (name, semiring) not in _REAL:
        D, T, strings, mode, trend = BOUND_CASES[name]
        rng = np.random.default_rng([7, D, T, semiring == "Arctic"])
        if semiring == "Arctic":
            X = rng.standard_normal((N, D, T)) + trend * np.arange(T)
        else:
            X = 0.25 + 0.75 * rng.random((N, D, T))
        G = rng.standard_normal((N, len(gr.output_prefixes(strings, mode)), T))
        hp = gm.iss_grad_max(X, G, strings, mode, semiring)
        A = gm.iss_grad_max(X, G, strings, mode, semiring, magnitude=True)
        for a in (X, G, hp, A):
            a.setflags(write=False)
        _REAL[name, semiring] = (X, G, hp, A, gm.n_ops_grad_max(strings, T, mode, semiring))
    return _REAL[name, semiring]


@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_gradient_within_bound(env, name, semiring):
    """|device - iss_grad_max| <= 2 n_ops_grad_max 2^-53 iss_grad_max(magnitude=True), elementwise."""
    _, _, strings, mode, _ = BOUND_CASES[name]
    X, G, hp, A, n = real_case(name, semiring)
    if semiring == "Bayesian":
        assert X.min() >= 0.25 and X.max() <= 1.0
    got, Y = device_grad(env, X, G, strings, mode, semiring)
    np.testing.assert_array_equal(Y, oracle_rows(X, strings, mode, semiring))
    worst = ib.check_bound(got, hp, A, n, f"grad {semiring} {name}", family=f"grad_max_{semiring}")
    print(f"grad {semiring} {name}: n_ops_grad_max = {n}, heads of dimension 1: "
          f"{int((A[:, 0] != 0).sum())}, largest err / bound = {worst:.3g}")


# ---------------------------------------------------------------- against Arctic(argmax=True)
@pytest.mark.parametrize("word", ["[1][2][1]", "[2][2]", "[1][3][2][1]"])
@pytest.mark.parametrize("T", [1, 7, 300, CHUNK + 5])
def test_gradient_counts_the_argmax_positions(env, word, T):
    """A one-hot G at the last step of the full word's row: dX[n, d, s] is the number of letters
    of dimension d + 1 whose back-tracked position - the last column of the position rows of
    ISS([word], EXTENDED, semiring=Arctic(argmax=True)), code pinned by the reference's goldens
    - is s.  Small integers: ties included."""
    fr, nn, torch = env
    D = 3
    X = np.random.default_rng([8, T, len(word)]).integers(-1, 2, size=(N, D, T)).astype(np.float64)
    X[1] += np.arange(T) // 4
    w = fr.words.SimpleWord(word)
    L = len(w)
    rows = fr.ISS([w], mode=fr.ISSMode.EXTENDED, semiring=fr.semiring.Arctic(argmax=True)).transform(X)
    index = (L - 1) + (L - 1) * L // 2                  # the block of the full word: value, then L positions
    positions = rows[index + 1:index + 1 + L, :, -1]    # (L, N)
    dims = [int(c) - 1 for c in word.replace("[", "").replace("]", "")]
    want = np.zeros((N, D, T))
    for k in range(L):
        for n in range(N):
            assert positions[k, n] == int(positions[k, n]) and 0 <= positions[k, n] < T
            want[n, dims[k], int(positions[k, n])] += 1.0
    G = np.zeros((N, 1, T))
    G[:, 0, -1] = 1.0
    got, Y = device_grad(env, X, G, [word], "SINGLE", "Arctic")
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(Y[:, 0], rows[index])
    if T >= 7:
        assert gm.smallest_gap(X, [word], "SINGLE", "Arctic") == 0.0


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
def test_backward_is_repeatable(env, semiring):
    _, _, strings, mode, _ = BOUND_CASES["words_2051"]
    X, G, _, _, _ = real_case("words_2051", semiring)
    first, _ = device_grad(env, X, G, strings, mode, semiring)
    again, _ = device_grad(env, X, G, strings, mode, semiring)
    np.testing.assert_array_equal(first, again)
    # the batch in two launches of 1 and 2 series: another grid, the same bits
    parts = [device_grad(env, np.ascontiguousarray(X[s]), np.ascontiguousarray(G[s]), strings, mode, semiring)[0]
             for s in (slice(0, 1), slice(1, 3))]
    np.testing.assert_array_equal(np.concatenate(parts), first)


# ---------------------------------------------------------------- autograd
def gradcheck_input(semiring, string, step=1e-6):
    """A seeded (2, 2, 9) input whose smallest gap exceeds 100 steps of gradcheck's difference
    quotient: no head appears or disappears while an element moves by +-step."""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((2, 2, 9)) if semiring == "Arctic" else 0.25 + 0.75 * rng.random((2, 2, 9))
    for mode in ("SINGLE", "EXTENDED"):
        assert gm.smallest_gap(X, [string], mode, semiring) > 100 * step
    return X


@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
@pytest.mark.parametrize("string", ["[1][2]", "[11][2]"])
def test_gradcheck(env, string, semiring):
    fr, nn, torch = env
    X = torch.from_numpy(gradcheck_input(semiring, string)).cuda().requires_grad_(True)
    words = words_of(fr, [string])
    sr = semiring_of(fr, semiring)
    assert torch.autograd.gradcheck(lambda x: nn.max_iss(x, words, semiring=sr), (X,))
    assert torch.autograd.gradcheck(nn.MaxISSLayer(words, fr.ISSMode.EXTENDED, semiring=sr), (X,))


@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
def test_strided_upstream_gradient(env, semiring):
    """Y[:, :, -1].sum(): the upstream gradient reaches the backward pass with strides of its
    own (an expanded scalar in a slice of zeros); Y.sum(): all strides 0."""
    fr, nn, torch = env
    _, T, strings, mode, _ = BOUND_CASES["words_700"]
    X = real_case("words_700", semiring)[0]
    K = len(gr.output_prefixes(strings, mode))
    for pick, G in ((lambda Y: Y[:, :, -1].sum(), np.zeros((N, K, T))), (lambda Y: Y.sum(), np.ones((N, K, T)))):
        if not G.any():
            G[:, :, -1] = 1.0
        Xd = torch.tensor(X, device="cuda").requires_grad_(True)
        pick(nn.max_iss(Xd, words_of(fr, strings), mode_of(fr, mode), semiring=semiring_of(fr, semiring))).backward()
        hp = gm.iss_grad_max(X, G, strings, mode, semiring)
        A = gm.iss_grad_max(X, G, strings, mode, semiring, magnitude=True)
        ib.check_bound(Xd.grad.cpu().numpy(), hp, A, gm.n_ops_grad_max(strings, T, mode, semiring),
                       f"strided G {semiring}")


@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
def test_gradients_accumulate_and_none_without_requires_grad(env, semiring):
    fr, nn, torch = env
    D, strings = WORD_SETS["siblings"]
    X = exact_input(semiring, D, 65)
    layer = nn.MaxISSLayer(words_of(fr, strings), fr.ISSMode.EXTENDED, semiring=semiring_of(fr, semiring))
    Xd = torch.from_numpy(X).cuda().requires_grad_(True)
    G = torch.ones((N, len(gr.output_prefixes(strings, "EXTENDED")), 65), dtype=torch.float64, device="cuda")
    before = nn.backward_calls()
    layer(Xd).backward(G)
    once = Xd.grad.clone()
    layer(Xd).backward(G)
    assert nn.backward_calls() == before + 2
    assert torch.equal(Xd.grad, 2 * once) and once.abs().max() > 0
    # no gradient asked for: no graph, no backward work, no gradient
    Xn = Xd.detach()
    Y = layer(Xn)
    assert not Y.requires_grad and Y.grad_fn is None and Xn.grad is None
    with torch.no_grad():
        assert not layer(Xd).requires_grad
    assert nn.backward_calls() == before + 2
    # only X is kept for the backward pass
    Y = layer(Xd)
    assert [t.data_ptr() for t in Y.grad_fn.saved_tensors] == [Xd.data_ptr()]


@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
def test_layer_copies_and_pickles(env, semiring):
    import copy
    import pickle
    fr, nn, torch = env
    strings = gr.orc.of_weight_strings(2, 2)
    layer = nn.MaxISSLayer(words_of(fr, strings), fr.ISSMode.EXTENDED, semiring=semiring_of(fr, semiring))
    X = exact_input(semiring, 2, 130)
    G = np.ones((N, len(gr.output_prefixes(strings, "EXTENDED")), 130))
    want, Yw = device_grad(env, X, G, strings, "EXTENDED", semiring)
    layer(torch.from_numpy(X).cuda())            # (the original holds device programs by now)
    for dup in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer)), layer.to("cuda"), layer.double()):
        Xd = torch.from_numpy(X).cuda().requires_grad_(True)
        Y = dup(Xd)
        Y.backward(torch.from_numpy(G).cuda())
        np.testing.assert_array_equal(Y.detach().cpu().numpy(), Yw)
        np.testing.assert_array_equal(Xd.grad.cpu().numpy(), want)


# ---------------------------------------------------------------- the Reals path keeps its bits
def test_reals_backward_keeps_its_bits(env):
    """nn.iss shares the table builder and the kernel arguments with the max semirings: its
    gradient on a real-valued two-chunk case is, bit for bit, what the library computed before
    they were shared (tests/golden/grad_reals_before_max.npz, written on an MI355X by the commit
    before fr_iss_backward_max)."""
    fr, nn, torch = env
    gold = np.load(os.path.join(HERE, "golden", "grad_reals_before_max.npz"))
    rng = np.random.default_rng(12)
    X = rng.standard_normal((N, 3, CHUNK + 6))
    G = rng.standard_normal((N, len(gr.output_prefixes(WORDS, "EXTENDED")), CHUNK + 6))
    Xd = torch.from_numpy(X).cuda().requires_grad_(True)
    nn.iss(Xd, words_of(fr, WORDS), fr.ISSMode.EXTENDED).backward(torch.from_numpy(G).cuda())
    assert gold["dX"].shape == (N, 3, CHUNK + 6) and (gold["dX"] != 0).sum() > 9000
    np.testing.assert_array_equal(Xd.grad.cpu().numpy(), gold["dX"])


@pytest.mark.parametrize("semiring", gm.SEMIRINGS)
def test_max_backward_keeps_its_bits(env, semiring):
    """The segmented adjoints share their chunk frame, their gather and their input kernel with
    the additive ones: the gradient on a real-valued two-chunk case is, bit for bit, what the
    library computed before they were shared (tests/golden/grad_<semiring>_before_shared_frame.npz,
    written on an MI355X by tools/grad_golden.py on the commit before).  A trend keeps the running
    maxima rising: more than a thousand entries are heads."""
    gold = np.load(os.path.join(HERE, "golden", f"grad_{semiring.lower()}_before_shared_frame.npz"))
    rng = np.random.default_rng([12, semiring == "Arctic"])
    if semiring == "Arctic":
        X = rng.standard_normal((N, 3, CHUNK + 6)) + 0.02 * np.arange(CHUNK + 6)
    else:
        X = 1 + 0.25 * rng.random((N, 3, CHUNK + 6)) + 0.001 * np.arange(CHUNK + 6)
    G = rng.standard_normal((N, len(gr.output_prefixes(WORDS, "EXTENDED")), CHUNK + 6))
    got, _ = device_grad(env, X, G, WORDS, "EXTENDED", semiring)
    assert gold["dX"].shape == (N, 3, CHUNK + 6) and (gold["dX"] != 0).sum() > 1000
    np.testing.assert_array_equal(got, gold["dX"])
