"""GPU tests of the differentiable iterated sums (fruits_amd.nn, fr_iss_backward): the forward
bits, the gradient against the long-double oracle of the adjoint recursion - exactly on
integer-valued inputs, within the derived rounding bound on real-valued ones - repeatability and
the autograd wiring."""
import copy
import pickle

import numpy as np
import pytest

import iss_bounds as ib
import iss_grad_ref as gr

pytestmark = pytest.mark.gpu

CHUNK = 1024       # time steps the suffix kernel scans at once (csrc/kernels.h, kGradChunk)
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
# (D, words): of_weight(3, 2); a word that is a proper prefix of others - an inner node with an
# upstream gradient AND children; a sibling fan-out of four; a squared letter; a division; a word
# of one letter alone
WORD_SETS = {
    "of_weight32": (2, gr.orc.of_weight_strings(3, 2)),
    "of_weight32_D3": (3, gr.orc.of_weight_strings(3, 2)),       # a dimension no word names
    "prefix": (2, ["[1]", "[1][2]", "[1][2][1]", "[2]", "[1][2]"]),
    "fanout": (3, ["[1][1]", "[1][2]", "[1][3]", "[1][12]", "[3]"]),
    "square": (2, ["[11][2]"]),
    "division": (2, ["[1][-2]"]),
    "one_letter": (1, ["[1]"]),
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


def exact_input(strings, N, D, T, seed=0):
    """Integer-valued X from {-2 ... 2} - zeros included - and from {+-0.5, +-1, +-2} in the
    dimensions some word divides by: every partial sum of the gradient is a dyadic rational far
    below 2^53, so any order of the additions gives the same bits."""
    rng = np.random.default_rng([seed, N, D, T])
    X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    for d in {d for s in strings for row in gr.orc.parse_word(s) for d, e in enumerate(row) if e < 0}:
        X[:, d] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=(N, T))
    return X


def device_grad(env, X, G, strings, mode):
    """X.grad of ``(nn.iss(X) * G).sum()`` as a host array, and the forward result."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)       # (copies: the shared cases are read-only)
    Y = nn.iss(Xd, words_of(fr, strings), mode_of(fr, mode))
    Y.backward(torch.tensor(G, device="cuda"))
    return Xd.grad.cpu().numpy(), Y.detach().cpu().numpy()


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
def test_forward_bits(env, mode):
    fr, nn, torch = env
    strings = ib.WORDS + gr.orc.of_weight_strings(2, 3)
    words = words_of(fr, strings)
    X = np.random.default_rng(3).standard_normal((5, 3, 300))
    want = fr.ISS(words, mode=mode_of(fr, mode)).transform(X)            # (K, N, T)
    Xd = torch.from_numpy(X).cuda()
    Y = nn.iss(Xd, words, mode_of(fr, mode))
    assert Y.shape == (5, want.shape[0], 300) and Y.device == Xd.device and not Y.requires_grad
    # a permuted view of the walk's (K, N, T) buffer, not a copy
    assert not Y.is_contiguous() and Y.permute(1, 0, 2).is_contiguous()
    np.testing.assert_array_equal(Y.cpu().numpy(), want.transpose(1, 0, 2))
    # an input that is not contiguous is made so
    Xt = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).cuda().transpose(1, 2)
    assert not Xt.is_contiguous()
    np.testing.assert_array_equal(nn.ISSLayer(words, mode_of(fr, mode))(Xt).cpu().numpy(),
                                  want.transpose(1, 0, 2))


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("name", list(WORD_SETS))
def test_gradient_exact(env, name, T, mode):
    D, strings = WORD_SETS[name]
    # N in {1, 3, 261}, every one with every word set; the 261 series (more workgroups than one
    # round of the device) on the lengths up to 257: the long-double oracle costs seconds beyond
    at = LENGTHS.index(T) + list(WORD_SETS).index(name) + (mode == "EXTENDED")
    N = (1, 3, 261)[at % 3] if T <= 257 else (1, 3)[at % 2]
    X = exact_input(strings, N, D, T)
    K = len(gr.output_prefixes(strings, mode))
    G = np.random.default_rng([5, T, K, N]).integers(-3, 4, size=(N, K, T)).astype(np.float64)
    got, Y = device_grad(env, X, G, strings, mode)
    want = gr.iss_grad(X, G, strings, mode)
    assert np.abs(want).max() < 2.0 ** 50 and (want == want.astype(np.float64)).all()
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=f"{name} N={N} T={T} {mode}")
    np.testing.assert_array_equal(Y, gr.orc.iss_transform(X, strings, mode).transpose(1, 0, 2))


# ---------------------------------------------------------------- the derived bound
def real_input(strings, N, D, T, seed=0):
    """Standard normal X with a few exact zeros in the dimensions no word divides by."""
    rng = np.random.default_rng([seed, N, D, T, 7])
    X = rng.standard_normal((N, D, T))
    divided = {d for s in strings for row in gr.orc.parse_word(s) for d, e in enumerate(row) if e < 0}
    for d in sorted(set(range(D)) - divided):
        X[rng.integers(0, N, 5), d, rng.integers(0, T, 5)] = 0.0
    return X, rng.standard_normal


BOUND_CASES = {
    # (shape, words, mode); iss_bounds.WORDS name three dimensions: on (3, 2, 4099) they are an
    # IndexError, not a case
    "of_weight42_1024": ((7, 3, 1024), gr.orc.of_weight_strings(4, 2), "EXTENDED"),
    "of_weight42_4099": ((3, 2, 4099), gr.orc.of_weight_strings(4, 2), "EXTENDED"),
    "words_1024": ((7, 3, 1024), ib.WORDS, "EXTENDED"),
    "words_1024_single": ((7, 3, 1024), ib.WORDS, "SINGLE"),
    "words_4099": ((3, 3, 4099), ib.WORDS, "EXTENDED"),
}
_REAL = {}


def real_case(name):
    """(X, G, hp, A, n) of a bound case: computed once, shared, never changed."""
    if name not in _REAL:
        (N, D, T), strings, mode = BOUND_CASES[name]
        X, normal = real_input(strings, N, D, T)
        G = normal((N, len(gr.output_prefixes(strings, mode)), T))
        hp = gr.iss_grad(X, G, strings, mode)
        A = gr.iss_grad(X, G, strings, mode, magnitude=True)
        for a in (X, G, hp, A):
            a.setflags(write=False)
        _REAL[name] = (X, G, hp, A, gr.n_ops_grad(strings, T, mode))
    return _REAL[name]


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_gradient_within_bound(env, name):
    """|device - iss_grad| <= 2 n_ops_grad 2^-53 iss_grad(magnitude=True), elementwise."""
    _, strings, mode = BOUND_CASES[name]
    X, G, hp, A, n = real_case(name)
    assert (X == 0).sum() >= 3
    got, _ = device_grad(env, X, G, strings, mode)
    worst = ib.check_bound(got, hp, A, n, f"grad {name}", family="grad")
    print(f"grad {name}: n_ops_grad = {n}, largest err / bound = {worst:.3g}")


# ---------------------------------------------------------------- repeatability
def test_backward_is_repeatable(env):
    _, strings, mode = BOUND_CASES["of_weight42_1024"]
    X, G, _, _, _ = real_case("of_weight42_1024")
    first, _ = device_grad(env, X, G, strings, mode)
    again, _ = device_grad(env, X, G, strings, mode)
    np.testing.assert_array_equal(first, again)
    # the batch in two launches of 3 and 4 series: another grid, the same bits
    parts = [device_grad(env, np.ascontiguousarray(X[s]), np.ascontiguousarray(G[s]), strings, mode)[0]
             for s in (slice(0, 3), slice(3, 7))]
    np.testing.assert_array_equal(np.concatenate(parts), first)


def test_tables_follow_the_row_map_and_the_dimensions(env):
    """fr_iss_backward keeps its tables with the plan: another row map, or an input of another
    D, on the SAME prefix plan rebuilds them - and going back rebuilds them again."""
    fr, nn, torch = env
    from fruits_amd import _native as nat
    strings = ["[1][2]", "[2]"]          # prefixes [1], [1][2], [2]: EXTENDED emits all, SINGLE two
    plan, rows_ext = nn._prefix_program(fr.ISS(words_of(fr, strings), mode=fr.ISSMode.EXTENDED))
    assert rows_ext.tolist() == [0, 1, 2]
    maps = {"EXTENDED": rows_ext, "SINGLE": np.array([1, 2], dtype=np.int32)}
    for mode, D in (("EXTENDED", 2), ("SINGLE", 2), ("EXTENDED", 3), ("EXTENDED", 2)):
        X = exact_input(strings, 3, D, 130, seed=D)
        G = np.random.default_rng(D).integers(-3, 4, size=(3, len(maps[mode]), 130)).astype(np.float64)
        Xd = torch.tensor(X, device="cuda")
        S = plan.run(Xd, None, layout="KNT")
        got = nat.iss_backward(plan, Xd, S, torch.tensor(G, device="cuda"), maps[mode])
        np.testing.assert_array_equal(got.cpu().numpy(),
                                      gr.iss_grad(X, G, strings, mode).astype(np.float64), err_msg=f"{mode} D={D}")


# ---------------------------------------------------------------- autograd
@pytest.mark.parametrize("string", ["[1][2]", "[11][2]"])
def test_gradcheck(env, string):
    fr, nn, torch = env
    X = torch.from_numpy(np.random.default_rng(11).standard_normal((2, 2, 9))).cuda().requires_grad_(True)
    words = words_of(fr, [string])
    assert torch.autograd.gradcheck(lambda x: nn.iss(x, words), (X,))
    assert torch.autograd.gradcheck(nn.ISSLayer(words, fr.ISSMode.EXTENDED), (X,))


def test_strided_upstream_gradient(env):
    """Y[:, :, -1].sum(): the upstream gradient reaches the backward pass with strides of its
    own (an expanded scalar in a slice of zeros); Y.sum(): all strides 0."""
    fr, nn, torch = env
    strings, N, D, T = ib.WORDS, 3, 3, 700
    X, _ = real_input(strings, N, D, T, seed=1)
    K = len(gr.output_prefixes(strings, "EXTENDED"))
    for pick, G in ((lambda Y: Y[:, :, -1].sum(), np.zeros((N, K, T))), (lambda Y: Y.sum(), np.ones((N, K, T)))):
        if not G.any():
            G[:, :, -1] = 1.0
        Xd = torch.from_numpy(X).cuda().requires_grad_(True)
        pick(nn.iss(Xd, words_of(fr, strings), fr.ISSMode.EXTENDED)).backward()
        hp = gr.iss_grad(X, G, strings, "EXTENDED")
        A = gr.iss_grad(X, G, strings, "EXTENDED", magnitude=True)
        ib.check_bound(Xd.grad.cpu().numpy(), hp, A, gr.n_ops_grad(strings, T, "EXTENDED"), "strided G")


def test_gradients_accumulate_and_none_without_requires_grad(env):
    fr, nn, torch = env
    strings = WORD_SETS["prefix"][1]
    X = exact_input(strings, 3, 2, 65)
    layer = nn.ISSLayer(words_of(fr, strings), fr.ISSMode.EXTENDED)
    Xd = torch.from_numpy(X).cuda().requires_grad_(True)
    G = torch.ones((3, len(gr.output_prefixes(strings, "EXTENDED")), 65), dtype=torch.float64, device="cuda")
    before = nn.backward_calls()
    layer(Xd).backward(G)
    once = Xd.grad.clone()
    layer(Xd).backward(G)
    assert nn.backward_calls() == before + 2
    assert torch.equal(Xd.grad, 2 * once) and once.abs().max() > 0
    # no gradient asked for: no graph, no backward work
    Y = layer(Xd.detach())
    assert not Y.requires_grad and Y.grad_fn is None
    with torch.no_grad():
        assert not layer(Xd).requires_grad
    assert nn.backward_calls() == before + 2
    # only X is kept for the backward pass
    Y = layer(Xd)
    assert [t.data_ptr() for t in Y.grad_fn.saved_tensors] == [Xd.data_ptr()]


def test_layer_copies_and_pickles(env):
    fr, nn, torch = env
    strings = gr.orc.of_weight_strings(2, 2)
    layer = nn.ISSLayer(words_of(fr, strings), fr.ISSMode.EXTENDED)
    X = exact_input(strings, 2, 2, 130)
    G = np.ones((2, len(gr.output_prefixes(strings, "EXTENDED")), 130))
    want, Yw = device_grad(env, X, G, strings, "EXTENDED")
    layer(torch.from_numpy(X).cuda())            # (the original holds device programs by now)
    for dup in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer)), layer.to("cuda"), layer.double()):
        Xd = torch.from_numpy(X).cuda().requires_grad_(True)
        Y = dup(Xd)
        Y.backward(torch.from_numpy(G).cuda())
        np.testing.assert_array_equal(Y.detach().cpu().numpy(), Yw)
        np.testing.assert_array_equal(Xd.grad.cpu().numpy(), want)
