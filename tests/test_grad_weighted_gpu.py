"""GPU tests of the differentiable weighted iterated sums (fruits_amd.nn.weighted_iss,
fr_iss_backward_weighted): the forward bits, the gradient against the long-double oracle of the
adjoint recursion - exactly where every exp factor is 1.0, within the derived rounding bound with
real weights - repeatability, the autograd wiring, a word list whose forward pass splits."""
import copy
import os
import pickle

import numpy as np
import pytest

import iss_bounds as ib
import iss_grad_ref as gr
import iss_grad_weighted_ref as gw

pytestmark = pytest.mark.gpu

# (restated from tests/test_grad_gpu.py: a test module imports none)
CHUNK = 1024       # time steps the scan kernels take at once (csrc/kernels.h, kGradChunk)
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
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


def words_of(fr, strings, alphas=None):
    out = [fr.words.SimpleWord(s) for s in strings]
    for w, a in zip(out, alphas if alphas is not None else []):
        w.alpha = a
    return out


def mode_of(fr, mode):
    return fr.ISSMode.EXTENDED if mode == "EXTENDED" else fr.ISSMode.SINGLE


def weighting_of(spec):
    from fruits_amd.iss import weighting as wt
    kind, kwargs = spec
    return getattr(wt, kind)(**kwargs)


def letters_of(s):
    return len(gr.orc.parse_word(s))


def zero_alphas(strings):
    return [np.zeros(letters_of(s), dtype=np.float32) for s in strings]


def drawn_alphas(strings, seed, pool=12):
    """One alpha per letter and word, drawn from [0.25, 2] as float32.  A plan - the forward pass's
    too - names a staged row with 7 bits (csrc/plan.cpp: "too many staged rows"), which is 63
    distinct alphas at the most, and of_weight(4, 2) has more letters than that: the letters
    draw from ``pool`` values, themselves uniform in [0.25, 2]."""
    rng = np.random.default_rng([seed, len(strings)])
    values = rng.uniform(0.25, 2.0, pool).astype(np.float32)
    return [rng.choice(values, letters_of(s)) for s in strings]


def exact_input(strings, N, D, T, seed=0):
    """Integer-valued X from {-2 ... 2} - zeros included - and from {+-0.5, +-1, +-2} in the
    dimensions some word divides by: every partial sum of the gradient is a dyadic rational far
    below 2^53, so any order of the additions gives the same bits."""
    rng = np.random.default_rng([seed, N, D, T])
    X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    for d in {d for s in strings for row in gr.orc.parse_word(s) for d, e in enumerate(row) if e < 0}:
        X[:, d] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=(N, T))
    return X


def real_input(strings, N, D, T, seed=0):
    """Standard normal X with a few exact zeros in the dimensions no word divides by."""
    rng = np.random.default_rng([seed, N, D, T, 7])
    X = rng.standard_normal((N, D, T))
    divided = {d for s in strings for row in gr.orc.parse_word(s) for d, e in enumerate(row) if e < 0}
    for d in sorted(set(range(D)) - divided):
        X[rng.integers(0, N, 5), d, rng.integers(0, T, 5)] = 0.0
    return X, rng.standard_normal


def device_grad(env, X, G, strings, alphas, mode, spec):
    """X.grad of ``(nn.weighted_iss(X) * G).sum()`` as a host array, the forward result, and the
    lookup the device used."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)       # (copies: the shared cases are read-only)
    op = fr.ISS(words_of(fr, strings, alphas), mode=mode_of(fr, mode), weighting=weighting_of(spec))
    Y = nn.weighted_iss(Xd, op)
    Y.backward(torch.tensor(G, device="cuda"))
    return Xd.grad.cpu().numpy(), Y.detach().cpu().numpy(), op.lookup_device(Xd).cpu().numpy()


# ---------------------------------------------------------------- forward
FORWARD_WEIGHTINGS = {
    "indices": ("Indices", {}),
    "indices_total": ("Indices", {"total": True}),
    "plateaus": ("Plateaus", {"n": 5}),
    "plateaus_total": ("Plateaus", {"n": 5, "total": True}),
}


@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("name", list(FORWARD_WEIGHTINGS))
def test_forward_bits(env, name, mode):
    fr, nn, torch = env
    strings = ib.WORDS + gr.orc.of_weight_strings(2, 3)
    words = words_of(fr, strings, drawn_alphas(strings, 1))
    X = np.random.default_rng(3).standard_normal((5, 3, 300))
    w = weighting_of(FORWARD_WEIGHTINGS[name])
    want = fr.ISS(words, mode=mode_of(fr, mode), weighting=w).transform(X)            # (K, N, T)
    Xd = torch.from_numpy(X).cuda()
    Y = nn.weighted_iss(Xd, words, mode_of(fr, mode), weighting=w)
    assert Y.shape == (5, want.shape[0], 300) and Y.device == Xd.device and not Y.requires_grad
    # a permuted view of the walk's contiguous (K, N, T) buffer, not a copy
    assert not Y.is_contiguous() and Y.permute(1, 0, 2).is_contiguous()
    np.testing.assert_array_equal(Y.cpu().numpy(), want.transpose(1, 0, 2))
    # an input that is not contiguous is made so
    Xt = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).cuda().transpose(1, 2)
    assert not Xt.is_contiguous()
    layer = nn.WeightedISSLayer(words, mode_of(fr, mode), weighting=w)
    np.testing.assert_array_equal(layer(Xt).cpu().numpy(), want.transpose(1, 0, 2))


# ---------------------------------------------------------------- exact
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("name", list(WORD_SETS))
def test_gradient_exact_with_alpha_zero(env, name, T, mode):
    """Every alpha is 0, so exp(+-g * 0) = 1.0 exactly and the gradient is that of the unweighted
    iterated sums, bit for bit: shifts, carries, gathers and both lane maps, whatever the rounding."""
    D, strings = WORD_SETS[name]
    # N in {1, 3, 261}, every one with every word set; the 261 series on the lengths up to 257
    at = LENGTHS.index(T) + list(WORD_SETS).index(name) + (mode == "EXTENDED")
    N = (1, 3, 261)[at % 3] if T <= 257 else (1, 3)[at % 2]
    X = exact_input(strings, N, D, T)
    K = len(gr.output_prefixes(strings, mode))
    G = np.random.default_rng([5, T, K, N]).integers(-3, 4, size=(N, K, T)).astype(np.float64)
    # the same expected array for both bodies, computed once
    want = gr.iss_grad(X, G, strings, mode)
    assert np.abs(want).max() < 2.0 ** 50 and (want == want.astype(np.float64)).all()
    forward = gr.orc.iss_transform(X, strings, mode).transpose(1, 0, 2)
    # both bodies up to T = 257, beyond it one of them, alternating by case
    # (at // 2: N alternates with at % 2 there)
    for total in ((False, True) if T <= 257 else (bool(at // 2 % 2),)):
        got, Y, lookup = device_grad(env, X, G, strings, zero_alphas(strings), mode,
                                     ("Indices", {"total": total}))
        assert T == 1 or lookup.max() == 50.0
        what = f"{name} N={N} T={T} {mode} total={total}"
        np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=what)
        np.testing.assert_array_equal(Y, forward, err_msg=what)


# ---------------------------------------------------------------- the derived bound
OFW42 = gr.orc.of_weight_strings(4, 2)
TWINS = ["[1][2]", "[1][2]", "[11][2][1]", "[11][2][1]", "[2]"]
BOUND_CASES = {
    # (shape, words, mode, weighting)
    "of_weight42_1024": ((7, 3, 1024), OFW42, "EXTENDED", ("Indices", {})),
    "of_weight42_1024_total": ((7, 3, 1024), OFW42, "EXTENDED", ("Indices", {"total": True})),
    "of_weight42_4099": ((3, 2, 4099), OFW42, "EXTENDED", ("Indices", {})),
    "of_weight42_4099_total": ((3, 2, 4099), OFW42, "EXTENDED", ("Indices", {"total": True})),
    "words_1024_single_plateaus": ((7, 3, 1024), ib.WORDS, "SINGLE", ("Plateaus", {"n": 5})),
    # equal words with other alphas: twin nodes all the way down, each an output row
    "twins_300": ((3, 2, 300), TWINS, "SINGLE", ("Indices", {"scale": 3.0})),
    "twins_300_total": ((3, 2, 300), TWINS, "SINGLE", ("Indices", {"scale": 3.0, "total": True})),
}
_REAL = {}


def real_case(name):
    """(X, G, alphas) of a bound case: computed once, shared, never changed."""
    if name not in _REAL:
        (N, D, T), strings, mode, _ = BOUND_CASES[name]
        X, normal = real_input(strings, N, D, T)
        alphas = drawn_alphas(strings, 2)
        G = normal((N, len(gw.output_nodes(strings, alphas, mode)), T))
        for a in [X, G] + alphas:
            a.setflags(write=False)
        _REAL[name] = (X, G, alphas)
    return _REAL[name]


def reference(name, lookup):
    """(hp, A, n) of a bound case on the lookup the device used: once per case."""
    key = (name, "ref")
    if key not in _REAL:
        (N, D, T), strings, mode, spec = BOUND_CASES[name]
        X, G, alphas = real_case(name)
        total = bool(spec[1].get("total", False))
        hp = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, mode)
        A = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, mode, magnitude=True)
        _REAL[key] = (hp, A, gw.n_ops_grad_weighted(strings, alphas, lookup, T, mode))
    return _REAL[key]


def twin_nodes(strings, alphas, mode):
    """Nodes of the trie that share their letters with another node."""
    nodes = gw.trie_nodes(gw.output_nodes(strings, alphas, mode))
    letters = [tuple(el for el, _ in v) for v in nodes]
    return sum(1 for l in letters if letters.count(l) > 1)


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_gradient_within_bound(env, name):
    """|device - iss_grad_weighted| <= 2 n_ops_grad_weighted 2^-53 iss_grad_weighted(magnitude=True),
    elementwise."""
    _, strings, mode, spec = BOUND_CASES[name]
    X, G, alphas = real_case(name)
    assert (X == 0).sum() >= 3
    # prefixes with equal letters and other alphas are nodes of their own
    assert twin_nodes(strings, alphas, mode) >= 2
    assert all(0.25 <= a.min() and a.max() <= 2.0 and a.dtype == np.float32 for a in alphas)
    got, _, lookup = device_grad(env, X, G, strings, alphas, mode, spec)
    hp, A, n = reference(name, lookup)
    worst = ib.check_bound(got, hp, A, n, f"grad_weighted {name}", family="grad_weighted")
    print(f"grad_weighted {name}: n_ops_grad_weighted = {n}, largest err / bound = {worst:.3g}")


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_native_entry_with_a_lookup_per_series(env, total):
    """_native.iss_backward_weighted with an N-row lookup, g uniform in [0, 5] and another for
    every series: within the bound."""
    fr, nn, torch = env
    from fruits_amd import _native as nat
    from fruits_amd.iss.weighting import Indices
    N, D, T = 3, 2, 300
    strings, mode = gr.orc.of_weight_strings(3, 2), "EXTENDED"
    alphas = drawn_alphas(strings, 4)
    X, normal = real_input(strings, N, D, T, seed=2)
    G = normal((N, len(gw.output_nodes(strings, alphas, mode)), T))
    lookup = np.random.default_rng(9).uniform(0.0, 5.0, size=(N, T))
    assert not np.array_equal(lookup[0], lookup[1])
    op = fr.ISS(words_of(fr, strings, alphas), mode=mode_of(fr, mode), weighting=Indices(total=total))
    plan, row_prefix = nn._weighted_prefix_program(op)
    got = nat.iss_backward_weighted(plan, torch.tensor(X, device="cuda"), torch.tensor(lookup, device="cuda"),
                                    torch.tensor(G, device="cuda"), row_prefix).cpu().numpy()
    hp = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, mode)
    A = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, mode, magnitude=True)
    n = gw.n_ops_grad_weighted(strings, alphas, lookup, T, mode)
    worst = ib.check_bound(got, hp, A, n, f"native N-row lookup total={total}", family="grad_weighted")
    print(f"grad_weighted native total={total}: n_ops_grad_weighted = {n}, largest err / bound = {worst:.3g}")
    # the rows are the series': with the lookup of series 0 for all, series 1 is elsewhere
    one = nat.iss_backward_weighted(plan, torch.tensor(X, device="cuda"),
                                    torch.tensor(lookup[:1].copy(), device="cuda"),
                                    torch.tensor(G, device="cuda"), row_prefix).cpu().numpy()
    np.testing.assert_array_equal(one[0], got[0])
    assert ib.violates(one[1:], hp[1:], A[1:], n)


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("name", ["of_weight42_1024", "of_weight42_1024_total"])
def test_backward_is_repeatable(env, name):
    _, strings, mode, spec = BOUND_CASES[name]
    X, G, alphas = real_case(name)
    first, _, _ = device_grad(env, X, G, strings, alphas, mode, spec)
    again, _, _ = device_grad(env, X, G, strings, alphas, mode, spec)
    np.testing.assert_array_equal(first, again)
    # the batch in two launches of 3 and 4 series: another grid, the same bits
    parts = [device_grad(env, np.ascontiguousarray(X[s]), np.ascontiguousarray(G[s]), strings, alphas,
                         mode, spec)[0] for s in (slice(0, 3), slice(3, 7))]
    np.testing.assert_array_equal(np.concatenate(parts), first)


def test_tables_follow_the_row_map_and_the_dimensions(env):
    """fr_iss_backward_weighted keeps its tables with the plan: another row map, or an input of
    another D, on the SAME prefix plan rebuilds them - and going back rebuilds them again."""
    fr, nn, torch = env
    from fruits_amd import _native as nat
    from fruits_amd.iss.weighting import Indices
    strings = ["[1][2]", "[2]"]          # prefixes [1], [1][2], [2]: EXTENDED emits all, SINGLE two
    for total in (False, True):
        op = fr.ISS(words_of(fr, strings, zero_alphas(strings)), mode=fr.ISSMode.EXTENDED,
                    weighting=Indices(total=total))
        plan, rows_ext = nn._weighted_prefix_program(op)
        assert rows_ext.tolist() == [0, 1, 2]
        maps = {"EXTENDED": rows_ext, "SINGLE": np.array([1, 2], dtype=np.int32)}
        for mode, D in (("EXTENDED", 2), ("SINGLE", 2), ("EXTENDED", 3), ("EXTENDED", 2)):
            X = exact_input(strings, 3, D, 130, seed=D)
            G = np.random.default_rng(D).integers(-3, 4, size=(3, len(maps[mode]), 130)).astype(np.float64)
            Xd = torch.tensor(X, device="cuda")
            got = nat.iss_backward_weighted(plan, Xd, op.lookup_device(Xd), torch.tensor(G, device="cuda"),
                                            maps[mode])
            np.testing.assert_array_equal(got.cpu().numpy(), gr.iss_grad(X, G, strings, mode).astype(np.float64),
                                          err_msg=f"{mode} D={D} total={total}")


# ---------------------------------------------------------------- autograd
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("string, alpha", [("[1][2]", [0.5, 1.5]), ("[11][2][1]", [1.25, 0.25, 2.0])])
def test_gradcheck(env, string, alpha, total):
    fr, nn, torch = env
    from fruits_amd.iss.weighting import Indices
    X = torch.from_numpy(np.random.default_rng(11).standard_normal((2, 2, 9))).cuda().requires_grad_(True)
    words = words_of(fr, [string], [alpha])
    w = Indices(scale=2, total=total)
    assert torch.autograd.gradcheck(lambda x: nn.weighted_iss(x, words, weighting=w), (X,))
    assert torch.autograd.gradcheck(nn.WeightedISSLayer(words, fr.ISSMode.EXTENDED, weighting=w), (X,))


def test_strided_upstream_gradient(env):
    """Y[:, :, -1].sum(): the upstream gradient reaches the backward pass with strides of its
    own (an expanded scalar in a slice of zeros); Y.sum(): all strides 0."""
    fr, nn, torch = env
    from fruits_amd.iss.weighting import Indices
    strings, N, D, T = ib.WORDS, 3, 3, 700
    alphas = drawn_alphas(strings, 6)
    X, _ = real_input(strings, N, D, T, seed=1)
    K = len(gw.output_nodes(strings, alphas, "EXTENDED"))
    for total in (False, True):
        for pick, G in ((lambda Y: Y[:, :, -1].sum(), np.zeros((N, K, T))), (lambda Y: Y.sum(), np.ones((N, K, T)))):
            if not G.any():
                G[:, :, -1] = 1.0
            op = fr.ISS(words_of(fr, strings, alphas), mode=fr.ISSMode.EXTENDED,
                        weighting=Indices(scale=4.0, total=total))
            Xd = torch.from_numpy(X).cuda().requires_grad_(True)
            pick(nn.weighted_iss(Xd, op)).backward()
            lookup = op.lookup_device(Xd).cpu().numpy()
            hp = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, "EXTENDED")
            A = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, "EXTENDED", magnitude=True)
            ib.check_bound(Xd.grad.cpu().numpy(), hp, A,
                           gw.n_ops_grad_weighted(strings, alphas, lookup, T, "EXTENDED"), "strided G")


def test_gradients_accumulate_and_none_without_requires_grad(env):
    fr, nn, torch = env
    from fruits_amd.iss.weighting import Plateaus
    strings = WORD_SETS["prefix"][1]
    X = exact_input(strings, 3, 2, 65)
    layer = nn.WeightedISSLayer(words_of(fr, strings), fr.ISSMode.EXTENDED, weighting=Plateaus(5, scale=2.0))
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
    from fruits_amd.iss.weighting import Indices
    strings = gr.orc.of_weight_strings(2, 2)
    alphas = drawn_alphas(strings, 8)
    spec = ("Indices", {"scale": 3.0, "total": True})
    layer = nn.WeightedISSLayer(words_of(fr, strings, alphas), fr.ISSMode.EXTENDED, weighting=weighting_of(spec))
    X, _ = real_input(strings, 2, 2, 130)
    G = np.ones((2, len(gw.output_nodes(strings, alphas, "EXTENDED")), 130))
    want, Yw, _ = device_grad(env, X, G, strings, alphas, "EXTENDED", spec)
    layer(torch.from_numpy(X).cuda())            # (the original holds device programs by now)
    for dup in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer)), layer.to("cuda"), layer.double()):
        Xd = torch.from_numpy(X).cuda().requires_grad_(True)
        Y = dup(Xd)
        Y.backward(torch.from_numpy(G).cuda())
        np.testing.assert_array_equal(Y.detach().cpu().numpy(), Yw)
        np.testing.assert_array_equal(Xd.grad.cpu().numpy(), want)


# ---------------------------------------------------------------- a forward pass in halves
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_split_forward_one_backward(env, total):
    """More distinct alphas than a workgroup stages exp tables for: the forward pass runs the word
    list in halves, the backward pass - which reads its tables from global memory - is one call."""
    fr, nn, torch = env
    from fruits_amd.iss.weighting import Indices
    N, D, T = 3, 2, 600
    strings, mode = gr.orc.of_weight_strings(2, 2), "SINGLE"
    letters = sum(letters_of(s) for s in strings)
    grid = np.linspace(0.25, 2.0, letters).astype(np.float32)      # every letter an alpha of its own
    alphas, at = [], 0
    for s in strings:
        alphas.append(grid[at:at + letters_of(s)])
        at += letters_of(s)
    op = fr.ISS(words_of(fr, strings, alphas), mode=mode_of(fr, mode), weighting=Indices(scale=3.0, total=total))
    assert not op._plan(0, len(op.words)).fits(T)
    assert not nn._weighted_prefix_program(op)[0].fits(T)
    X, normal = real_input(strings, N, D, T, seed=3)
    G = normal((N, len(strings), T))
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    before = nn.backward_calls()
    Y = nn.weighted_iss(Xd, op)
    np.testing.assert_array_equal(Y.detach().cpu().numpy(), op.transform(X).transpose(1, 0, 2))
    Y.backward(torch.tensor(G, device="cuda"))
    assert nn.backward_calls() == before + 1
    lookup = op.lookup_device(Xd).cpu().numpy()
    hp = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, mode)
    A = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, mode, magnitude=True)
    ib.check_bound(Xd.grad.cpu().numpy(), hp, A, gw.n_ops_grad_weighted(strings, alphas, lookup, T, mode),
                   f"split forward total={total}", family="grad_weighted")


# ---------------------------------------------------------------- the old entries are unmoved
def test_entries_keep_to_their_plans(env):
    fr, nn, torch = env
    from fruits_amd import _native as nat
    from fruits_amd.iss.weighting import Indices
    strings = ["[1][2]", "[2]"]
    X = torch.tensor(exact_input(strings, 2, 2, 40), device="cuda")
    weighted_op = fr.ISS(words_of(fr, strings), weighting=Indices())
    wplan, wrows = nn._weighted_prefix_program(weighted_op)
    plan, rows = nn._prefix_program(fr.ISS(words_of(fr, strings)))
    G = torch.ones((2, 2, 40), dtype=torch.float64, device="cuda")
    S = torch.zeros((wplan.rows, 2, 40), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="fr_iss_backward: the plan is not an unweighted Reals trie plan"):
        nat.iss_backward(wplan, X, S, G, wrows)
    with pytest.raises(ValueError, match="fr_iss_backward_max: the plan is a Reals plan"):
        nat.iss_backward_max(wplan, X, S, G, wrows)
    with pytest.raises(ValueError, match="fr_iss_backward_weighted: the plan is an unweighted Reals plan - "
                                              "its backward pass is fr_iss_backward"):
        nat.iss_backward_weighted(plan, X, weighted_op.lookup_device(X), G, rows)


# ---------------------------------------------------------------- the weighted paths keep their bits
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_weighted_backward_keeps_its_bits(env, total):
    """The weighted adjoints share their scans, their gather and their input kernel with the
    others: the gradient on a real-valued two-chunk case with real weights is, bit for bit, what
    the library computed before they were shared
    (tests/golden/grad_weighted_[non]total_before_shared_frame.npz, written on an MI355X by
    tools/grad_golden.py on the commit before).  The gradient is dense."""
    name = f"grad_weighted_{'total' if total else 'nontotal'}_before_shared_frame.npz"
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    N, D, T = 3, 3, CHUNK + 6
    strings = ["[1][2][3]", "[11][2]", "[1][-2]", "[12][2][3][1]"]     # (WORDS of tests/test_grad_max_gpu.py)
    alphas = drawn_alphas(strings, seed=12)
    rng = np.random.default_rng(12)
    X = rng.standard_normal((N, D, T))
    G = rng.standard_normal((N, len(gw.output_nodes(strings, alphas, "EXTENDED")), T))
    got, _, _ = device_grad(env, X, G, strings, alphas, "EXTENDED", ("Indices", {"total": total}))
    assert gold["dX"].shape == (N, D, T) and (gold["dX"] != 0).sum() > 9000
    np.testing.assert_array_equal(got, gold["dX"])
