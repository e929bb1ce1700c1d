"""GPU tests of per-series lengths in the differentiable iterated sums (fruits_amd.nn with
``lengths=``, fr_plan_set_grad_lengths).  The expected values are the existing
oracles of the five adjoints run series by series on the TRUNCATED series (ragged_grad_ref):
bit for bit on inputs where all arithmetic is exact, within the derived bound of the kind
evaluated at L_n on real-valued ones; +0.0 behind every series; nothing of a tail - of X or of the
upstream gradient - reaches a result; the features of the truncated rows; repeatability; the
stream order."""
import ctypes as C

import numpy as np
import pytest

import features_grad_ref as fg
import iss_bounds as ib
import iss_grad_ref as gr
import ragged_grad_ref as rr
import stream_order as so

pytestmark = pytest.mark.gpu

# (restated from tests/test_grad_gpu.py: a test module imports none)
WORD_SETS = {
    "of_weight32": (2, gr.orc.of_weight_strings(3, 2)),
    "of_weight32_D3": (3, gr.orc.of_weight_strings(3, 2)),       # a dimension no word names
    "prefix": (2, ["[1]", "[1][2]", "[1][2][1]", "[2]", "[1][2]"]),      # two rows on one node
    "fanout": (3, ["[1][1]", "[1][2]", "[1][3]", "[1][12]", "[3]"]),
    "square": (2, ["[11][2]"]),
    "division": (2, ["[1][-2]"]),
    "one_letter": (1, ["[1]"]),
}
MODES = ("SINGLE", "EXTENDED")
# padded T = two chunks + 3, every class of length twice: N = 34
T_CHUNKS = 2 * rr.CHUNK + 3
L_CHUNKS = rr.deal(rr.CLASSES, 2, seed=11)
# more workgroups than one round of the device: N = 261 series of 1 ... 257 steps
T_ROUND = 257
L_ROUND = rr.deal(tuple(range(1, T_ROUND + 1)) + (1, 64, 256, 257), 1, seed=12)
assert L_CHUNKS.shape == (34,) and L_CHUNKS.max() == T_CHUNKS and L_ROUND.shape == (261,)


@pytest.fixture(scope="module")
def env():
    import torch
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    nat.require_device()
    yield fr, nn, torch
    ib.print_ratios()


def letters_of(s):
    return len(gr.orc.parse_word(s))


def zero_alphas(strings):
    return [np.zeros(letters_of(s), dtype=np.float32) for s in strings]


def drawn_alphas(strings, seed, pool=12):
    """One alpha per letter and word from a pool of float32 values in [0.25, 2] (the draw of
    tests/test_grad_weighted_gpu.py)."""
    rng = np.random.default_rng([seed, len(strings)])
    values = rng.uniform(0.25, 2.0, pool).astype(np.float32)
    return [rng.choice(values, letters_of(s)) for s in strings]


def layer_of(env, kind, strings, mode, alphas=None):
    """(layer, row): the layer of ``kind`` and, weighted, the row of a series of L steps."""
    fr, nn, torch = env
    from fruits_amd.iss.weighting import Indices
    words = [fr.words.SimpleWord(s) for s in strings]
    m = fr.ISSMode.EXTENDED if mode == "EXTENDED" else fr.ISSMode.SINGLE
    if kind == "reals":
        return nn.ISSLayer(words, m), None
    if kind in ("arctic", "bayesian"):
        return nn.MaxISSLayer(words, m, semiring=getattr(fr.semiring, kind.capitalize())()), None
    for w, a in zip(words, alphas):
        w.alpha = a
    weighting = Indices(total=kind == "total")
    return nn.WeightedISSLayer(words, m, weighting=weighting), weighting._row


def divided(strings):
    return {d for s in strings for row in gr.orc.parse_word(s) for d, e in enumerate(row) if e < 0}


def exact_input(kind, strings, N, D, T, seed=0):
    """(N, D, T) on which every sum and product of both passes is exact (the inputs of
    tests/test_grad_gpu.py and tests/test_grad_max_gpu.py): small integers, zeros included, and
    {+-0.5, +-1, +-2} where a word divides; Arctic: two of three series on staircases - heads and
    ties all along; Bayesian: powers of two."""
    rng = np.random.default_rng([seed, N, D, T])
    if kind == "bayesian":
        return 2.0 ** rng.integers(-2, 2, size=(N, D, T)).astype(np.float64)
    X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    if kind == "arctic":
        X[1::3] += np.arange(T) // 5
        X[2::3] -= np.arange(T) // 5
        return X
    for d in divided(strings):
        X[:, d] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=(N, T))
    return X


def real_input(kind, strings, N, D, T, seed=0):
    """Real-valued X: standard normal with a few exact zeros where no word divides (Reals), with a
    rising trend (Arctic: heads all along), uniform in [0.25, 1] (Bayesian)."""
    rng = np.random.default_rng([seed, N, D, T, 7])
    if kind == "bayesian":
        return 0.25 + 0.75 * rng.random((N, D, T))
    X = rng.standard_normal((N, D, T))
    if kind == "arctic":
        return X + 0.02 * np.arange(T)
    for d in sorted(set(range(D)) - divided(strings)):
        X[rng.integers(0, N, 5), d, rng.integers(0, T, 5)] = 0.0
    return X


def tail_mask(lengths, T):
    """(N, 1, T): True behind a series' end."""
    return (np.arange(T)[np.newaxis, :] >= np.asarray(lengths)[:, np.newaxis])[:, np.newaxis, :]


def device_grad(env, layer, X, G, lengths):
    """X.grad of ``(layer(X, lengths) * G).sum()`` and the forward result, as host arrays."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    Y = layer(Xd, lengths=lengths)
    Y.backward(torch.tensor(G, device="cuda"))
    return Xd.grad.cpu().numpy(), Y.detach().cpu().numpy()


def truncated_rows(env, layer, X, lengths):
    """Per series the DENSE call on the truncated series: a list of (K, L_n) host arrays."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda")
    return [layer(Xd[n:n + 1, :, :int(L)].contiguous())[0].cpu().numpy() for n, L in enumerate(lengths)]


def assert_valid_rows_equal(Y, rows, lengths, what):
    for n, L in enumerate(int(v) for v in lengths):
        np.testing.assert_array_equal(Y[n, :, :L], rows[n], err_msg=f"{what}: forward rows of series {n} (L = {L})")


# ---------------------------------------------------------------- exact
def exact_case(env, kind, name, mode, T, lengths):
    D, strings = WORD_SETS[name]
    N = lengths.shape[0]
    X = exact_input(kind, strings, N, D, T)
    K = len(gr.output_prefixes(strings, mode))
    G = np.random.default_rng([5, T, K, N]).integers(-3, 4, size=(N, K, T)).astype(np.float64)
    G[np.broadcast_to(tail_mask(lengths, T), G.shape)] = np.nan       # (never read)
    layer, _ = layer_of(env, kind, strings, mode, zero_alphas(strings))
    got, Y = device_grad(env, layer, X, G, lengths)
    # every alpha is 0: exp(+-g * 0) = 1.0 exactly, the weighted gradient is the unweighted one
    want = rr.grad("reals" if kind in ("nontotal", "total") else kind, X, G, lengths, strings, mode)
    assert np.abs(want).max() < 2.0 ** 50 and (want == want.astype(np.float64)).all()
    what = f"{kind} {name} {mode} T={T} N={N}"
    tail = np.broadcast_to(tail_mask(lengths, T), got.shape)
    for n in np.flatnonzero((got != want.astype(np.float64)).any(axis=(1, 2))):
        raise AssertionError(f"{what}: series {n} (L = {lengths[n]}) differs from the truncated oracle")
    assert not got[tail].any() and not np.signbit(got[tail]).any(), f"{what}: the tail of X.grad is not +0.0"
    assert np.abs(want).max() > 0
    assert_valid_rows_equal(Y, truncated_rows(env, layer, X, lengths), lengths, what)
    assert np.isfinite(Y).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(WORD_SETS))
@pytest.mark.parametrize("kind", rr.KINDS)
def test_gradient_exact(env, kind, name, mode):
    """Padded T = 2051, every class of length twice (N = 34): X.grad[n, :, :L_n] is the oracle on
    the truncated series bit for bit, the tail +0.0, the forward rows the dense call's."""
    exact_case(env, kind, name, mode, T_CHUNKS, L_CHUNKS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["prefix", "fanout"])
@pytest.mark.parametrize("kind", rr.KINDS)
def test_gradient_exact_many_series(env, kind, name, mode):
    """N = 261 series of 1 ... 257 steps in T = 257: more workgroups than one round."""
    exact_case(env, kind, name, mode, T_ROUND, L_ROUND)


# ---------------------------------------------------------------- the derived bound
MAX_WORDS = ["[1][2][3]", "[11][2]", "[1][-2]", "[12][2][3][1]"]      # tests/test_grad_max_gpu.py
BOUND_WORDS = {"reals": ib.WORDS, "nontotal": ib.WORDS, "total": ib.WORDS, "arctic": MAX_WORDS,
               "bayesian": MAX_WORDS}


@pytest.mark.parametrize("kind", rr.KINDS)
def test_gradient_within_bound(env, kind):
    """|device - oracle| <= 2 n_ops 2^-53 magnitude elementwise, per series: n_ops_grad,
    n_ops_grad_weighted, n_ops_grad_max and the magnitude run as they exist, evaluated on the
    truncated series at L_n.  No measured error enters."""
    fr, nn, torch = env
    strings, mode, T, lengths, D = BOUND_WORDS[kind], "EXTENDED", T_CHUNKS, L_CHUNKS, 3
    N = lengths.shape[0]
    X = real_input(kind, strings, N, D, T)
    alphas = drawn_alphas(strings, 2)
    rng = np.random.default_rng([9, N, T])
    layer, row = layer_of(env, kind, strings, mode, alphas)
    K = layer(torch.tensor(X[:1, :, :4], device="cuda")).shape[1]
    G = rng.standard_normal((N, K, T))
    got, Y = device_grad(env, layer, X, G, lengths)
    assert np.isfinite(got).all()
    tail = np.broadcast_to(tail_mask(lengths, T), got.shape)
    assert not got[tail].any() and not np.signbit(got[tail]).any()
    worst = 0.0
    for n, L in enumerate(int(v) for v in lengths):
        Xn, Gn = rr.truncated(X, n, L), rr.truncated(G, n, L)
        lookup = None if row is None else np.asarray(row(L), dtype=np.float64)[np.newaxis, :]
        if kind in ("arctic", "bayesian"):
            # the precondition for shared heads: the forward bits are the oracle's
            rows = gr.orc.iss_transform(Xn, strings, mode, semiring=kind.capitalize())
            np.testing.assert_array_equal(Y[n, :, :L], rows[:, 0])
        hp = rr.series_grad(kind, Xn, Gn, strings, mode, alphas, lookup)
        A = rr.series_grad(kind, Xn, Gn, strings, mode, alphas, lookup, magnitude=True)
        ops = rr.n_ops(kind, strings, L, mode, alphas, lookup)
        worst = max(worst, ib.check_bound(got[n:n + 1, :, :L], hp, A, ops, f"ragged grad {kind} series {n} L={L}",
                                          family=f"grad_ragged_{kind}"))
    print(f"ragged grad {kind}: largest err / bound over {N} series = {worst:.3g}")


# ---------------------------------------------------------------- tails
@pytest.mark.parametrize("tail", ["finite", "huge"])
@pytest.mark.parametrize("kind", rr.KINDS)
def test_tails_influence_nothing(env, kind, tail):
    """The tail of X replaced by other finite values / by alternating +-1e160, the tail of the
    upstream gradient by NaN: no bit of X.grad or of the valid rows changes, X.grad is finite."""
    D, strings = WORD_SETS["prefix"]
    T, lengths, mode = T_CHUNKS, L_CHUNKS, "EXTENDED"
    N = lengths.shape[0]
    X = real_input(kind, strings, N, D, T, seed=3)
    layer, _ = layer_of(env, kind, strings, mode, drawn_alphas(strings, 4))
    K = len(gr.output_prefixes(strings, mode))
    rng = np.random.default_rng([13, N, T])
    G = rng.standard_normal((N, K, T))
    base, Y = device_grad(env, layer, X, G, lengths)
    assert np.isfinite(base).all() and np.abs(base).max() > 0
    X2, G2 = X.copy(), G.copy()
    other = (rng.standard_normal(X.shape) * 3.0 if tail == "finite"
             else np.broadcast_to(1e160 * (-1.0) ** np.arange(T), X.shape))
    if kind == "bayesian" and tail == "finite":
        other = 0.25 + 0.75 * rng.random(X.shape)
    at = np.broadcast_to(tail_mask(lengths, T), X.shape)
    X2[at] = other[at]
    G2[np.broadcast_to(tail_mask(lengths, T), G.shape)] = np.nan
    assert np.isfinite(X2).all() and not np.array_equal(X2, X)
    got, Y2 = device_grad(env, layer, X2, G2, lengths)
    np.testing.assert_array_equal(got, base)
    assert np.isfinite(got).all() and not np.signbit(got[at]).any() and not got[at].any()
    for n, L in enumerate(int(v) for v in lengths):
        np.testing.assert_array_equal(Y2[n, :, :L], Y[n, :, :L], err_msg=f"series {n}")


# ---------------------------------------------------------------- features
def feature_heads(fr):
    sv = fr.sieving
    return [sv.END([-1]), sv.END([2]), sv.MAX([2, -1]), sv.MIN([-1])]


L_FEATURES = rr.deal(rr.CLASSES[1:], 2, seed=14)       # lengths >= 2: END([2]) needs two steps


@pytest.mark.parametrize("form", ["layer", "functional"])
@pytest.mark.parametrize("kind", rr.KINDS)
def test_features(env, kind, form):
    """Values and positions are ``pick`` on the truncated oracle rows, every position < L_n;
    X.grad is the dense entry armed with the same lengths on ``dense_upstream``, bit for bit."""
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    T, lengths, mode = T_CHUNKS, L_FEATURES, "EXTENDED"
    N = lengths.shape[0]
    X = exact_input(kind, strings, N, D, T, seed=2)
    layer, _ = layer_of(env, kind, strings, mode, zero_alphas(strings))
    heads = feature_heads(fr)
    F = fg.nfeatures(heads)
    if form == "layer":
        head = nn.FeatureLayer(layer.op, sieves=heads)
        forward = lambda x: head(x, lengths=torch.from_numpy(lengths).cuda())      # noqa: E731 (a device tensor)
    else:
        forward = lambda x: nn.iss_features_ragged(x, lengths, layer.op, sieves=heads)      # noqa: E731
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    feats = forward(Xd)
    K = feats.shape[1] // F
    pos = feats.grad_fn.saved_tensors[1].cpu().numpy()
    assert pos.shape == (N, K, F) and pos.dtype == np.int32
    saved = feats.grad_fn.saved_tensors
    assert len(saved) == 3 and saved[2].dtype == torch.int32 and saved[2].cpu().tolist() == lengths.tolist()
    semiring = kind.capitalize() if kind in ("arctic", "bayesian") else "Reals"
    ties = empty = shared = 0
    for n, L in enumerate(int(v) for v in lengths):
        rows = gr.orc.iss_transform(rr.truncated(X, n, L), strings, mode, semiring=semiring).transpose(1, 0, 2)
        want_f, want_p = fg.pick(rows, heads)
        np.testing.assert_array_equal(feats[n].detach().cpu().numpy().reshape(K, F), want_f[0], err_msg=f"series {n}")
        np.testing.assert_array_equal(pos[n], want_p[0], err_msg=f"positions of series {n} (L = {L})")
        assert (pos[n] < L).all()
        ties += int((fg.attained(rows, heads) > 1).sum())
        empty += int((want_p < 0).sum())
        shared += sum(len(set(p[p >= 0].tolist())) < int((p >= 0).sum()) for p in want_p[0])
    # ties, an empty band, two features on one element - from the reference
    assert ties > 0 and empty > 0 and shared > 0
    g = np.random.default_rng([15, N]).integers(-3, 4, size=(N, K * F)).astype(np.float64)
    feats.backward(torch.tensor(g, device="cuda"))
    want, _ = device_grad(env, layer, X, fg.dense_upstream(pos, g, T), lengths)
    np.testing.assert_array_equal(Xd.grad.cpu().numpy(), want)
    at = np.broadcast_to(tail_mask(lengths, T), want.shape)
    got = Xd.grad.cpu().numpy()
    assert not got[at].any() and not np.signbit(got[at]).any() and np.abs(got).max() > 0


def test_features_keep_features_positions_and_lengths_alone(env):
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    T, lengths = T_CHUNKS, L_FEATURES
    N = lengths.shape[0]
    layer, _ = layer_of(env, "reals", strings, "EXTENDED")
    head = nn.FeatureLayer(layer.op, sieves=feature_heads(fr))
    Xd = torch.tensor(exact_input("reals", strings, N, D, T, seed=2), device="cuda").requires_grad_(True)
    head(Xd, lengths=lengths)          # (plans and tables: they exist from here on)

    def allocated():
        # (a block that another stream used - an upload - is handed back once its events are seen)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.memory_allocated()
    before = allocated()
    feats = head(Xd, lengths=lengths)
    grown = allocated() - before
    block = lambda nbytes: -(-nbytes // 512) * 512      # noqa: E731 (the allocator's granularity)
    K, F = feats.shape[1] // head.head.F, head.head.F
    assert grown == block(8 * N * K * F) + block(4 * N * K * F) + block(4 * N), (grown, N, K, F)


def test_end_cut_outside_a_series_raises_before_any_launch(env):
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    layer, _ = layer_of(env, "reals", strings, "EXTENDED")
    head = nn.FeatureLayer(layer.op, sieves=[fr.sieving.END([3])])
    Xd = torch.zeros((3, D, 9), dtype=torch.float64, device="cuda")
    before = nn.backward_calls()
    with pytest.raises(IndexError, match="index 2 is out of bounds for axis 1 with size 2"):
        head(Xd, lengths=np.array([5, 2, 9]))
    with pytest.raises(ValueError, match="1..9"):
        head(Xd, lengths=np.array([5, 2, 10]))
    with pytest.raises(TypeError, match="array of integers"):
        layer(Xd, lengths=torch.tensor([5.0, 2.0, 9.0], device="cuda"))
    assert nn.backward_calls() == before


# ---------------------------------------------------------------- repeatability
@pytest.fixture
def setter_calls(monkeypatch):
    """How often fr_plan_set_grad_lengths was called with a table (not to clear)."""
    from fruits_amd import _native as nat
    L, armed = nat.lib(), []
    real = L.fr_plan_set_grad_lengths

    def spy(plan, table, n):
        if getattr(table, "value", table):
            armed.append(int(getattr(n, "value", n)))
        return real(plan, table, n)
    monkeypatch.setattr(L, "fr_plan_set_grad_lengths", spy)
    return armed


@pytest.mark.parametrize("kind", rr.KINDS)
def test_repeatable_and_split(env, kind, setter_calls):
    D, strings = WORD_SETS["fanout"]
    T, lengths, mode = T_CHUNKS, L_CHUNKS, "EXTENDED"
    N = lengths.shape[0]
    X = real_input(kind, strings, N, D, T, seed=5)
    layer, _ = layer_of(env, kind, strings, mode, drawn_alphas(strings, 6))
    G = np.random.default_rng([17, N, T]).standard_normal((N, len(gr.output_prefixes(strings, mode)), T))
    first, Y = device_grad(env, layer, X, G, lengths)
    again, Y2 = device_grad(env, layer, X, G, lengths)
    np.testing.assert_array_equal(first, again)
    np.testing.assert_array_equal(Y, Y2)
    assert setter_calls == [N, N]
    # the batch in two launches of 15 and 19 series: another grid, the same bits
    parts = [device_grad(env, layer, np.ascontiguousarray(X[s]), np.ascontiguousarray(G[s]), lengths[s])[0]
             for s in (slice(0, 15), slice(15, N))]
    np.testing.assert_array_equal(np.concatenate(parts), first)


@pytest.mark.parametrize("kind", rr.KINDS)
def test_all_equal_lengths_take_the_dense_path(env, kind, setter_calls):
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    N, T, mode = 5, rr.CHUNK + 1, "EXTENDED"
    X = real_input(kind, strings, N, D, T, seed=7)
    layer, _ = layer_of(env, kind, strings, mode, drawn_alphas(strings, 8))
    G = np.random.default_rng([19, N, T]).standard_normal((N, len(gr.output_prefixes(strings, mode)), T))
    before = nn.backward_calls()
    dense, Yd = device_grad(env, layer, X, G, None)
    full, Yf = device_grad(env, layer, X, G, np.full(N, T))
    tensor, _ = device_grad(env, layer, X, G, torch.full((N,), T, dtype=torch.int32, device="cuda"))
    assert nn.backward_calls() == before + 3 and setter_calls == []
    np.testing.assert_array_equal(full, dense)
    np.testing.assert_array_equal(tensor, dense)
    np.testing.assert_array_equal(Yf, Yd)
    # one shorter series arms the plan - and leaves the others' bits alone
    lengths = np.full(N, T)
    lengths[2] = T - 1
    ragged, _ = device_grad(env, layer, X, G, lengths)
    assert setter_calls == [N]
    keep = np.arange(N) != 2
    np.testing.assert_array_equal(ragged[keep], dense[keep])
    assert not ragged[2, :, T - 1].any() and np.abs(ragged[2]).max() > 0
    # only X and the lengths are kept for the backward pass of a ragged batch, X alone otherwise
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    Y = layer(Xd, lengths=np.full(N, T))
    assert [t.data_ptr() for t in Y.grad_fn.saved_tensors] == [Xd.data_ptr()]
    Y = layer(Xd, lengths=lengths)
    saved = Y.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == Xd.data_ptr() and saved[1].dtype == torch.int32


# ---------------------------------------------------------------- stream order
S_N, S_T = 9, 1100
S_LENGTHS = np.array([1100, 1, 1024, 700, 1025, 63, 1099, 257, 5], dtype=np.int64)
S_WORDS = ["[1]", "[1][2]", "[12][3]", "[1][2][3]"]


def draw(seed, kind, shape):
    """Finite random values: seed 1 the true input, 2 the wrong one, 3 and 4 further ones."""
    rng = np.random.default_rng([2029, seed, shape[-1]])
    return 0.25 + 0.75 * rng.random(shape) if kind == "bayesian" else rng.standard_normal(shape)


@pytest.mark.parametrize("kind", rr.KINDS + ("features",))
def test_ragged_backward_behind_a_producer(env, kind, record_property):
    """Forward under the side stream on an ``X`` that is still being produced, ``backward()`` from
    the default-stream context (tests/test_streams_gpu.py::test_backward): the lengths, the
    per-series lookup and cut tables reach the device in stream order."""
    fr, nn, torch = env
    layer, _ = layer_of(env, "reals" if kind == "features" else kind, S_WORDS, "EXTENDED", drawn_alphas(S_WORDS, 10))
    if kind == "features":
        head = nn.FeatureLayer(layer.op, sieves=[fr.sieving.END([S_T // 2, -1]), fr.sieving.MAX([-1], (-1, 0, 1))])
        lengths = np.maximum(S_LENGTHS, S_T // 2)
        forward = lambda x: head(x, lengths=lengths)      # noqa: E731
    else:
        forward = lambda x: layer(x, lengths=S_LENGTHS)      # noqa: E731
    shape_x = (S_N, 3, S_T)
    X = draw(1, kind, shape_x)
    shape_g = tuple(forward(torch.from_numpy(X).cuda()).shape)
    # (the rows behind a series' end are unspecified: not compared.  The mask is on the device
    # before the producer starts - an upload inside the call would wait for it)
    behind = torch.from_numpy(tail_mask(S_LENGTHS, S_T)).cuda()
    torch.cuda.synchronize()

    def call(xb, gb):
        x = xb.detach().requires_grad_(True)
        y = forward(x)
        side = torch.cuda.current_stream()
        with torch.cuda.stream(torch.cuda.default_stream()):
            y.backward(gb)
        side.wait_stream(torch.cuda.default_stream())
        valid = y.detach() if kind == "features" else torch.where(behind, torch.zeros_like(y.detach()), y.detach())
        return valid, x.grad
    _, report = so.behind_producer(call, [X, draw(3, "normal", shape_g)],
                                   [draw(2, kind, shape_x), draw(4, "normal", shape_g)],
                                   what=f"nn ragged {kind} forward + backward")
    so.note(record_property, report)


def test_grad_lengths_replaced_in_flight(env, record_property):
    """fr_plan_set_grad_lengths: old lengths queued, new lengths set from the host before the
    queue drains - the queued pass keeps the old ones (the entry read the pointer once and handed
    it to its kernels by value)."""
    fr, nn, torch = env
    from fruits_amd import _native as nat
    op = fr.ISS([fr.words.SimpleWord(s) for s in S_WORDS], mode=fr.ISSMode.EXTENDED)
    plan, row_prefix = nn._prefix_program(op)
    old = nat.to_device(S_LENGTHS.astype(np.int32), dtype=np.int32)
    new = nat.to_device(S_LENGTHS[::-1].astype(np.int32).copy(), dtype=np.int32)
    torch.cuda.synchronize()

    def arm(table):
        nat.check(nat.lib().fr_plan_set_grad_lengths(plan._h, C.c_void_p(table.data_ptr()), C.c_int64(S_N)),
                  "fr_plan_set_grad_lengths")

    def run(xb, gb):
        S = plan.run(xb, None, layout="KNT")
        return nat.iss_backward(plan, xb, S, gb, row_prefix)
    shape_x, shape_g = (S_N, 3, S_T), (S_N, len(row_prefix), S_T)
    try:
        report = so.replaced_in_flight(run, lambda: arm(old), lambda: arm(new),
                                       [draw(1, "normal", shape_x), draw(3, "normal", shape_g)],
                                       [draw(2, "normal", shape_x), draw(4, "normal", shape_g)],
                                       what="set_grad_lengths")
    finally:
        torch.cuda.synchronize()
        nat.check(nat.lib().fr_plan_set_grad_lengths(plan._h, None, C.c_int64(0)), "fr_plan_set_grad_lengths")
    so.note(record_property, report)
