"""GPU tests of the differentiable features (fruits_amd.nn.iss_features, fr_sieve_pick,
fr_iss_backward_picked): the forward bits and positions, the gradient against the long-double
oracle on integer-valued inputs, the sparse upstream against the dense one bit for bit for all
five adjoints, repeatability and the autograd wiring."""
import numpy as np
import pytest

import features_grad_ref as fg
import iss_grad_ref as gr

pytestmark = pytest.mark.gpu

CHUNK = 1024       # time steps the suffix kernels scan at once (csrc/kernels.h, kGradChunk)
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
# (D, words) of test_grad_gpu.py: two rows on one node and an inner node with rows AND children;
# a sibling fan-out of four
WORD_SETS = {
    "prefix": (2, ["[1]", "[1][2]", "[1][2][1]", "[2]", "[1][2]"]),
    "fanout": (3, ["[1][1]", "[1][2]", "[1][3]", "[1][12]", "[3]"]),
}
# the five adjoints: (semiring, weighting, total)
KINDS = {
    "reals": (None, None, False),
    "arctic": ("Arctic", None, False),
    "bayesian": ("Bayesian", None, False),
    "nontotal": (None, "Indices", False),
    "total": (None, "Indices", True),
}


@pytest.fixture(scope="module")
def env():
    import torch
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    nat.require_device()
    return fr, nn, torch


def mode_of(fr, mode):
    return fr.ISSMode.EXTENDED if mode == "EXTENDED" else fr.ISSMode.SINGLE


def sieve_list(T):
    """Several features on one position (the ENDs at T - 1, the extremes wherever they fall),
    segments that start past 0, a band split at 0."""
    from fruits_amd.sieving import END, MAX, MIN
    h = T // 2 or 1
    return [END([-1]), END([1, h, -1]), MAX([-1]), MIN([h, -1]), MAX([-1], q=(-1, 0, 1))]


def edge_sieves(T):
    """``sieve_list`` and an END whose positions are t = 0, 1023, 1024 (where the series has
    them) and T - 1: the two sides of a chunk edge of the scan."""
    from fruits_amd.sieving import END
    return sieve_list(T) + [END([1] + [c for c in (CHUNK, CHUNK + 1) if c <= T] + [-1])]


def make_op(fr, strings, mode, kind):
    """The ISS of a kind; a weighted one with an alpha per letter from {0.5, 1, 1.5}."""
    semiring, weighting, total = KINDS[kind]
    words = [fr.words.SimpleWord(s) for s in strings]
    kw = {}
    if semiring:
        kw["semiring"] = getattr(fr.semiring, semiring)()
    if weighting:
        from fruits_amd.iss.weighting import Indices
        kw["weighting"] = Indices(total=total)
        for i, w in enumerate(words):
            w.alpha = [0.5 * (1 + (i + j) % 3) for j in range(len(gr.orc.parse_word(strings[i])))]
    return fr.ISS(words, mode=mode_of(fr, mode), **kw)


def dense_entry(nn, kind):
    return {"reals": nn.iss, "arctic": nn.max_iss, "bayesian": nn.max_iss}.get(kind, nn.weighted_iss)


def features_grad(env, X, g, op, sieves):
    """(features (N, K * F), positions (N, K, F), X.grad) of ``(iss_features(X) * g).sum()``, as
    host arrays; ``g`` None: no backward pass."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    feats = nn.iss_features(Xd, op, sieves=sieves)
    saved = feats.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == Xd.data_ptr() and saved[1].dtype == torch.int32
    pos = saved[1].cpu().numpy()
    if g is not None:
        feats.backward(torch.tensor(g, device="cuda").view(feats.shape))
    return feats.detach().cpu().numpy(), pos, None if g is None else Xd.grad.cpu().numpy()


def dense_grad(env, X, G, op, kind):
    """X.grad of ``(rows(X) * G).sum()`` through the dense entry of the kind."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    dense_entry(nn, kind)(Xd, op).backward(torch.tensor(G, device="cuda"))
    return Xd.grad.cpu().numpy()


def exact_input(strings, N, D, T, seed):
    """Integer-valued X from {-2 ... 2}, ties everywhere (test_grad_gpu.py).  Series 0 is made
    non-negative with a 1 in front: its one-letter rows are positive and never fall, so the band
    (-inf, 0] of such a row is EMPTY and its extremes are attained wherever the input is 0."""
    rng = np.random.default_rng([seed, N, D, T])
    X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    X[0] = np.abs(X[0])
    X[0, :, 0] = 1.0
    return X


def real_input(kind, N, D, T, seed=0):
    """Real-valued X: Reals and weighted - standard normal around 1; Arctic - standard normal on
    a rising trend; Bayesian - uniform in [0.25, 1] (as test_grad_max_gpu.py)."""
    rng = np.random.default_rng([seed, N, D, T, 11])
    if kind == "arctic":
        return rng.standard_normal((N, D, T)) + 0.02 * np.arange(T)
    if kind == "bayesian":
        return 0.25 + 0.75 * rng.random((N, D, T))
    return rng.standard_normal((N, D, T)) + 1.0


def batch_of(T, at):
    """N in {1, 3}; 261 series - more workgroups than one round of the device - up to T = 257."""
    return (1, 3, 261)[at % 3] if T <= 257 else (1, 3)[at % 2]


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("kind", ["reals", "arctic", "total"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("name", list(WORD_SETS))
def test_forward_bits_and_positions(env, name, T, kind):
    fr, nn, torch = env
    D, strings = WORD_SETS[name]
    mode = "EXTENDED" if (LENGTHS.index(T) + (name == "fanout")) % 2 else "SINGLE"
    N = batch_of(T, LENGTHS.index(T) + list(KINDS).index(kind))
    X = exact_input(strings, N, D, T, seed=3) if kind != "total" else real_input(kind, N, D, T)
    op, sieves = make_op(fr, strings, mode, kind), edge_sieves(T)
    F = sum(s.nfeatures() for s in sieves)
    feats, pos, _ = features_grad(env, X, None, op, sieves)
    # the rows, and every sieve on every row by the standalone kernels
    Xd = torch.tensor(X, device="cuda")
    Y = op.transform_device(Xd)                                        # (K, N, T)
    K = int(Y.shape[0])
    assert feats.shape == (N, K * F) and pos.shape == (N, K, F)
    want = torch.zeros((K, N, F), dtype=torch.float64, device="cuda")
    for k in range(K):
        col = 0
        for s in sieves:
            s.transform_device(Y[k], want[k], col)
            col += s.nfeatures()
    # Fruit's column order: iterated sum, then sieve, then the sieve's (segment, band) order
    np.testing.assert_array_equal(feats.reshape(N, K, F), want.cpu().numpy().transpose(1, 0, 2))
    rows = Y.cpu().numpy().transpose(1, 0, 2)
    ref_feats, ref_pos = fg.pick(rows, sieves)
    np.testing.assert_array_equal(pos, ref_pos)
    np.testing.assert_array_equal(feats.reshape(N, K, F), ref_feats)
    # the last END: t = 0, the two sides of the chunk edge, T - 1
    assert pos[0, 0, -1] == T - 1 and pos[0, 0, F - (2 + (T >= CHUNK) + (T > CHUNK))] == 0
    assert {0, T - 1} | {c for c in (CHUNK - 1, CHUNK) if c < T} <= set(pos[0, 0].tolist())


# ---------------------------------------------------------------- exact
EXACT_SEED = 1     # (chosen so that every case meets the three conditions asserted below)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("name", list(WORD_SETS))
def test_gradient_exact(env, name, T):
    """Integer inputs, integer feature gradients: X.grad is the long-double oracle's gradient of
    the rows for the scattered upstream, bit for bit - with ties, empty bands and several
    features on one element."""
    fr, nn, torch = env
    D, strings = WORD_SETS[name]
    at = LENGTHS.index(T) + (name == "fanout")
    mode = "EXTENDED" if at % 2 else "SINGLE"
    N = batch_of(T, at)
    X = exact_input(strings, N, D, T, seed=EXACT_SEED)
    sieves = sieve_list(T)
    rows = gr.orc.iss_transform(X, strings, mode).transpose(1, 0, 2)   # (N, K, T)
    ref_feats, ref_pos = fg.pick(rows, sieves)
    K, F = ref_pos.shape[1:]
    # what the case has to hold, from the reference alone
    count = fg.attained(rows, sieves)
    kinds = np.concatenate([[type(s).__name__] * s.nfeatures() for s in sieves])
    if T >= 2:
        assert (count[:, :, kinds != "END"] > 1).any(), "no MAX / MIN attains its extreme twice"
    assert (ref_pos == -1).any(), "no empty feature"
    assert 2 * (ref_pos >= 0).sum() >= ref_pos.size, "fewer than half of the features select"
    g = np.random.default_rng([6, T, K, N]).integers(-3, 4, size=(N, K * F)).astype(np.float64)
    feats, pos, got = features_grad(env, X, g, make_op(fr, strings, mode, "reals"), sieves)
    np.testing.assert_array_equal(pos, ref_pos)
    np.testing.assert_array_equal(feats.reshape(N, K, F), ref_feats)
    want = gr.iss_grad(X, fg.dense_upstream(ref_pos, g, T), strings, mode)
    assert np.abs(want).max() < 2.0 ** 50 and (want == want.astype(np.float64)).all()
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=f"{name} N={N} T={T} {mode}")
    assert np.abs(want).max() > 0


# ---------------------------------------------------------------- sparse equals dense
@pytest.mark.parametrize("T", [2, 65, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
@pytest.mark.parametrize("name", list(WORD_SETS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_sparse_equals_dense(env, kind, name, T):
    """Real-valued X, integer-valued feature gradients: every b is a sum of integers - exact in
    any order - so the sparse route has the bits of the dense entry on the scattered gradient."""
    fr, nn, torch = env
    D, strings = WORD_SETS[name]
    at = LENGTHS.index(T) + list(KINDS).index(kind) + (name == "fanout")
    mode = "EXTENDED" if at % 2 else "SINGLE"
    N = batch_of(T, at)
    X = real_input(kind, N, D, T)
    op, sieves = make_op(fr, strings, mode, kind), edge_sieves(T)
    feats, pos, _ = features_grad(env, X, None, op, sieves)
    K, F = pos.shape[1:]
    g = np.random.default_rng([8, T, K, N]).integers(-3, 4, size=(N, K * F)).astype(np.float64)
    _, pos2, got = features_grad(env, X, g, op, sieves)
    np.testing.assert_array_equal(pos2, pos)
    assert {0, T - 1} | {c for c in (CHUNK - 1, CHUNK) if c < T} <= set(pos[0, 0].tolist())
    want = dense_grad(env, X, fg.dense_upstream(pos, g, T), op, kind)
    np.testing.assert_array_equal(got, want, err_msg=f"{kind} {name} N={N} T={T} {mode}")
    assert np.abs(want).max() > 0 and np.isfinite(want).all()


@pytest.mark.parametrize("T", [CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3])
@pytest.mark.parametrize("kind", list(KINDS))
def test_sparse_equals_dense_real_gradients(env, kind, T):
    """Real-valued feature gradients on positions that do not coincide: every b is 0.0 + one
    weight, in both routes - bit for bit again."""
    from fruits_amd.sieving import END, MIN
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    N, mode = 3, "EXTENDED"
    X = real_input(kind, N, D, T, seed=1)
    op, sieves = make_op(fr, strings, mode, kind), [END([-1]), MIN([-1])]
    feats, pos, _ = features_grad(env, X, None, op, sieves)
    assert (pos[:, :, 0] == T - 1).all() and (pos[:, :, 1] != pos[:, :, 0]).all() and (pos[:, :, 1] >= 0).all()
    g = np.random.default_rng([9, T]).standard_normal(feats.shape)
    _, _, got = features_grad(env, X, g, op, sieves)
    want = dense_grad(env, X, fg.dense_upstream(pos, g, T), op, kind)
    np.testing.assert_array_equal(got, want, err_msg=f"{kind} T={T}")
    assert np.abs(want).max() > 0


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("kind", list(KINDS))
def test_backward_is_repeatable(env, kind):
    fr, nn, torch = env
    D, strings = WORD_SETS["fanout"]
    N, T = 7, CHUNK + 1
    X = real_input(kind, N, D, T, seed=2)
    op, sieves = make_op(fr, strings, "EXTENDED", kind), sieve_list(T)
    feats, pos, _ = features_grad(env, X, None, op, sieves)
    g = np.random.default_rng(10).standard_normal(feats.shape)
    f1, p1, first = features_grad(env, X, g, op, sieves)
    f2, p2, again = features_grad(env, X, g, op, sieves)
    for a, b in ((f1, f2), (p1, p2), (first, again)):
        np.testing.assert_array_equal(a, b)
    # the batch in two launches of 3 and 4 series: another grid, the same bits
    parts = [features_grad(env, np.ascontiguousarray(X[s]), np.ascontiguousarray(g[s]), op, sieves)
             for s in (slice(0, 3), slice(3, 7))]
    for i, whole in enumerate((f1, p1, first)):
        np.testing.assert_array_equal(np.concatenate([p[i] for p in parts]), whole)


# ---------------------------------------------------------------- autograd
def test_layer_in_a_model(env):
    """FeatureLayer in front of a Linear head: loss.backward() fills X.grad, one backward pass."""
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    N, T = 5, 130
    sieves = sieve_list(T)
    words = [fr.words.SimpleWord(s) for s in strings]
    layer = nn.FeatureLayer(words, fr.ISSMode.EXTENDED, sieves)
    F = sum(s.nfeatures() for s in sieves)
    K = len(gr.output_prefixes(strings, "EXTENDED"))
    torch.manual_seed(0)
    model = torch.nn.Sequential(layer, torch.nn.Linear(K * F, 3).double()).cuda()
    X = real_input("reals", N, D, T, seed=3)
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    before = nn.backward_calls()
    loss = model(Xd).square().sum()
    loss.backward()
    assert nn.backward_calls() == before + 1
    assert Xd.grad is not None and Xd.grad.shape == Xd.shape and Xd.grad.abs().max() > 0
    assert model[1].weight.grad.abs().max() > 0
    # the same numbers through the dense route: rows, then torch's own selection by the positions
    feats, pos, _ = features_grad(env, X, None, layer.op, sieves)
    Xe = torch.tensor(X, device="cuda").requires_grad_(True)
    Y = nn.iss(Xe, words, fr.ISSMode.EXTENDED)                          # (N, K, T)
    idx = torch.tensor(pos, device="cuda").long()
    picked = torch.where(idx >= 0, torch.gather(Y, 2, idx.clamp(min=0)), torch.zeros((), dtype=torch.float64, device="cuda"))
    assert torch.equal(picked.reshape(N, -1), torch.tensor(feats, device="cuda"))
    model[1](picked.reshape(N, -1)).square().sum().backward()
    # (torch scatters coinciding features with atomics, in no fixed order: close, not equal)
    torch.testing.assert_close(Xd.grad, Xe.grad, rtol=1e-10, atol=1e-10)
    # the functional form, a list of words: the same bits as the layer
    Xf = torch.tensor(X, device="cuda").requires_grad_(True)
    model[1](nn.iss_features(Xf, words, fr.ISSMode.EXTENDED, sieves)).square().sum().backward()
    assert torch.equal(Xf.grad, Xd.grad)


def test_expanded_gradient_and_no_graph(env):
    """.sum().backward(): the upstream arrives as an expanded scalar and is made contiguous."""
    fr, nn, torch = env
    D, strings = WORD_SETS["fanout"]
    N, T = 3, 300
    sieves = sieve_list(T)
    X = real_input("reals", N, D, T, seed=4)
    op = make_op(fr, strings, "SINGLE", "reals")
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    before = nn.backward_calls()
    feats = nn.iss_features(Xd, op, sieves=sieves)
    feats.sum().backward()
    assert nn.backward_calls() == before + 1
    _, pos, _ = features_grad(env, X, None, op, sieves)
    want = dense_grad(env, X, fg.dense_upstream(pos, np.ones(feats.shape), T), op, "reals")
    np.testing.assert_array_equal(Xd.grad.cpu().numpy(), want)
    # a column slice: a strided upstream
    Xs = torch.tensor(X, device="cuda").requires_grad_(True)
    nn.iss_features(Xs, op, sieves=sieves)[:, ::2].sum().backward()
    g = np.zeros(feats.shape)
    g[:, ::2] = 1.0
    np.testing.assert_array_equal(Xs.grad.cpu().numpy(),
                                  dense_grad(env, X, fg.dense_upstream(pos, g, T), op, "reals"))
    # no gradient asked for: no graph, no backward work
    calls = nn.backward_calls()
    assert nn.iss_features(Xd.detach(), op, sieves=sieves).grad_fn is None
    with torch.no_grad():
        assert not nn.iss_features(Xd, op, sieves=sieves).requires_grad
    assert nn.backward_calls() == calls


def test_only_the_input_and_the_positions_are_kept(env):
    """After the forward call the (K, N, T) buffer of the walk is dead: the allocated memory has
    grown by the features and the positions (X itself is the caller's, already counted; a copy of
    it would be allowed), not by K N T doubles."""
    fr, nn, torch = env
    D, strings = WORD_SETS["fanout"]
    N, T = 64, 2 * CHUNK + 3
    sieves = sieve_list(T)
    layer = nn.FeatureLayer([fr.words.SimpleWord(s) for s in strings], fr.ISSMode.SINGLE, sieves)
    K, F = len(strings), sum(s.nfeatures() for s in sieves)
    Xd = torch.tensor(real_input("reals", N, D, T, seed=5), device="cuda").requires_grad_(True)
    layer(Xd)                      # (the device programs and tables of the layer exist from here on)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    feats = layer(Xd)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    # slack: the allocator rounds each of the two tensors up to 512 bytes; 64 KiB is far above
    # that and far below the rows
    slack = 64 * 1024
    rows = K * N * T * 8
    allowed = N * K * F * 8 + N * K * F * 4 + Xd.numel() * 8 + slack
    assert rows > 16 * slack and allowed < rows
    assert 0 < grown <= allowed, (grown, allowed, rows)
    assert grown <= N * K * F * 12 + slack      # (X was contiguous: not even a copy of it)
    feats.sum().backward()
    assert Xd.grad.abs().max() > 0
