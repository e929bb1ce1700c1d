"""GPU tests of the band features (fruits_amd.nn.iss_band_features, fr_sieve_heads,
fr_sieve_heads_adjoint): the forward bits against the standalone sieves, the
expansion against the numpy reference bit for bit, the whole gradient against the dense entries on
the reference's upstream for all five adjoints and against the long-double oracle, ragged batches,
the autograd wiring and a run on a side stream."""
import numpy as np
import pytest

import heads_grad_ref as hg
import iss_bounds as ib
import iss_grad_ref as gr
import ragged_grad_ref as rr
import stream_order as so
from test_features_gpu import (KINDS, WORD_SETS, batch_of, dense_entry, exact_input, make_op, mode_of,
                               real_input)

pytestmark = pytest.mark.gpu

TILE = 1024        # time steps the expansion forms at once (csrc/kernels.h, kHeadsTile)
LENGTHS = (1, 2, 3, 9, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
UNWEIGHTED = ("reals", "arctic", "bayesian")


@pytest.fixture(scope="module")
def env():
    import torch
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    nat.require_device()
    return fr, nn, torch


def head_list(T):
    """Every order the issue names - with T <= inc, where D is all zeros -, a segment that starts
    past 0, bands split at 0, and two selecting sieves."""
    from fruits_amd.sieving import CUR, END, MAX, MPI
    h = T // 2 or 1
    return [MPI([-1], inc=0), MPI([h, -1], q=(-1, 0, 1), inc=1), MPI([-1], inc=2), MPI([-1], inc=8),
            CUR([-1]), CUR([1, h, -1], q=(-1, 0, 1)), END([-1]), MAX([-1])]


def edge_heads(T):
    """``head_list`` and an END whose positions are t = 0, the two sides of the tile edge (where
    the series has them) and T - 1; the bands of the MPI / CUR sieves hold every step."""
    from fruits_amd.sieving import END
    return head_list(T) + [END([1] + [c for c in (TILE, TILE + 1) if c <= T] + [-1])]


def kinds_of(sieves):
    return np.concatenate([[type(s).__name__] * s.nfeatures() for s in sieves])


def device_rows(env, X, op, lengths=None):
    """The iterated sums ``(N, K, T)`` by the dense entry of the configuration, as a host array."""
    fr, nn, torch = env
    kind = "reals" if op.weighting is None and type(op.semiring).__name__ == "Reals" else (
        "total" if op.weighting is not None else "arctic")
    with torch.no_grad():
        Y = dense_entry(nn, kind)(torch.tensor(X, device="cuda"), op, lengths=lengths)
    return Y.cpu().numpy()


def band_grad(env, X, g, op, sieves, lengths=None):
    """(features (N, K * F), companion (N, K, F), X.grad) of ``(iss_band_features(X) * g).sum()`` as
    host arrays; ``g`` None: no backward pass.  Asserts what is kept for the backward pass."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    if lengths is None:
        feats = nn.iss_band_features(Xd, op, sieves=sieves)
    else:
        feats = nn.iss_band_features_ragged(Xd, lengths, op, sieves=sieves)
    saved = feats.grad_fn.saved_tensors
    ragged = lengths is not None and not (np.asarray(lengths) == X.shape[2]).all()
    assert len(saved) == 2 + ragged and saved[0].data_ptr() == Xd.data_ptr() and saved[1].dtype == torch.int32
    assert tuple(saved[1].shape[:2]) == (X.shape[0], feats.shape[1] // saved[1].shape[2])
    if ragged:
        assert saved[2].dtype == torch.int32 and tuple(saved[2].shape) == (X.shape[0],)
    comp = saved[1].cpu().numpy()
    if g is not None:
        feats.backward(torch.tensor(g, device="cuda").view(feats.shape))
    return feats.detach().cpu().numpy(), comp, None if g is None else Xd.grad.cpu().numpy()


def dense_grad(env, X, G, op, kind, lengths=None):
    """X.grad of ``(rows(X) * G).sum()`` through the dense entry of the kind."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    dense_entry(nn, kind)(Xd, op, lengths=lengths).backward(torch.tensor(G, device="cuda"))
    return Xd.grad.cpu().numpy()


def exact_gradients(comp, sieves, seed):
    """Integer feature gradients whose MPI columns are multiples of the in-band count: every
    weight g / c is an integer, and on integer rows so is every operation of the expansion."""
    g = np.random.default_rng(seed).integers(-3, 4, size=comp.shape).astype(np.float64)
    mpi = kinds_of(sieves) == "MPI"
    g[:, :, mpi] *= np.maximum(comp[:, :, mpi], 1)
    return g


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("inputs", ["integer", "real"])
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("name", list(WORD_SETS))
def test_forward_bits_and_companion(env, name, T, inputs):
    fr, nn, torch = env
    D, strings = WORD_SETS[name]
    at = LENGTHS.index(T) + (name == "fanout")
    mode = "EXTENDED" if at % 2 else "SINGLE"
    N = batch_of(T, at + (inputs == "real"))
    # (integer rows: the unweighted kinds; real ones: all five in turn)
    kind = UNWEIGHTED[at % 3] if inputs == "integer" else list(KINDS)[at % 5]
    X = exact_input(strings, N, D, T, seed=3) if inputs == "integer" else real_input(kind, N, D, T)
    op, sieves = make_op(fr, strings, mode, kind), edge_heads(T)
    F = sum(s.nfeatures() for s in sieves)
    feats, comp, _ = band_grad(env, X, None, op, sieves)
    Xd = torch.tensor(X, device="cuda")
    Y = op.transform_device(Xd)                                        # (K, N, T)
    K = int(Y.shape[0])
    assert feats.shape == (N, K * F) and comp.shape == (N, K, F)
    want = torch.zeros((K, N, F), dtype=torch.float64, device="cuda")
    for k in range(K):
        col = 0
        for s in sieves:
            s.transform_device(Y[k], want[k], col)
            col += s.nfeatures()
    want = want.cpu().numpy().transpose(1, 0, 2)
    feats = feats.reshape(N, K, F)
    rows = Y.cpu().numpy().transpose(1, 0, 2)
    ref_feats, ref_comp = hg.heads(rows, sieves)
    np.testing.assert_array_equal(comp, ref_comp)
    cur = kinds_of(sieves) == "CUR"
    np.testing.assert_array_equal(feats[:, :, ~cur], want[:, :, ~cur])
    if inputs == "integer":
        # (integer rows whose sums of squares are below 2^53: exact in any association)
        assert (rows == np.rint(rows)).all() and ref_feats[:, :, cur].max() < 2.0 ** 53
        np.testing.assert_array_equal(feats, want)
        np.testing.assert_array_equal(feats, ref_feats)
    else:
        # one rounding per square and c - 1 additions of non-negative terms, here and - with
        # contraction - in kernels_sieve.hip
        bound = (ref_comp[:, :, cur] + 2) * 2.0 ** -53 * want[:, :, cur]
        err = np.abs(feats[:, :, cur] - want[:, :, cur])
        print(f"CUR {name} T={T} {kind}: largest err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
        assert (err <= bound).all()
    assert (ref_comp[:, :, cur] > 0).any() or T < 3


# ---------------------------------------------------------------- the expansion alone
@pytest.mark.parametrize("inputs", ["integer", "real"])
@pytest.mark.parametrize("T", LENGTHS)
def test_expansion_equals_the_reference(env, T, inputs):
    """fr_sieve_heads_adjoint on downloaded rows against band_upstream, bit for bit, with real
    feature gradients; through a row map into a larger buffer and without one."""
    from fruits_amd import _native as nat
    fr, nn, torch = env
    at = LENGTHS.index(T)
    N, K = batch_of(T, at + (inputs == "real")), 3
    rng = np.random.default_rng([12, T, N])
    if inputs == "integer":
        rows = np.cumsum(rng.integers(-2, 3, size=(N, K, T)), axis=-1).astype(np.float64)
    else:
        rows = np.cumsum(rng.standard_normal((N, K, T)), axis=-1)
    sieves = edge_heads(T)
    head = nn._BandHead(sieves)
    tables = head.tables(T, torch.device("cuda", torch.cuda.current_device()))
    ref_feats, ref_comp = hg.heads(rows, sieves)
    g = rng.standard_normal(ref_comp.shape)
    want = hg.band_upstream(rows, sieves, ref_comp, g)
    kinds = kinds_of(sieves)
    # positions on t = 0, T - 1 and both sides of the tile edge; band elements everywhere
    pos = set(ref_comp[0, 0, np.isin(kinds, ("END", "MAX"))].tolist())
    assert {0, T - 1} | {c for c in (TILE - 1, TILE) if c < T} <= pos
    assert (ref_comp[:, :, np.flatnonzero(kinds == "CUR")[0]] == T).all()          # (CUR([-1]) holds every step)
    assert T < 3 or (np.abs(want[:, :, 0]).max() > 0 and np.abs(want[:, :, T - 1]).max() > 0)
    Yd = torch.tensor(rows.transpose(1, 0, 2).copy(), device="cuda")          # (K, N, T)
    comp_d, g_d = torch.tensor(ref_comp, device="cuda"), torch.tensor(g, device="cuda")
    feats, comp = nat.sieve_heads(Yd, *tables, head.F)
    np.testing.assert_array_equal(comp.cpu().numpy(), ref_comp)
    G = nat.sieve_heads_adjoint(Yd, *tables, comp_d, g_d)
    assert G.shape == (N, K, T) and G.is_contiguous()
    assert np.array_equal(G.cpu().numpy(), want), f"T={T} N={N} {inputs}"
    assert not np.signbit(G.cpu().numpy()[want == 0]).any()
    # the rows behind a row map: a buffer of K + 2 rows, the K rows in another order
    order = np.array([3, 0, 4], dtype=np.int32)
    S = torch.full((K + 2, N, T), 7.5, dtype=torch.float64, device="cuda")
    S[torch.tensor(order.astype(np.int64), device="cuda")] = Yd
    G2 = nat.sieve_heads_adjoint(S, *tables, comp_d, g_d, row_map=order,
                                 row_map_d=torch.tensor(order, device="cuda"))
    assert torch.equal(G2, G)


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("name", list(WORD_SETS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_gradient_equals_the_dense_entry(env, kind, name, T):
    """Real inputs, real feature gradients: X.grad equals X.grad of the dense entry run backward on
    the reference's G of the downloaded rows - the same adjoint kernels on the same bits."""
    fr, nn, torch = env
    D, strings = WORD_SETS[name]
    at = LENGTHS.index(T) + list(KINDS).index(kind) + (name == "fanout")
    mode = "EXTENDED" if at % 2 else "SINGLE"
    N = batch_of(T, at)
    X = real_input(kind, N, D, T)
    op, sieves = make_op(fr, strings, mode, kind), edge_heads(T)
    rows = op.transform_device(torch.tensor(X, device="cuda")).cpu().numpy().transpose(1, 0, 2)
    ref_feats, ref_comp = hg.heads(rows, sieves)
    g = np.random.default_rng([13, T, N]).standard_normal(ref_comp.shape)
    feats, comp, got = band_grad(env, X, g, op, sieves)
    np.testing.assert_array_equal(comp, ref_comp)
    want = dense_grad(env, X, hg.band_upstream(rows, sieves, ref_comp, g), op, kind)
    assert np.array_equal(got, want), f"{kind} {name} N={N} T={T} {mode}"
    assert np.abs(want).max() > 0 and np.isfinite(want).all()


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("name", list(WORD_SETS))
def test_gradient_exact(env, name, T):
    """Integer inputs over Reals, exact feature gradients: X.grad is the long-double oracle's
    gradient of the rows for the reference's G, bit for bit."""
    fr, nn, torch = env
    D, strings = WORD_SETS[name]
    at = LENGTHS.index(T) + (name == "fanout")
    mode = "EXTENDED" if at % 2 else "SINGLE"
    N = batch_of(T, at)
    X = exact_input(strings, N, D, T, seed=1)
    sieves = head_list(T)
    rows = gr.orc.iss_transform(X, strings, mode).transpose(1, 0, 2)          # (N, K, T)
    ref_feats, ref_comp = hg.heads(rows, sieves)
    g = exact_gradients(ref_comp, sieves, [6, T, N])
    G = hg.band_upstream(rows, sieves, ref_comp, g)
    assert (G == np.rint(G)).all()
    feats, comp, got = band_grad(env, X, g, make_op(fr, strings, mode, "reals"), sieves)
    np.testing.assert_array_equal(comp, ref_comp)
    np.testing.assert_array_equal(feats.reshape(ref_feats.shape), ref_feats)
    want = gr.iss_grad(X, G, strings, mode)
    assert np.abs(want).max() < 2.0 ** 50 and (want == want.astype(np.float64)).all()
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=f"{name} N={N} T={T} {mode}")
    assert np.abs(want).max() > 0


# ---------------------------------------------------------------- ragged
RAGGED_T = TILE + 1
RAGGED_LENGTHS = np.array([1, TILE, RAGGED_T, 9, 257, 2, TILE - 1])


def unweighted_alphas(fr, strings, mode, kind):
    """``make_op`` with every alpha 0: the exp factors of the weighted kinds are exactly 1."""
    op = make_op(fr, strings, mode, kind)
    if op.weighting is not None:
        words = [fr.words.SimpleWord(s) for s in strings]
        for i, w in enumerate(words):
            w.alpha = [0.0] * len(gr.orc.parse_word(strings[i]))
        op = fr.ISS(words, mode=mode_of(fr, mode), weighting=op.weighting)
    return op


@pytest.mark.parametrize("name", list(WORD_SETS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_ragged_equals_truncated_exact(env, kind, name):
    """All arithmetic exact (integer inputs, alpha 0, exact feature gradients): row n and
    X.grad[n, :, :L_n] are the bits of the call on the truncated series, the tail is +0.0."""
    fr, nn, torch = env
    D, strings = WORD_SETS[name]
    T, lengths = RAGGED_T, RAGGED_LENGTHS
    N, mode = len(lengths), "EXTENDED" if kind in ("reals", "total") else "SINGLE"
    X = np.abs(exact_input(strings, N, D, T, seed=2)) if kind == "bayesian" else exact_input(strings, N, D, T, seed=2)
    op, sieves = unweighted_alphas(fr, strings, mode, kind), head_list(T // 2)
    rows = device_rows(env, X, op, lengths)
    assert all((rows[n, :, :L] == np.rint(rows[n, :, :L])).all() for n, L in enumerate(lengths))
    ref_feats, ref_comp = hg.heads(rows, sieves, lengths)
    g = exact_gradients(ref_comp, sieves, [14, N])
    feats, comp, got = band_grad(env, X, g, op, sieves, lengths)
    np.testing.assert_array_equal(comp, ref_comp)
    np.testing.assert_array_equal(feats.reshape(ref_feats.shape), ref_feats)
    for n, L in enumerate(int(v) for v in lengths):
        f1, c1, g1 = band_grad(env, rr.truncated(X, n, L), g[n:n + 1], op, sieves)
        np.testing.assert_array_equal(feats[n:n + 1], f1, err_msg=f"{kind} series {n} L={L}")
        np.testing.assert_array_equal(comp[n:n + 1], c1)
        np.testing.assert_array_equal(got[n:n + 1, :, :L], g1, err_msg=f"{kind} series {n} L={L}")
        assert not got[n, :, L:].any() and not np.signbit(got[n, :, L:]).any()
    assert np.abs(got).max() > 0
    # ... and the dense entry with lengths on the reference's G: the same bits
    want = dense_grad(env, X, hg.band_upstream(rows, sieves, ref_comp, g, lengths), op, kind, lengths)
    np.testing.assert_array_equal(got, want)


def test_ragged_within_bound(env):
    """Real inputs over Reals: per series within 2 n_ops 2^-53 magnitude of the long-double oracle on
    the truncated series, the upstream being the reference's G of the rows the
    ragged forward pass formed."""
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    T, lengths, mode = RAGGED_T, RAGGED_LENGTHS, "EXTENDED"
    N = len(lengths)
    X = real_input("reals", N, D, T, seed=6)
    X[:, :, :] = np.where(np.arange(T) < lengths[:, None, None], X, 1e160 * (-1.0) ** np.arange(T))
    op, sieves = make_op(fr, strings, mode, "reals"), head_list(T // 2)
    rows = device_rows(env, X, op, lengths)
    ref_feats, ref_comp = hg.heads(rows, sieves, lengths)
    g = np.random.default_rng([15, N]).standard_normal(ref_comp.shape)
    feats, comp, got = band_grad(env, X, g, op, sieves, lengths)
    np.testing.assert_array_equal(comp, ref_comp)
    G = hg.band_upstream(rows, sieves, ref_comp, g, lengths)
    worst = 0.0
    for n, L in enumerate(int(v) for v in lengths):
        Xn, Gn = rr.truncated(X, n, L), rr.truncated(G, n, L)
        hp = rr.series_grad("reals", Xn, Gn, strings, mode)
        A = rr.series_grad("reals", Xn, Gn, strings, mode, magnitude=True)
        worst = max(worst, ib.check_bound(got[n:n + 1, :, :L], hp, A, rr.n_ops("reals", strings, L, mode),
                                          f"ragged band features series {n} L={L}"))
        assert not got[n, :, L:].any() and not np.signbit(got[n, :, L:]).any()
    print(f"ragged band features: largest err / bound over {N} series = {worst:.3g}")


# ---------------------------------------------------------------- autograd wiring
@pytest.mark.parametrize("kind", list(KINDS))
def test_backward_is_repeatable(env, kind):
    fr, nn, torch = env
    D, strings = WORD_SETS["fanout"]
    N, T = 7, TILE + 1
    X = real_input(kind, N, D, T, seed=2)
    op, sieves = make_op(fr, strings, "EXTENDED", kind), head_list(T)
    feats, comp, _ = band_grad(env, X, None, op, sieves)
    g = np.random.default_rng(10).standard_normal(feats.shape)
    f1, c1, first = band_grad(env, X, g, op, sieves)
    f2, c2, again = band_grad(env, X, g, op, sieves)
    for a, b in ((f1, f2), (c1, c2), (first, again)):
        np.testing.assert_array_equal(a, b)
    # the batch in two launches of 3 and 4 series: another grid, the same bits
    parts = [band_grad(env, np.ascontiguousarray(X[s]), np.ascontiguousarray(g[s]), op, sieves)
             for s in (slice(0, 3), slice(3, 7))]
    for i, whole in enumerate((f1, c1, first)):
        np.testing.assert_array_equal(np.concatenate([p[i] for p in parts]), whole)


def test_only_the_input_and_the_companion_are_kept(env):
    """After the forward call the (K, N, T) buffer of the walk is dead: the allocated memory has
    grown by the features and the companion alone."""
    fr, nn, torch = env
    D, strings = WORD_SETS["fanout"]
    N, T = 64, 2 * TILE + 3
    sieves = head_list(T)
    layer = nn.BandFeatureLayer([fr.words.SimpleWord(s) for s in strings], fr.ISSMode.SINGLE, sieves)
    K, F = len(strings), sum(s.nfeatures() for s in sieves)
    Xd = torch.tensor(real_input("reals", N, D, T, seed=5), device="cuda").requires_grad_(True)
    layer(Xd)                      # (the device programs and tables of the layer exist from here on)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    feats = layer(Xd)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    saved = feats.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[0].data_ptr() == Xd.data_ptr()
    assert saved[1].dtype == torch.int32 and tuple(saved[1].shape) == (N, K, F)
    slack = 64 * 1024           # (the allocator rounds each of the two tensors up to 512 bytes)
    assert K * N * T * 8 > 16 * slack
    assert 0 < grown <= N * K * F * 12 + slack, (grown, N * K * F * 12)
    before_backward = torch.cuda.memory_allocated()
    feats.sum().backward()
    torch.cuda.synchronize()
    assert Xd.grad.abs().max() > 0
    # G died with the backward call: what is left is X.grad
    assert torch.cuda.memory_allocated() - before_backward <= Xd.numel() * 8 + slack


def test_layer_trains_a_step(env):
    """BandFeatureLayer in front of a Linear head: one optimiser step, one backward pass, a lower
    loss; the functional form gives the layer's bits."""
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    N, T = 5, 130
    sieves = head_list(T)
    words = [fr.words.SimpleWord(s) for s in strings]
    layer = nn.BandFeatureLayer(words, fr.ISSMode.EXTENDED, sieves)
    assert "features per iterated sum" in repr(layer) and layer.sieves == sieves
    F = sum(s.nfeatures() for s in sieves)
    K = len(gr.output_prefixes(strings, "EXTENDED"))
    torch.manual_seed(0)
    scale = torch.nn.Parameter(torch.ones((1, D, 1), dtype=torch.float64, device="cuda"))
    lin = torch.nn.Linear(K * F, 3).double().cuda()
    X = torch.tensor(0.1 * real_input("reals", N, D, T, seed=3), device="cuda")
    opt = torch.optim.SGD([scale] + list(lin.parameters()), lr=1e-6)
    losses = []
    for _ in range(2):
        opt.zero_grad()
        before = nn.backward_calls()
        loss = lin(layer(X * scale)).square().mean()
        loss.backward()
        assert nn.backward_calls() == before + 1
        assert scale.grad.abs().max() > 0 and lin.weight.grad.abs().max() > 0
        losses.append(float(loss.detach()))
        opt.step()
    assert losses[1] < losses[0]
    Xa = (X * 1.0).requires_grad_(True)
    Xb = (X * 1.0).requires_grad_(True)
    layer(Xa).square().sum().backward()
    nn.iss_band_features(Xb, words, fr.ISSMode.EXTENDED, sieves).square().sum().backward()
    assert torch.equal(Xa.grad, Xb.grad)
    # no gradient asked for: no graph, no backward work
    calls = nn.backward_calls()
    assert layer(X).grad_fn is None
    assert nn.backward_calls() == calls


GRADCHECK_SEED = 3     # (of the seeds 0 ... 7 the one with the largest margins asserted below)


def test_gradcheck(env):
    """torch.autograd.gradcheck with its default tolerances on Reals, (2, 2, 9); the seed keeps
    every D[t] further than 1e-3 from every threshold, by the reference."""
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    N, T, mode = 2, 9, "EXTENDED"
    X = np.random.default_rng(GRADCHECK_SEED).standard_normal((N, D, T))
    sieves = head_list(T)
    rows = gr.orc.iss_transform(X, strings, mode).transpose(1, 0, 2)
    lead = [len(prefix) - 1 for prefix in gr.output_prefixes(strings, mode)]
    assert hg.threshold_distance(rows, sieves, lead) > 1e-3
    # (MAX: the two largest elements of a row apart, so that the step of gradcheck moves no argmax)
    top = np.sort(rows, axis=-1)
    assert (top[..., -1] - top[..., -2]).min() > 1e-3
    op = make_op(fr, strings, mode, "reals")
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: nn.iss_band_features(x, op, sieves=sieves), (Xd,))


# ---------------------------------------------------------------- a side stream
@pytest.mark.parametrize("kind", ["reals", "total"])
def test_behind_an_unfinished_producer(env, kind, record_property):
    """Forward and backward on a side stream while the producer of X and of the feature gradients
    is still running: the default-stream bits, and the call returns before its producer ends."""
    fr, nn, torch = env
    D, strings = WORD_SETS["prefix"]
    N, T = 9, TILE + 76
    op, sieves = make_op(fr, strings, "EXTENDED", kind), head_list(T)
    draw = lambda seed: real_input(kind, N, D, T, seed=seed)          # noqa: E731
    probe = nn.iss_band_features(torch.tensor(draw(1), device="cuda"), op, sieves=sieves)
    shape_g = tuple(probe.shape)
    torch.cuda.synchronize()

    def call(xb, gb):
        x = xb.detach().requires_grad_(True)
        y = nn.iss_band_features(x, op, sieves=sieves)
        side = torch.cuda.current_stream()
        with torch.cuda.stream(torch.cuda.default_stream()):
            y.backward(gb)
        side.wait_stream(torch.cuda.default_stream())
        return y.detach(), x.grad

    rng = np.random.default_rng(16)
    want, report = so.behind_producer(call, [draw(1), rng.standard_normal(shape_g)],
                                      [draw(2), rng.standard_normal(shape_g)],
                                      what=f"nn iss_band_features {kind} forward + backward")
    so.note(record_property, report)
    assert np.abs(want[1]).max() > 0
