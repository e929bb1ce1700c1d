"""GPU tests of the differentiable cosine weighted iterated sums (fruits_amd.nn.cos_iss,
fr_iss_backward with a CosWISS plan): the forward bits, the gradient against the long-double
oracle of the adjoint recursion - exactly where the weight is 1, within the derived rounding
bound with real frequencies -, torch's gradcheck, repeatability and the split into series blocks,
the autograd wiring, a side stream."""
import functools

import numpy as np
import pytest

import coswiss_grad_ref as cg
import iss_bounds as ib
import iss_grad_ref as gr
import stream_order as so

pytestmark = pytest.mark.gpu

WORDS = ["[1]", "[1][2]", "[12][1][-2]"]
D = 2
FREQS = [0.25, 1.5]
# every length at which a kernel changes path: the wave edge (64 lanes x 4 steps: 255 ... 257; a
# lane: 63 ... 65), the packed / cooperative forward edge (384, 385), the chunk edge, two chunks + 3
LENGTHS = (2, 3, 63, 64, 65, 255, 256, 257, 384, 385, 1023, 1024, 1025, 2051)
# The error of the device library's double sin / cos, in ulp, that n_ops_grad_cos is run with
# (DESIGN.md 4.14.7): no accuracy table of the HIP math functions is installed with ROCm, so it is
# the smallest U with which the FORWARD pass of the very configurations of
# test_gradient_within_the_bound meets its own long-double oracle under the same counting
# (cg.n_ops_cos) - test_forward_needs_no_more_than_U holds that.
COS_U = 0


@pytest.fixture(scope="module")
def env():
    import torch
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    nat.require_device()
    yield fr, nn, torch
    ib.print_ratios()


def words_of(fr, strings=WORDS):
    return [fr.words.SimpleWord(s) for s in strings]


def exact_input(N, T, seed=0):
    """Integer-valued X from {-2 ... 2} - zeros included - and {+-0.5, +-1, +-2} in dimension 2,
    which WORDS divides by: every partial sum of the gradient is a dyadic rational below 2^53, so
    any order of the additions gives the same bits."""
    rng = np.random.default_rng([seed, N, T])
    X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
    X[:, 1] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=(N, T))
    return X


def real_input(N, T, seed=0):
    """Inputs in [0.5, 1.5] (a word divides by dimension 2) and a standard normal upstream."""
    rng = np.random.default_rng([seed, N, T, 7])
    return rng.uniform(0.5, 1.5, size=(N, D, T)), rng.standard_normal


def device_grad(env, X, G, freqs, S, total, strings=WORDS):
    """X.grad of ``(nn.cos_iss(X) * G).sum()`` and the forward result, as host arrays."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    Y = nn.cos_iss(Xd, words_of(fr, strings), freqs, S, total)
    Y.backward(torch.tensor(G, device="cuda"))
    return Xd.grad.cpu().numpy(), Y.detach().cpu().numpy()


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("T", [100, 1100])
def test_forward_is_transform(env, T, total):
    fr, nn, torch = env
    X, _ = real_input(3, T)
    want = fr.CosWISS(words_of(fr), FREQS, 2, total).transform(X)              # (W * F, N, T)
    got = nn.cos_iss(torch.tensor(X, device="cuda"), words_of(fr), FREQS, 2, total)
    assert tuple(got.shape) == (3, len(WORDS) * len(FREQS), T)
    np.testing.assert_array_equal(got.cpu().numpy(), want.transpose(1, 0, 2))
    layer = nn.CosWISSLayer(words_of(fr), FREQS, total_weighting=total)
    np.testing.assert_array_equal(layer(torch.tensor(X, device="cuda")).cpu().numpy(), want.transpose(1, 0, 2))


# ---------------------------------------------------------------- exact
@functools.lru_cache(maxsize=None)
def exact_case(T):
    """(X, G, the unweighted gradient) at length T, shared by every exponent and weighting."""
    X = exact_input(3, T)
    G = np.random.default_rng([1, T]).integers(-3, 4, size=(3, len(WORDS), T)).astype(np.float64)
    want = gr.iss_grad(X, G, WORDS, "SINGLE").astype(np.float64)
    for a in (X, G, want):
        a.setflags(write=False)
    return X, G, want


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("T", LENGTHS)
def test_infinite_frequency_is_the_unweighted_gradient(env, T, S, total):
    """freqs = [inf]: the device angle is exactly 0, sin = 0, cos = 1, q_S = 1 and every other
    q_m = 0 - on integer-valued inputs the gradient is the unweighted oracle's, bit for bit:
    shifts, both lane maps, carries and the gather, whatever the rounding model."""
    X, G, want = exact_case(T)
    got, Y = device_grad(env, X, G, [np.inf], S, total)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(Y, gr.orc.iss_transform(X, WORDS, "SINGLE").transpose(1, 0, 2))
    assert np.abs(want).max() > 0


@pytest.mark.parametrize("T", [65, 1025, 2051])
def test_expanded_scalar_and_a_row_named_twice(env, T):
    fr, nn, torch = env
    from fruits_amd import _native as nat
    X, G, _ = exact_case(T)
    for S, total in ((1, True), (3, False)):
        # an upstream that is an expanded scalar: zero strides in every axis
        Xd = torch.tensor(X, device="cuda").requires_grad_(True)
        nn.cos_iss(Xd, words_of(fr), [np.inf], S, total).sum().backward()
        np.testing.assert_array_equal(Xd.grad.cpu().numpy(),
                                      gr.iss_grad(X, np.ones_like(G), WORDS, "SINGLE").astype(np.float64))
        # row 1 named by two rows of the upstream, through the raw wrapper
        plan = nat.CosPlan([np.asarray(w.table(), dtype=np.int32) for w in words_of(fr)], [np.inf], S, total)
        G4 = np.concatenate([G, G[:, :1] - 1.0], axis=1)
        got = nat.iss_backward_cos(plan, torch.tensor(X, device="cuda"), torch.tensor(G4, device="cuda"),
                                   np.array([0, 1, 2, 1], dtype=np.int32))
        summed = G.copy()
        summed[:, 1] += G4[:, 3]
        np.testing.assert_array_equal(got.cpu().numpy(), gr.iss_grad(X, summed, WORDS, "SINGLE").astype(np.float64))


def test_one_step_one_letter_is_the_suffix(env):
    """T = 1: the rows are NaN wherever a trig factor enters (0 / 0 in the angle, as in the
    reference) - but a one-letter word without total weighting has none: dX = suffix(G)."""
    fr, nn, torch = env
    X = np.array([[[2.0], [3.0]], [[-1.0], [0.5]]])
    G = np.array([[[5.0], [0.25]], [[-2.0], [7.0]]])
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    Y = nn.cos_iss(Xd, words_of(fr, ["[1]"]), FREQS, 2, False)
    Y.backward(torch.tensor(G, device="cuda"))
    np.testing.assert_array_equal(Y.detach().cpu().numpy(), np.repeat(X[:, :1], 2, axis=1))
    want = np.zeros_like(X)
    want[:, 0] = G.sum(axis=1)
    np.testing.assert_array_equal(Xd.grad.cpu().numpy(), want)
    assert not np.signbit(Xd.grad.cpu().numpy()[:, 1]).any()       # a dimension no word names: +0.0


# ---------------------------------------------------------------- every m
BOUND_CASES = [(3, 300), (3, 1030), (2, 2051)]


@functools.lru_cache(maxsize=None)
def bound_inputs(N, T):
    X, normal = real_input(N, T, seed=2)
    G = normal((N, len(WORDS) * len(FREQS), T))
    for a in (X, G):
        a.setflags(write=False)
    return X, G


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("N,T", BOUND_CASES)
def test_gradient_within_the_bound(env, N, T, S, total):
    """|dX_dev - coswiss_grad| <= 2 n_ops_grad_cos 2^-53 coswiss_grad(magnitude=True), elementwise,
    the oracle fed long-double trig values."""
    X, G = bound_inputs(N, T)
    got, _ = device_grad(env, X, G, FREQS, S, total)
    hp = cg.coswiss_grad(X, G, WORDS, FREQS, S, total)
    A = cg.coswiss_grad(X, G, WORDS, FREQS, S, total, magnitude=True)
    n = cg.n_ops_grad_cos(WORDS, T, FREQS, S, total, COS_U)
    r = ib.check_bound(got, hp, A, n, f"cos grad N={N} T={T} S={S} total={total}", "grad_cos")
    print(f"COS-GRAD-RATIO T={T} S={S} total={total}: err / bound = {r:.3g} (n_ops {n})")
    # the bound is no formality: the other weighting's gradient lies far outside
    assert ib.violates(cg.coswiss_grad(X, G, WORDS, FREQS, S, not total, dtype=np.float64), hp, A, n)


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_largest_instantiation_within_the_bound(env, total):
    """S = 8, two letters: the instantiation with the most registers runs."""
    words, N, T, S = ["[1]", "[1][2]"], 2, 70, 8
    X, normal = real_input(N, T, seed=3)
    G = normal((N, len(words) * len(FREQS), T))
    got, _ = device_grad(env, X, G, FREQS, S, total, words)
    hp = cg.coswiss_grad(X, G, words, FREQS, S, total)
    A = cg.coswiss_grad(X, G, words, FREQS, S, total, magnitude=True)
    n = cg.n_ops_grad_cos(words, T, FREQS, S, total, COS_U)
    r = ib.check_bound(got, hp, A, n, f"cos grad S=8 total={total}", "grad_cos_s8")
    print(f"COS-GRAD-RATIO T={T} S=8 total={total}: err / bound = {r:.3g} (n_ops {n})")


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("N,T", BOUND_CASES)
def test_forward_needs_no_more_than_U(env, N, T, S, total):
    """Where COS_U comes from: the forward pass of the same configurations against its own
    long-double oracle, under the same counting with the same U."""
    fr, nn, torch = env
    X, _ = bound_inputs(N, T)
    got = nn.cos_iss(torch.tensor(X, device="cuda"), words_of(fr), FREQS, S, total).cpu().numpy()
    hp = cg.coswiss_forward(X, WORDS, FREQS, S, total)
    ones = (np.ones((len(FREQS), T)), np.ones((len(FREQS), T)))
    A = cg.coswiss_forward(np.abs(X), WORDS, None, S, total, tables=ones)
    n = cg.n_ops_cos(WORDS, T, FREQS, S, total, COS_U)
    r = ib.check_bound(got, hp, A, n, f"cos forward N={N} T={T} S={S} total={total}", "forward_cos_same_count")
    print(f"COS-FWD-RATIO T={T} S={S} total={total}: err / bound = {r:.3g} (n_ops {n})")


# ---------------------------------------------------------------- gradcheck
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_gradcheck(env, total):
    """Independent of any trig accuracy: a wrong binomial or a wrong q_m[t + 1] shows here."""
    fr, nn, torch = env
    X, _ = real_input(2, 9, seed=4)
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    layer = nn.CosWISSLayer(words_of(fr), FREQS, 2, total)
    assert torch.autograd.gradcheck(layer, (Xd,), eps=1e-6, atol=1e-6, rtol=1e-5)


# ---------------------------------------------------------------- one association
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_same_bits_however_the_batch_is_split(env, total, monkeypatch):
    fr, nn, torch = env
    from fruits_amd import _native as nat
    N, T, S = 7, 1100, 3
    X, normal = real_input(N, T, seed=5)
    G = normal((N, len(WORDS) * len(FREQS), T))
    whole, _ = device_grad(env, X, G, FREQS, S, total)
    again, _ = device_grad(env, X, G, FREQS, S, total)
    np.testing.assert_array_equal(again, whole)
    first, _ = device_grad(env, X[:3], G[:3], FREQS, S, total)
    second, _ = device_grad(env, X[3:], G[3:], FREQS, S, total)
    np.testing.assert_array_equal(np.concatenate([first, second]), whole)
    # the wrapper's own series blocks: a budget of two series' scratch
    op = fr.CosWISS(words_of(fr), FREQS, S, total)
    rows = sum(nat.coswiss_grad_rows(op._plan(0, len(WORDS))))
    calls = []
    real_backward = nat.iss_backward_cos
    monkeypatch.setattr(nn, "_device_budget_bytes", lambda: 2 * 8 * rows * T)
    monkeypatch.setattr(nat, "iss_backward_cos", lambda plan, Xd, *a, **k: (calls.append(int(Xd.shape[0])),
                                                                             real_backward(plan, Xd, *a, **k))[1])
    before = nn.backward_calls()
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    nn.cos_iss(Xd, op).backward(torch.tensor(G, device="cuda"))
    assert calls == [2, 2, 2, 1] and nn.backward_calls() == before + 1
    np.testing.assert_array_equal(Xd.grad.cpu().numpy(), whole)


# ---------------------------------------------------------------- layer and graph
def test_layer_trains_and_counts(env):
    fr, nn, torch = env
    from fruits_amd import _native as nat
    N, T, S, total = 4, 50, 2, True
    K = len(WORDS) * len(FREQS)
    X, normal = real_input(N, T, seed=6)
    torch.manual_seed(0)
    layer = nn.CosWISSLayer(words_of(fr), FREQS, S, total)
    assert "3 words, 2 frequencies, exponent 2, total" in repr(layer)
    model = torch.nn.Sequential(layer, torch.nn.Flatten(), torch.nn.Linear(K * T, 1).double()).cuda()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    target = torch.tensor(normal((N, 1)), device="cuda")
    before = nn.backward_calls()
    loss0 = ((model(Xd) - target) ** 2).mean()
    loss0.backward()
    assert nn.backward_calls() == before + 1
    assert Xd.grad is not None and torch.isfinite(Xd.grad).all() and Xd.grad.abs().max() > 0
    opt.step()
    loss1 = ((model(Xd) - target) ** 2).mean()
    assert torch.isfinite(loss1) and loss1.item() != loss0.item()
    # a row no loss reads: zeros in the dense upstream - the raw call that does not name it at all
    # launches nothing for it and gives the same dX
    G = normal((N, K, T))
    keep = [0, 1, 2, 4, 5]
    Xe = torch.tensor(X, device="cuda").requires_grad_(True)
    Y = nn.cos_iss(Xe, layer.op)
    (Y[:, keep] * torch.tensor(G[:, keep], device="cuda")).sum().backward()
    plan = layer.op._plan(0, len(WORDS))
    raw = nat.iss_backward_cos(plan, torch.tensor(X, device="cuda"),
                               torch.tensor(np.ascontiguousarray(G[:, keep]), device="cuda"),
                               np.array(keep, dtype=np.int32))
    np.testing.assert_array_equal(raw.cpu().numpy(), Xe.grad.cpu().numpy())


def test_entry_refuses_a_dropout_mask(env):
    fr, nn, torch = env
    from fruits_amd import _native as nat
    T = 20
    plan = nat.CosPlan([np.array([[1]], dtype=np.int32)], [0.5], 2, False)
    nat.coswiss_set_dropout(plan, np.array([[[[3, 7]]]], dtype=np.int32), T)
    Xd = torch.ones((2, 1, T), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="fr_iss_backward: the CosWISS plan has a dropout mask set"):
        nat.iss_backward_cos(plan, Xd, torch.ones((2, 1, T), dtype=torch.float64, device="cuda"),
                             np.array([0], dtype=np.int32))


# ---------------------------------------------------------------- a side stream
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_backward_on_a_side_stream(env, record_property, total):
    """One backward call at T = 1100 on a non-blocking side stream behind an unfinished producer
    of X and of G: the result of the default stream, bit for bit (tests/stream_order.py)."""
    fr, nn, torch = env
    from fruits_amd import _native as nat
    N, T, S = 3, 1100, 2
    K = len(WORDS) * len(FREQS)
    plan = nat.CosPlan([np.asarray(w.table(), dtype=np.int32) for w in words_of(fr)], FREQS, S, total)
    rows = np.arange(K, dtype=np.int32)
    X, normal = real_input(N, T, seed=8)
    G = normal((N, K, T))
    Xw, normal_w = real_input(N, T, seed=9)
    Gw = normal_w((N, K, T))

    def call(xb, gb):
        return nat.iss_backward_cos(plan, xb, gb, rows)

    _, report = so.behind_producer(call, [X, G], [Xw, Gw], what=f"fr_iss_backward (CosWISS, total={total})")
    so.note(record_property, report)
