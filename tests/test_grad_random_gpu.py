"""Random differential tests of the backward pass, all five adjoints (fruits_amd.nn: fr_iss_backward,
fr_iss_backward_max, fr_iss_backward_weighted, fr_iss_backward_picked, fr_sieve_pick) on the
random cases of tests/grad_random.py: the forward bits and the gradient against the long-double
oracles - bit for bit where every sum is exact, within the derived rounding bounds on real-valued
inputs -, the sparse upstream of picked features against the dense one, and repeatability.

``FRUITS_TEST_RANDOM_CASES`` sets the number of seeds (a soak: 200)."""
import os

import numpy as np
import pytest

import features_grad_ref as fg
import grad_random as rnd
import iss_bounds as ib
import iss_grad_max_ref as gm
import iss_grad_ref as gr
import iss_grad_weighted_ref as gw

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("FRUITS_TEST_RANDOM_CASES", str(rnd.DEFAULT_SEEDS))))
SEMIRING = {"arctic": "Arctic", "bayesian": "Bayesian"}
FAMILY = {"reals": "grad", "arctic": "grad_max_Arctic", "bayesian": "grad_max_Bayesian",
          "nontotal": "grad_weighted", "total": "grad_weighted"}
TIES = {"arctic": [], "bayesian": []}      # per exact case of T >= 63: whether it has an exact tie
_OPS = {}
_EXACT_REF = {}


@pytest.fixture(scope="module")
def env():
    import torch
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    nat.require_device()
    yield fr, nn, torch
    ib.print_ratios()
    for kind, ties in TIES.items():
        print(f"grad_random {kind}: {sum(ties)} of {len(ties)} exact cases of T >= 63 have exact ties")
    _OPS.clear()


def make_op(fr, c, kind, zero):
    """The ISS of a kind on the words of a case; the weighted kinds with the case's alphas, or
    with zeros.  Kept while the case's tests run (the tests run seed by seed): a case meets the same
    device programs and tables in all of them."""
    key = (c.seed, c.strings, c.mode, kind, zero)
    if key not in _OPS:
        words = [fr.words.SimpleWord(s) for s in c.strings]
        kw = {}
        if kind in SEMIRING:
            kw["semiring"] = getattr(fr.semiring, SEMIRING[kind])()
        if kind in ("nontotal", "total"):
            from fruits_amd.iss.weighting import Indices
            kw["weighting"] = Indices(total=kind == "total")
            for w, a in zip(words, c.zero_alphas() if zero else c.alpha_arrays()):
                w.alpha = a
        mode = fr.ISSMode.EXTENDED if c.mode == "EXTENDED" else fr.ISSMode.SINGLE
        rnd.keep(_OPS, key, fr.ISS(words, mode=mode, **kw), most=10)
    return _OPS[key]


def dense_entry(nn, kind):
    return {"reals": nn.iss, "arctic": nn.max_iss, "bayesian": nn.max_iss}.get(kind, nn.weighted_iss)


def device_grad(env, op, kind, X, G):
    """(X.grad of ``(rows(X) * G).sum()``, the rows (N, K, T), the lookup the device used or None),
    as host arrays."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)       # (copies: the shared inputs are read-only)
    Y = dense_entry(nn, kind)(Xd, op)
    Y.backward(torch.tensor(G, device="cuda"))
    lookup = op.lookup_device(Xd).cpu().numpy() if op.weighting is not None else None
    return Xd.grad.cpu().numpy(), Y.detach().cpu().numpy(), lookup


def oracle_rows(c, X, kind):
    """The oracle's rows in the layout of fruits_amd.nn, (N, K, T); the weighted kinds at alpha 0."""
    return gr.orc.iss_transform(X, list(c.strings), c.mode, semiring=SEMIRING.get(kind, "Reals")).transpose(1, 0, 2)


def exact_reference(c, kind):
    """(gradient in long double, rows) of the exact inputs of a case: once per group of kinds."""
    key = (c.seed, rnd.GROUP[kind])
    if key not in _EXACT_REF:
        e = rnd.exact_inputs(c, kind)
        if kind in SEMIRING:
            want = gm.iss_grad_max(e.X, e.G, list(c.strings), c.mode, SEMIRING[kind])
        else:
            want = gr.iss_grad(e.X, e.G, list(c.strings), c.mode)
        rnd.keep(_EXACT_REF, key, (want, oracle_rows(c, e.X, kind)))
    return _EXACT_REF[key]


def is_exact(want):
    return bool(np.abs(want).max(initial=0) < 2.0 ** 50 and (want == want.astype(np.float64)).all())


def held_to_bound(got, hp, A, n, kind, what):
    try:
        return ib.check_bound(got, hp, A, n, f"grad_random {kind}", family=FAMILY[kind])
    except AssertionError as err:
        raise AssertionError(f"{err} {what}") from None


# ---------------------------------------------------------------- exact
def check_exact(env, c, kind):
    e = rnd.exact_inputs(c, kind)
    what = f"{kind} exact T={e.T} {c.describe()}"
    got, Y, lookup = device_grad(env, make_op(env[0], c, kind, True), kind, e.X, e.G)
    want, rows = exact_reference(c, kind)
    assert is_exact(want), what
    if lookup is not None:
        assert e.T == 1 or lookup.max() == 50.0, what      # (a real lookup: alpha = 0 makes it exact)
    np.testing.assert_array_equal(Y, rows, err_msg=what)
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=what)
    if kind in SEMIRING and e.T >= 63:
        TIES[kind].append(gm.smallest_gap(e.X, list(c.strings), c.mode, SEMIRING[kind]) == 0.0)


@pytest.mark.parametrize("kind", rnd.KINDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_random_exact(env, kind, seed):
    """Inputs on which every partial sum is exact (``grad_random.exact_inputs`` carries the proof):
    the rows and the gradient are the oracle's, bit for bit - whatever the order of the additions."""
    check_exact(env, rnd.case(seed), kind)


# ---------------------------------------------------------------- the derived bound
@pytest.mark.parametrize("kind", rnd.KINDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_random_within_bound(env, kind, seed):
    """|device - oracle| <= 2 n_ops 2^-53 oracle(magnitude=True) elementwise, with the counts
    ``n_ops_grad``, ``n_ops_grad_max`` and ``n_ops_grad_weighted`` as they stand."""
    c = rnd.case(seed)
    what = f"{kind} {c.describe()}"
    strings = list(c.strings)
    X, G, alphas = rnd.real_inputs(c, kind)
    got, Y, lookup = device_grad(env, make_op(env[0], c, kind, False), kind, X, G)
    if kind in SEMIRING:
        # the precondition for shared heads: the forward bits are the oracle's
        np.testing.assert_array_equal(Y, oracle_rows(c, X, kind), err_msg=what)
        hp = gm.iss_grad_max(X, G, strings, c.mode, SEMIRING[kind])
        A = gm.iss_grad_max(X, G, strings, c.mode, SEMIRING[kind], magnitude=True)
        n = gm.n_ops_grad_max(strings, c.T, c.mode, SEMIRING[kind])
    elif kind == "reals":
        hp = gr.iss_grad(X, G, strings, c.mode)
        A = gr.iss_grad(X, G, strings, c.mode, magnitude=True)
        n = gr.n_ops_grad(strings, c.T, c.mode)
    else:
        # on the lookup the device used
        total = kind == "total"
        hp = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, c.mode)
        A = gw.iss_grad_weighted(X, G, strings, alphas, lookup, total, c.mode, magnitude=True)
        n = gw.n_ops_grad_weighted(strings, alphas, lookup, c.T, c.mode)
    worst = held_to_bound(got, hp, A, n, kind, what)
    print(f"grad_random {kind} seed {seed}: n_ops = {n}, largest err / bound = {worst:.3g}")


# ---------------------------------------------------------------- picked features
def sieve_objects(specs):
    from fruits_amd import sieving
    return [getattr(sieving, name)(list(cuts)) if q is None else getattr(sieving, name)(list(cuts), q=q)
            for name, cuts, q in specs]


def features_grad(env, op, X, g, sieves):
    """(features (N, K * F), positions (N, K, F), X.grad) of ``(iss_features(X) * g).sum()``."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    feats = nn.iss_features(Xd, op, sieves=sieves)
    saved = feats.grad_fn.saved_tensors
    assert len(saved) == 2 and saved[1].dtype == torch.int32
    pos = saved[1].cpu().numpy()
    feats.backward(torch.tensor(g, device="cuda").view(feats.shape))
    return feats.detach().cpu().numpy(), pos, Xd.grad.cpu().numpy()


def check_picked(env, c, kind, specs):
    fr, nn, torch = env
    what = f"{kind} picked {specs} {c.describe()}"
    refs, sieves = rnd.reference_specs(specs), sieve_objects(specs)
    K, F, T = len(rnd.rows_of(c)), rnd.nfeatures(specs), c.T
    g = np.random.default_rng([2026, c.seed, 8, F]).integers(-3, 4, size=(c.N, K * F)).astype(np.float64)
    X, _, _ = rnd.real_inputs(c, kind)
    op = make_op(fr, c, kind, False)
    feats, pos, got = features_grad(env, op, X, g, sieves)
    assert feats.shape == (c.N, K * F) and pos.shape == (c.N, K, F), what
    # positions and feature bits: the reference's selection on the device's own rows
    rows = op.transform_device(torch.tensor(X, device="cuda")).cpu().numpy().transpose(1, 0, 2)
    ref_feats, ref_pos = fg.pick(rows, refs)
    np.testing.assert_array_equal(pos, ref_pos, err_msg=what)
    np.testing.assert_array_equal(feats.reshape(c.N, K, F), ref_feats, err_msg=what)
    # integer feature gradients: every b is a sum of integers, so the sparse route has the bits
    # of the dense entry on the scattered gradient
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    dense_entry(nn, kind)(Xd, op).backward(torch.tensor(fg.dense_upstream(pos, g, T), device="cuda"))
    np.testing.assert_array_equal(got, Xd.grad.cpu().numpy(), err_msg=what)
    assert np.isfinite(got).all(), what


def check_exact_picked(env, c, short):
    fr, nn, torch = env
    kind, specs = "reals", rnd.sieves_of(short)
    e = rnd.exact_inputs(c, kind)
    what = f"{kind} picked exact T={e.T} {specs} {c.describe()}"
    refs, sieves = rnd.reference_specs(specs), sieve_objects(specs)
    K, F = len(rnd.rows_of(c)), rnd.nfeatures(specs)
    g = np.random.default_rng([2026, c.seed, 9, F]).integers(-3, 4, size=(c.N, K * F)).astype(np.float64)
    ref_feats, ref_pos = fg.pick(oracle_rows(c, e.X, kind), refs)
    feats, pos, got = features_grad(env, make_op(fr, c, kind, True), e.X, g, sieves)
    np.testing.assert_array_equal(pos, ref_pos, err_msg=what)
    np.testing.assert_array_equal(feats.reshape(c.N, K, F), ref_feats, err_msg=what)
    upstream = fg.dense_upstream(ref_pos, g, e.T)
    # the scattered upstream sums coinciding features: the proof of exactness, taken again for it
    assert max(rnd.magnitudes(short, "reals", e.X, upstream)) * 2.0 ** e.q <= 2.0 ** 53, what
    want = gr.iss_grad(e.X, upstream, list(c.strings), c.mode)
    assert is_exact(want), what
    np.testing.assert_array_equal(got, want.astype(np.float64), err_msg=what)


@pytest.mark.parametrize("kind", rnd.KINDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_random_picked(env, kind, seed):
    """END, MAX and MIN heads drawn from the seed on the rows of the case: positions, feature
    bits, and the sparse upstream against the dense one - for Reals against the oracle too."""
    c = rnd.case(seed)
    check_picked(env, c, kind, rnd.sieves_of(c))
    if kind == "reals":
        # (the exact inputs may be shorter than the case: their sieves are those of that length)
        check_exact_picked(env, c, rnd.exact_inputs(c, kind).case(c))


@pytest.mark.parametrize("kind", rnd.KINDS)
def test_picked_with_256_features(env, kind):
    """Exactly the 256 features a row may have (csrc/kernels.h, kPickMaxFeatures)."""
    c = rnd.with_shape(rnd.case(0), 3, 300)
    specs = rnd.full_sieves(c.T)
    assert rnd.nfeatures(specs) == 256
    check_picked(env, c, kind, specs)


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("kind", rnd.KINDS)
def test_random_repeatable(env, kind):
    """A second run gives the same bits; so does the batch in two launches - another grid."""
    for seed in SEEDS[:8]:
        c = rnd.case(seed)
        what = f"{kind} {c.describe()}"
        X, G, _ = rnd.real_inputs(c, kind)
        op = make_op(env[0], c, kind, False)
        first, _, _ = device_grad(env, op, kind, X, G)
        again, _, _ = device_grad(env, op, kind, X, G)
        np.testing.assert_array_equal(first, again, err_msg=what)
        if c.N < 2:
            continue
        cut = (c.N + 1) // 3 or 1
        parts = [device_grad(env, op, kind, np.ascontiguousarray(X[s]), np.ascontiguousarray(G[s]))[0]
                 for s in (slice(0, cut), slice(cut, c.N))]
        np.testing.assert_array_equal(np.concatenate(parts), first, err_msg=what)
