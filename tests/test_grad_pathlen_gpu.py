"""GPU tests of the differentiable path-length weighting (fruits_amd.nn.pathlen_iss,
fr_plan_set_grad_pathlen around fr_iss_backward_weighted): the forward bits, the gradient against
the long-double oracle - exactly where the lookup part vanishes, within the derived rounding bound
with real weights, dg on its own too - repeatability, the autograd wiring, the arming state and one
run on a side stream."""
import numpy as np
import pytest

import iss_bounds as ib
import iss_grad_pathlen_ref as gp
import iss_grad_ref as gr
import iss_grad_weighted_ref as gw
import stream_order as so

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 64, 65, 513, 1024, 1025, 2049, 4099)      # lanes, waves, one chunk, carries across chunks
PREFIX = ["[1]", "[1][2]", "[1][2][1]", "[2]", "[1][2]", "[11][2]"]
TWINS = ["[1][2]", "[1][2]", "[11][2][1]", "[11][2][1]", "[2]"]
W22 = gr.orc.of_weight_strings(2, 2) + ["[1][2][1]", "[11][2][2]"]


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


def weighting_of(norm, **kwargs):
    from fruits_amd.iss import weighting as wt
    return (wt.L1 if norm == 1 else wt.L2)(**kwargs)


def letters_of(s):
    return len(gr.orc.parse_word(s))


def zero_alphas(strings):
    return [np.zeros(letters_of(s), dtype=np.float32) for s in strings]


def drawn_alphas(strings, seed, pool=12):
    """One alpha per letter and word from ``pool`` values uniform in [0.25, 2], as float32."""
    rng = np.random.default_rng([seed, len(strings)])
    values = rng.uniform(0.25, 2.0, pool).astype(np.float32)
    return [rng.choice(values, letters_of(s)) for s in strings]


def device_lookup(env, Xd, norm, kwargs):
    """The lookup the device forms for ``Xd``: what the Reals forward and backward pass use."""
    from fruits_amd import _native as nat
    return nat.pathlen_lookup(Xd, norm, 1 if kwargs.get("relative", False) else 0,
                              float(kwargs.get("scale", 50)), exact=False)


def device_grad(env, X, G, strings, alphas, mode, norm, kwargs):
    """X.grad of ``(nn.pathlen_iss(X) * G).sum()`` as a host array, the forward result, and the
    lookup the device used."""
    fr, nn, torch = env
    Xd = torch.tensor(X, device="cuda").requires_grad_(True)
    op = fr.ISS(words_of(fr, strings, alphas), mode=mode_of(fr, mode), weighting=weighting_of(norm, **kwargs))
    Y = nn.pathlen_iss(Xd, op)
    Y.backward(torch.tensor(G, device="cuda"))
    return Xd.grad.cpu().numpy(), Y.detach().cpu().numpy(), device_lookup(env, Xd.detach(), norm, kwargs).cpu().numpy()


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("norm", [1, 2], ids=["l1", "l2"])
def test_forward_bits(env, norm, total, mode):
    fr, nn, torch = env
    strings = ib.WORDS + gr.orc.of_weight_strings(2, 3)
    words = words_of(fr, strings, drawn_alphas(strings, 1))
    X = np.random.default_rng(3).standard_normal((5, 3, 300))
    for kwargs in ({"total": total}, {"total": total, "relative": True, "scale": 7, "on_prepared": True}):
        w = weighting_of(norm, **kwargs)
        want = fr.ISS(words, mode=mode_of(fr, mode), weighting=w).transform(X)            # (K, N, T)
        Xd = torch.from_numpy(X).cuda()
        Y = nn.pathlen_iss(Xd, words, mode_of(fr, mode), weighting=w)
        assert Y.shape == (5, want.shape[0], 300) and Y.device == Xd.device and not Y.requires_grad
        np.testing.assert_array_equal(Y.cpu().numpy(), want.transpose(1, 0, 2))
        layer = nn.PathLengthISSLayer(words, mode_of(fr, mode), weighting=w)
        Xt = torch.from_numpy(np.ascontiguousarray(X.transpose(0, 2, 1))).cuda().transpose(1, 2)
        assert not Xt.is_contiguous()
        np.testing.assert_array_equal(layer(Xt).cpu().numpy(), want.transpose(1, 0, 2))


# ---------------------------------------------------------------- exact
_EXACT = {}


def exact_case(T, constant):
    """(X, G, want) on integers, N = 3, shared by the bodies and norms: ``want`` is the UNWEIGHTED
    oracle.  ``constant``: dimension 0 does not move."""
    key = (T, constant)
    if key not in _EXACT:
        N, D = 3, 2
        rng = np.random.default_rng([11, T, int(constant)])
        X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
        if constant:
            X[:, 0] = np.array([1.0, -2.0, 2.0])[:, None]
        K = len(gr.output_prefixes(PREFIX, "EXTENDED"))
        G = rng.integers(-3, 4, size=(N, K, T)).astype(np.float64)
        want = gr.iss_grad(X, G, PREFIX, "EXTENDED")
        assert np.abs(want).max() < 2.0 ** 50 and (want == want.astype(np.float64)).all()
        for a in (X, G, want):
            a.setflags(write=False)
        _EXACT[key] = (X, G, want.astype(np.float64))
    return _EXACT[key]


@pytest.mark.parametrize("T", LENGTHS)
def test_gradient_exact_with_alpha_zero(env, T):
    """Every alpha is 0: dg is exactly 0 and so is what the path-length kernel adds - the gradient
    is that of the unweighted iterated sums bit for bit, whatever g is."""
    X, G, want = exact_case(T, constant=False)
    for norm, total in [(1, False), (1, True), (2, False), (2, True)]:
        got, _, lookup = device_grad(env, X, G, PREFIX, zero_alphas(PREFIX), "EXTENDED", norm,
                                     {"total": total, "scale": 5})
        assert T == 1 or lookup.max() == 5.0
        np.testing.assert_array_equal(got, want, err_msg=f"T={T} norm={norm} total={total}")


@pytest.mark.parametrize("T", LENGTHS)
def test_gradient_exact_with_a_constant_first_dimension(env, T):
    """r_L = 0: g = 0, every exp factor 1.0, no lookup part - no 0 / 0, no NaN - with real alphas."""
    X, G, want = exact_case(T, constant=True)
    alphas = drawn_alphas(PREFIX, 3)
    for norm, total in [(1, False), (1, True), (2, False), (2, True)]:
        got, _, lookup = device_grad(env, X, G, PREFIX, alphas, "EXTENDED", norm, {"total": total, "scale": 5})
        assert not lookup.any()
        np.testing.assert_array_equal(got, want, err_msg=f"T={T} norm={norm} total={total}")


# ---------------------------------------------------------------- the derived bound
BOUND_CASES = {
    # (shape, words, mode, norm, weighting kwargs); scale = 5, alphas from [0.25, 2]
    "l1_1024": ((7, 3, 1024), ib.WORDS, "EXTENDED", 1, {"scale": 5}),
    "l1_total_1024": ((7, 3, 1024), ib.WORDS, "EXTENDED", 1, {"scale": 5, "total": True}),
    "l2_twins_1025": ((3, 2, 1025), TWINS, "SINGLE", 2, {"scale": 5}),
    "l2_total_twins_1025": ((3, 2, 1025), TWINS, "SINGLE", 2, {"scale": 5, "total": True, "relative": True}),
    "l1_total_4099": ((3, 2, 4099), W22, "EXTENDED", 1, {"scale": 5, "total": True}),
    "l2_4099": ((3, 2, 4099), W22, "EXTENDED", 2, {"scale": 5}),
}
_REAL = {}


def real_case(name):
    """(X, G, alphas) of a bound case: computed once, shared, never changed."""
    if name not in _REAL:
        (N, D, T), strings, mode, _, _ = BOUND_CASES[name]
        rng = np.random.default_rng([N, D, T, 7])
        X = rng.standard_normal((N, D, T))
        divided = {d for s in strings for row in gr.orc.parse_word(s) for d, e in enumerate(row) if e < 0}
        for d in sorted(set(range(D)) - divided):
            X[rng.integers(0, N, 5), d, rng.integers(0, T, 5)] = 0.0
        alphas = drawn_alphas(strings, 2)
        G = rng.standard_normal((N, len(gw.output_nodes(strings, alphas, mode)), T))
        for a in [X, G] + alphas:
            a.setflags(write=False)
        _REAL[name] = (X, G, alphas)
    return _REAL[name]


def reference(name, lookup):
    """The references of a bound case on the lookup the device used, once per case:
    (hp, A, n) of the full gradient and of dg."""
    key = (name, "ref")
    if key not in _REAL:
        (N, D, T), strings, mode, norm, kwargs = BOUND_CASES[name]
        X, G, alphas = real_case(name)
        total, scale = bool(kwargs.get("total", False)), float(kwargs["scale"])
        args = (X, G, strings, alphas, lookup, total)
        full = (gp.iss_grad_pathlen(*args, norm, scale, mode),
                gp.iss_grad_pathlen(*args, norm, scale, mode, magnitude=True),
                gp.n_ops_grad_pathlen(strings, alphas, lookup, T, mode))
        dg = (gp.iss_grad_lookup(*args, mode), gp.iss_grad_lookup(*args, mode, magnitude=True),
              gp.n_ops_grad_lookup(strings, alphas, lookup, T, mode))
        _REAL[key] = (full, dg)
    return _REAL[key]


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_gradient_and_dg_within_bound(env, name):
    """|device - R| <= 2 n 2^-53 A elementwise, for dg alone (n_ops_grad_lookup) and for the full
    gradient (n_ops_grad_pathlen), R and A on the device's own lookup."""
    fr, nn, torch = env
    from fruits_amd import _native as nat
    _, strings, mode, norm, kwargs = BOUND_CASES[name]
    X, G, alphas = real_case(name)
    assert all(0.25 <= a.min() and a.max() <= 2.0 and a.dtype == np.float32 for a in alphas)
    got, _, lookup = device_grad(env, X, G, strings, alphas, mode, norm, kwargs)
    assert lookup.max() == 5.0 and lookup.min() == 0.0
    (hp, A, n), (dg_hp, dg_A, dg_n) = reference(name, lookup)
    # the lookup part is no rounding matter: without it the gradient lies far outside
    inp = gw.iss_grad_weighted(X, G, strings, alphas, lookup, bool(kwargs.get("total", False)), mode,
                               dtype=np.float64)
    assert ib.violates(inp, hp, A, n)
    worst = ib.check_bound(got, hp, A, n, f"grad_pathlen {name}", family="grad_pathlen")
    print(f"grad_pathlen {name}: n_ops_grad_pathlen = {n}, largest err / bound = {worst:.3g}")
    # dg on its own, through the native wrapper
    op = fr.ISS(words_of(fr, strings, alphas), mode=mode_of(fr, mode), weighting=weighting_of(norm, **kwargs))
    plan, row_prefix = nn._prefix_program(op)
    Xd = torch.tensor(X, device="cuda")
    dX, dg = nat.iss_backward_weighted(plan, Xd, device_lookup(env, Xd, norm, kwargs), torch.tensor(G, device="cuda"),
                                       row_prefix, pathlen=(norm, 5.0), return_dg=True)
    np.testing.assert_array_equal(dX.cpu().numpy(), got)
    worst = ib.check_bound(dg.cpu().numpy(), dg_hp, dg_A, dg_n, f"grad_pathlen dg {name}", family="grad_pathlen_dg")
    print(f"grad_pathlen dg {name}: n_ops_grad_lookup = {dg_n}, largest err / bound = {worst:.3g}")


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("name", ["l1_1024", "l1_total_1024"])
def test_backward_is_repeatable(env, name):
    _, strings, mode, norm, kwargs = BOUND_CASES[name]
    X, G, alphas = real_case(name)
    first, _, _ = device_grad(env, X, G, strings, alphas, mode, norm, kwargs)
    again, _, _ = device_grad(env, X, G, strings, alphas, mode, norm, kwargs)
    np.testing.assert_array_equal(first, again)
    parts = [device_grad(env, np.ascontiguousarray(X[s]), np.ascontiguousarray(G[s]), strings, alphas,
                         mode, norm, kwargs)[0] for s in (slice(0, 3), slice(3, 7))]
    np.testing.assert_array_equal(np.concatenate(parts), first)


# ---------------------------------------------------------------- autograd
def kink_free(torch, N, D, T, seed):
    """Standard normal X whose dimension 0 moves by at least 0.25 per step."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D, T))
    X[:, 0] = np.cumsum(rng.uniform(0.25, 1.0, (N, T)) * rng.choice([-1.0, 1.0], (N, T)), axis=1)
    return torch.from_numpy(X).cuda().requires_grad_(True)


@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
@pytest.mark.parametrize("norm", [1, 2], ids=["l1", "l2"])
@pytest.mark.parametrize("string, alpha", [("[1][2]", [0.5, 1.5]), ("[11][2][1]", [1.25, 0.25, 2.0])])
def test_gradcheck(env, string, alpha, norm, total):
    fr, nn, torch = env
    X = kink_free(torch, 2, 2, 9, seed=11)
    words = words_of(fr, [string], [alpha])
    w = weighting_of(norm, scale=2, total=total)
    assert torch.autograd.gradcheck(lambda x: nn.pathlen_iss(x, words, weighting=w), (X,))
    assert torch.autograd.gradcheck(nn.PathLengthISSLayer(words, fr.ISSMode.EXTENDED, weighting=w), (X,))


def test_strided_upstream_gradient(env):
    """Y[:, :, -1].sum(): the upstream gradient reaches the backward pass - the dg gather too - with
    strides of its own; Y.sum(): all strides 0."""
    fr, nn, torch = env
    strings, N, D, T = ib.WORDS, 3, 3, 700
    alphas = drawn_alphas(strings, 6)
    X = np.random.default_rng(1).standard_normal((N, D, T))
    K = len(gw.output_nodes(strings, alphas, "EXTENDED"))
    for total in (False, True):
        for pick, G in ((lambda Y: Y[:, :, -1].sum(), np.zeros((N, K, T))), (lambda Y: Y.sum(), np.ones((N, K, T)))):
            if not G.any():
                G[:, :, -1] = 1.0
            kwargs = {"scale": 4.0, "total": total}
            op = fr.ISS(words_of(fr, strings, alphas), mode=fr.ISSMode.EXTENDED, weighting=weighting_of(1, **kwargs))
            Xd = torch.from_numpy(X).cuda().requires_grad_(True)
            pick(nn.pathlen_iss(Xd, op)).backward()
            lookup = device_lookup(env, Xd.detach(), 1, kwargs).cpu().numpy()
            args = (X, G, strings, alphas, lookup, total, 1, 4.0, "EXTENDED")
            ib.check_bound(Xd.grad.cpu().numpy(), gp.iss_grad_pathlen(*args), gp.iss_grad_pathlen(*args, magnitude=True),
                           gp.n_ops_grad_pathlen(strings, alphas, lookup, T, "EXTENDED"), "strided G")


def test_gradients_accumulate_and_none_without_requires_grad(env):
    fr, nn, torch = env
    X, _, _ = exact_case(65, constant=False)
    layer = nn.PathLengthISSLayer(words_of(fr, PREFIX, drawn_alphas(PREFIX, 5)), fr.ISSMode.EXTENDED,
                                  weighting=weighting_of(2, scale=2.0))
    Xd = torch.from_numpy(X.copy()).cuda().requires_grad_(True)
    G = torch.ones((3, len(gr.output_prefixes(PREFIX, "EXTENDED")), 65), dtype=torch.float64, device="cuda")
    before = nn.backward_calls()
    layer(Xd).backward(G)
    once = Xd.grad.clone()
    layer(Xd).backward(G)
    assert nn.backward_calls() == before + 2
    assert torch.equal(Xd.grad, 2 * once) and once.abs().max() > 0
    Y = layer(Xd.detach())
    assert not Y.requires_grad and Y.grad_fn is None
    with torch.no_grad():
        assert not layer(Xd).requires_grad
    assert nn.backward_calls() == before + 2
    # only X is kept for the backward pass: the lookup is formed again
    Y = layer(Xd)
    assert [t.data_ptr() for t in Y.grad_fn.saved_tensors] == [Xd.data_ptr()]
    # the functional form keeps its ISS between calls
    w = weighting_of(1)
    words = words_of(fr, PREFIX)
    nn.pathlen_iss(Xd.detach(), words, weighting=w)
    kept = [op for op in nn._OPS.values() if op.weighting is w]
    nn.pathlen_iss(Xd.detach(), words, weighting=w)
    assert len(kept) == 1 and [op for op in nn._OPS.values() if op.weighting is w] == kept


# ---------------------------------------------------------------- the arming state
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_unarmed_and_cleared_plans_keep_their_bits(env, total):
    fr, nn, torch = env
    from fruits_amd import _native as nat
    N, D, T = 3, 2, 1030
    alphas = drawn_alphas(TWINS, 9)
    rng = np.random.default_rng(13)
    X, G = rng.standard_normal((N, D, T)), rng.standard_normal((N, len(TWINS), T))
    Xd, Gd = torch.tensor(X, device="cuda"), torch.tensor(G, device="cuda")
    lookup = device_lookup(env, Xd, 1, {"scale": 5})
    make = lambda: nn._prefix_program(fr.ISS(words_of(fr, TWINS, alphas), weighting=weighting_of(1, total=total)))  # noqa: E731
    plan, rows = make()
    unarmed = nat.iss_backward_weighted(plan, Xd, lookup, Gd, rows).cpu().numpy()
    armed = nat.iss_backward_weighted(plan, Xd, lookup, Gd, rows, pathlen=(1, 5.0)).cpu().numpy()
    assert np.array_equal(armed[:, 1], unarmed[:, 1]) and not np.array_equal(armed[:, 0], unarmed[:, 0])
    # armed, then cleared (the wrapper clears behind its call): the bits of before, and of a plan
    # that was never armed
    np.testing.assert_array_equal(nat.iss_backward_weighted(plan, Xd, lookup, Gd, rows).cpu().numpy(), unarmed)
    fresh, fresh_rows = make()
    assert fresh is not plan
    np.testing.assert_array_equal(nat.iss_backward_weighted(fresh, Xd, lookup, Gd, fresh_rows).cpu().numpy(), unarmed)
    # the armed entry wants a lookup row per series
    with pytest.raises(ValueError, match="the lookup has to have N rows"):
        nat.iss_backward_weighted(plan, Xd, lookup[:1].contiguous(), Gd, rows, pathlen=(1, 5.0))
    np.testing.assert_array_equal(nat.iss_backward_weighted(plan, Xd, lookup, Gd, rows).cpu().numpy(), unarmed)


# ---------------------------------------------------------------- a side stream
@pytest.mark.parametrize("total", [False, True], ids=["nontotal", "total"])
def test_armed_entry_follows_the_callers_stream(env, record_property, total):
    """The armed fr_iss_backward_weighted behind an unfinished producer on a side stream: the lookup,
    the two new kernels and the dg scratch follow that stream - dX and dg bit for bit those of the
    default-stream run."""
    fr, nn, torch = env
    from fruits_amd import _native as nat
    N, D, T = 5, 2, 1500
    alphas = drawn_alphas(TWINS, 9)
    plan, rows = nn._prefix_program(fr.ISS(words_of(fr, TWINS, alphas), weighting=weighting_of(2, total=total)))
    rng = np.random.default_rng(17)
    true = [rng.standard_normal((N, D, T)), rng.standard_normal((N, len(TWINS), T))]
    wrong = [rng.standard_normal((N, D, T)), rng.standard_normal((N, len(TWINS), T))]

    def call(Xd, Gd):
        lookup = nat.pathlen_lookup(Xd, 2, 0, 5.0, exact=False)
        return nat.iss_backward_weighted(plan, Xd, lookup, Gd, rows, pathlen=(2, 5.0), return_dg=True)

    want, report = so.behind_producer(call, true, wrong, what=f"armed fr_iss_backward_weighted total={total}")
    so.note(record_property, report)
    assert np.abs(want[1]).max() > 0
