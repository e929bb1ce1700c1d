"""GPU tests of generic words: the two streaming kernels (fr_letter_rows, fr_rows_unshift)
against numpy, bit for bit; the ISS of generic words against the reference's recorded outputs
(tests/golden/golden_words.npz) and against the restatement tests/words_ref.py; and fruits whose
ISS holds generic words.

Tolerance of the iterated sums: the project's bar as test_hip_parity.py applies it -
max|delta| <= 1e-6 * max|ref| per (k, n) row, plus elementwise rtol = 1e-6 on the U[0, 1) Reals
cases.  The leading p - 1 positions of the row of a generic prefix of length p are exactly 0.0
for Reals and Bayesian (Arctic's slow path does not shift: words_ref.py).
"""
import json
import os

import numpy as np
import pytest

import words_ref as wref
from conftest import GOLDEN_DIR, gen_input
from oracle import ref_numpy as orc

pytestmark = pytest.mark.gpu

ARR = np.load(os.path.join(GOLDEN_DIR, "golden_words.npz"))
with open(os.path.join(GOLDEN_DIR, "golden_words.json")) as f:
    MAN = json.load(f)
RTOL = 1e-6

# (tests/golden/make_golden_words.py: lengths 1, 2, 3 and 5, shared prefixes, an empty extended
# letter, custom letters)
WORDS = ["[ABS(1)DIM(2)][ABS(1)]", "[ABS(1)DIM(2)][DIM(3)][DIM(1)DIM(1)]", "[DIM(2)]",
         "[ABS(1)DIM(2)][ABS(1)][ReLU(2)][DIM(3)][ABS(2)]", "[DIM(1)][][DIM(2)]",
         "[SQ(3)ReLU(1)][ABS(2)]"]


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    wref.register(fruits_amd)
    return fruits_amd


@pytest.fixture(scope="module")
def nat(fr):
    from fruits_amd import _native
    return _native


def rowwise_close(got, ref, rtol=RTOL):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    flat_g = got.reshape(-1, got.shape[-1])
    flat_r = ref.reshape(-1, ref.shape[-1])
    scale = np.max(np.abs(flat_r), axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    err = np.max(np.abs(flat_g - flat_r) / scale)
    assert err <= rtol, f"row-wise relative error {err:.3e} > {rtol}"
    return err


def x_of(spec):
    return gen_input(spec) + spec.get("offset", 0.0)


def make_word(fr, s):
    return fr.words.Word(s) if wref.is_generic(s) else fr.words.SimpleWord(s)


def make_iss(fr, case):
    words = [make_word(fr, s) for s in case["words"]]
    for w, a in zip(words, case.get("alphas") or []):
        if a is not None:
            w.alpha = a
    weighting = None
    if case.get("weighting") is not None:
        kw = {k: v for k, v in case["weighting"].items() if k != "kind"}
        weighting = getattr(fr.iss.weighting, case["weighting"]["kind"])(**kw)
    return fr.ISS(words, mode=getattr(fr.ISSMode, case["mode"]),
                  semiring=getattr(fr.semiring, case["semiring"])(), weighting=weighting)


def assert_heads_zero(out, words, mode, semiring):
    heads = wref.head_lengths(words, mode, semiring)
    depths = wref.cache_plan(words) if mode == "EXTENDED" else [1] * len(words)
    generic = [wref.is_generic(s) for s, d in zip(words, depths) for _ in range(d)]
    assert len(heads) == out.shape[0]
    for k, head in enumerate(heads):
        if generic[k] and head:
            assert np.all(out[k][:, :head] == 0.0), (k, head)


# ---------------------------------------------------------------- the two kernels, bit for bit
def rows_ref(X, ext, spec, one):
    N, _, T = X.shape
    V = np.zeros((N, len(spec), T))
    for r, (kind, src, shift) in enumerate(spec):
        if kind == 3:
            base = np.full((N, T), one)
        elif kind == 2:
            base = ext[:, src]
        else:
            base = X[:, src] if kind == 0 else np.abs(X[:, src])
        if shift < T:
            V[:, r, :T - shift] = base[:, shift:]
    return V


@pytest.mark.parametrize("H", [0, 2])
@pytest.mark.parametrize("T", [1, 2, 5, 63, 64, 65, 257, 2051])
def test_letter_rows_kernel(nat, T, H):
    rng = np.random.default_rng(1000 * T + H)
    N, D = 3, 3
    X = rng.standard_normal((N, D, T))
    X[0, 0, 0] = -0.0
    ext = rng.standard_normal((N, H, T)) if H else None
    shifts = sorted({0, 1, 3, max(T - 1, 0), T, T + 2})
    kinds = [0, 1, 3] + ([2] if H else [])
    spec = [(k, (s + k) % (H if k == 2 else D), s) for k in kinds for s in shifts]
    Xd = nat.to_device(X)
    ext_d = nat.to_device(ext) if H else None
    for one_is_zero in (False, True):
        got = nat.to_host(nat.letter_rows(Xd, spec, ext_d, one_is_zero=one_is_zero))
        ref = rows_ref(X, ext, spec, 0.0 if one_is_zero else 1.0)
        assert got.shape == (N, len(spec), T)
        np.testing.assert_array_equal(got, ref)
    # the padding is +0.0 and fabs gives +0.0; a copied -0.0 keeps its sign
    plain = nat.to_host(nat.letter_rows(Xd, [(0, 0, 0), (1, 0, 0), (0, 0, T)], None))
    assert np.signbit(plain[0, 0, 0]) and not np.signbit(plain[0, 1, 0])
    assert not np.signbit(plain[:, 2]).any()
    # a view that starts 8 bytes off a 16-byte boundary: the 8-byte path
    if T % 2 == 0:
        t = nat.torch()
        flat = t.zeros(N * D * T + 1, dtype=t.float64, device=Xd.device)
        off = flat[1:].view(N, D, T)
        off.copy_(Xd)
        some = spec[:len(shifts) * 2]
        got = nat.to_host(nat.letter_rows(off, some, None))
        np.testing.assert_array_equal(got, rows_ref(X, None, some, 1.0))
        # ... and an OUTPUT that starts 8 bytes off: the 8-byte stores, aligned input or not
        for src in (Xd, off):
            guard = t.full((N * len(some) * T + 2,), 7.0, dtype=t.float64, device=Xd.device)
            out = guard[1:-1].view(N, len(some), T)
            assert out.data_ptr() % 16 == 8
            nat.letter_rows(src, some, None, out=out)
            np.testing.assert_array_equal(nat.to_host(out), rows_ref(X, None, some, 1.0))
            assert guard[0].item() == 7.0 and guard[-1].item() == 7.0


@pytest.mark.parametrize("T", [1, 2, 5, 63, 64, 65, 257, 2051])
def test_rows_unshift_kernel(nat, T):
    rng = np.random.default_rng(T)
    shifts = sorted({0, 1, 2, 3, max(T - 1, 0), T, T + 2})
    K, N = len(shifts), 3
    A = rng.standard_normal((K, N, T))
    ref = np.zeros_like(A)
    for k, s in enumerate(shifts):
        if s < T:
            ref[k, :, s:] = A[k, :, :T - s]
    Ad = nat.to_device(A)
    got = nat.to_host(nat.rows_unshift(Ad, shifts))
    np.testing.assert_array_equal(got, ref)
    for k, s in enumerate(shifts):      # the head is +0.0
        assert not np.signbit(got[k, :, :min(s, T)]).any()
    if T % 2 == 0:
        # an input and / or an output that starts 8 bytes off a 16-byte boundary (even T: every
        # row is then misaligned): the 8-byte loads and stores
        t = nat.torch()
        flat = t.zeros(K * N * T + 1, dtype=t.float64, device=Ad.device)
        A_off = flat[1:].view(K, N, T)
        A_off.copy_(Ad)
        np.testing.assert_array_equal(nat.to_host(nat.rows_unshift(A_off, shifts)), ref)
        for src in (Ad, A_off):
            guard = t.full((K * N * T + 2,), 7.0, dtype=t.float64, device=Ad.device)
            out = guard[1:-1].view(K, N, T)
            assert out.data_ptr() % 16 == 8
            nat.rows_unshift(src, shifts, out=out)
            np.testing.assert_array_equal(nat.to_host(out), ref)
            assert guard[0].item() == 7.0 and guard[-1].item() == 7.0
    with pytest.raises(ValueError, match="null or aliased"):
        nat.rows_unshift(Ad, shifts, out=Ad)
    with pytest.raises(ValueError, match="negative shift"):
        nat.rows_unshift(Ad, [-1] * K)


# ---------------------------------------------------------------- ISS against the goldens
@pytest.mark.parametrize("case", MAN["iss"], ids=lambda c: c["name"])
def test_iss_golden(fr, case):
    X = x_of(case["x_gen"])
    iss = make_iss(fr, case)
    out = iss.fit_transform(X)
    ref = ARR[case["out"]]
    assert out.shape == ref.shape == (case["K"], X.shape[0], X.shape[2])
    assert [iss.label(i) for i in range(iss.n_iterated_sums())] == case["labels"]
    err = rowwise_close(out, ref)
    print(f"[words] {case['name']}: row-wise error {err:.2e}")
    if case["semiring"] == "Reals" and case["x_gen"]["dist"] == "uniform":
        np.testing.assert_allclose(out, ref, rtol=RTOL)
    assert_heads_zero(out, case["words"], case["mode"], case["semiring"])


def test_reference_test_general_scenarios(fr):
    """The two scenarios of the reference's tests/signature/test_general.py through fruits_amd:
    its X_1 next to the numbers it expects, and slow path = fast path for two simple words
    spelled with custom letters that pick a dimension (data: golden_words.json, "literal")."""
    x1 = MAN["literal"]["x1"]
    mix = fr.ISS([make_word(fr, s) for s in x1["words"]]).fit_transform(ARR[x1["x"]])
    np.testing.assert_allclose(mix, ARR[x1["expected"]])
    np.testing.assert_allclose(mix, ARR[x1["out"]])
    # the same word, assembled from extended letters on a word whose string names none
    built = fr.words.Word("no brackets")
    for body in ("ReLU(1)", "ReLU(2)"):
        built.multiply(fr.words.ExtendedLetter(body))
    assert str(built) == x1["words"][0]
    again = fr.ISS([built, make_word(fr, x1["words"][1])]).fit_transform(ARR[x1["x"]])
    np.testing.assert_array_equal(again, mix)

    fs = MAN["literal"]["fast_slow"]
    bare, named = fs["letters"]
    have = fr.words.letters.get_available()
    if bare not in have:           # the decorator's bare form takes the function's name
        def picker(X, i):
            return X[i, :]
        picker.__name__ = bare
        fr.words.letter(picker)
    if named not in have:
        fr.words.letter(name=named)(lambda X, i: X[i, :])
    slow_words = [fr.words.Word(s) for s in fs["strings"]]
    X = gen_input(fs["x_gen"])
    fast = fr.ISS([fr.words.SimpleWord(s) for s in fs["simple"]]).fit_transform(X)
    slow = fr.ISS(slow_words).fit_transform(X)
    np.testing.assert_allclose(slow, fast)
    np.testing.assert_allclose(slow, ARR[fs["slow"]], rtol=RTOL)
    np.testing.assert_allclose(fr.ISS([w.copy() for w in slow_words]).fit_transform(X), slow)
    # replace_letters spells the simple words the same way
    respelled = [fr.words.replace_letters(fr.words.SimpleWord(s), iter([n] * 99))
                 for s, n in zip(fs["simple"], fs["letters"])]
    assert [str(w) for w in respelled] == fs["strings"]


# ---------------------------------------------------------------- ISS against the restatement
REF_CACHE = {}


def reference(semiring, dist, T, mode):
    key = (semiring, dist, T, mode)
    if key not in REF_CACHE:
        spec = {"dist": "uniform", "seed": 300 + T, "shape": [4, 3, T]}
        if dist == "normal":
            spec["dist"] = "normal"
        elif dist == "uniform05":
            spec["offset"] = 0.5
        X = x_of(spec)
        ref = wref.iss_transform(X, WORDS, mode, semiring)
        X.setflags(write=False)
        ref.setflags(write=False)
        REF_CACHE[key] = (X, ref)
    return REF_CACHE[key]


CASES = [(s, d) for s in ("Reals", "Arctic") for d in ("uniform", "normal")] + [("Bayesian", "uniform05")]


@pytest.mark.parametrize("mode", ["SINGLE", "EXTENDED"])
@pytest.mark.parametrize("T", [5, 64, 65, 257, 1100, 4100])
@pytest.mark.parametrize("semiring,dist", CASES)
def test_iss_against_words_ref(fr, semiring, dist, T, mode):
    X, ref = reference(semiring, dist, T, mode)
    iss = fr.ISS([fr.words.Word(s) for s in WORDS], mode=getattr(fr.ISSMode, mode),
                 semiring=getattr(fr.semiring, semiring)())
    out = iss.fit_transform(np.array(X))
    err = rowwise_close(out, ref)
    print(f"[words] {semiring} {dist} T={T} {mode}: row-wise error {err:.2e}")
    if semiring == "Reals" and dist == "uniform":
        np.testing.assert_allclose(out, ref, rtol=RTOL)
    assert_heads_zero(out, WORDS, mode, semiring)


@pytest.mark.parametrize("semiring,dist", [("Reals", "normal"), ("Arctic", "normal"), ("Bayesian", "uniform05")])
def test_batches_and_index_subsets(fr, nat, semiring, dist):
    X, ref = reference(semiring, dist, 65, "EXTENDED")
    X = np.array(X)
    iss = fr.ISS([fr.words.Word(s) for s in WORDS], mode=fr.ISSMode.EXTENDED,
                 semiring=getattr(fr.semiring, semiring)())
    for batch_size in (1, 4):
        parts = list(iss.batch_transform(X, batch_size=batch_size))
        assert len(parts) == -(-len(WORDS) // batch_size)
        rowwise_close(np.concatenate(parts, axis=0), ref)
    depths = wref.cache_plan(WORDS)
    first = np.concatenate([[0], np.cumsum(depths)])
    order = (5, 1, 3, 0)
    got = nat.to_host(iss.transform_device(nat.to_device(X), indices=order))
    want = np.concatenate([ref[first[i]:first[i + 1]] for i in order], axis=0)
    rowwise_close(got, want)


def test_argmax_with_generic_words_raises(fr):
    iss = fr.ISS([fr.words.Word("[DIM(1)][ABS(1)]")], mode=fr.ISSMode.EXTENDED,
                 semiring=fr.semiring.Arctic(argmax=True))
    with pytest.raises(NotImplementedError, match="slow path"):
        iss.fit_transform(np.random.default_rng(0).random((2, 1, 8)))


def test_bad_letter_and_missing_dimension(fr):
    X = np.random.default_rng(0).random((2, 2, 8))
    with pytest.raises(IndexError, match="references dimension 3"):
        fr.ISS([fr.words.Word("[DIM(3)]")]).fit_transform(X)
    if "gpu_test_scalar" not in fr.words.letters.get_available():
        @fr.words.letter(name="gpu_test_scalar")
        def scalar(X, i):
            return X[i, :].sum()
    with pytest.raises(ValueError, match="one value per time step"):
        fr.ISS([fr.words.Word("[gpu_test_scalar(1)]")]).fit_transform(X)


# ---------------------------------------------------------------- fruits
# (no ReLU here: its exact zeros are summands that sit ON the threshold 0 of the default sieves)
SLICE_WORDS = ["[ABS(1)][DIM(2)]", "[DIM(1)DIM(2)]", "[ABS(2)]", "[ABS(1)][SQ(2)ABS(1)]"]


def slice_input(semiring):
    """Inputs on which the reference restatement alone shows no threshold tie: the default
    sieves ask ``0 < increment``.  Reals: normal data, the increments of a sum are its summands.
    Arctic / Bayesian: a ramp whose increments grow, so every running maximum grows by a margin
    at every step (no plateau)."""
    rng = np.random.default_rng(79)     # (77, 78: one summand of the last word within 1e-10 of 0)
    N, D, T = 6, 2, 130
    if semiring == "Reals":
        return rng.standard_normal((N, D, T))
    t = np.arange(T, dtype=np.float64)
    return 0.01 * t * t + 0.3 * t + 1e-3 * rng.random((N, D, T))


def oracle_features(X, semiring, words):
    P = orc.inc_transform(X, 1, 1, False)
    its = wref.iss_transform(P, words, "EXTENDED", semiring)
    cols, expo = [], []
    for row in its:
        for kind in ("NPI", "MPI", "END"):
            sv = orc.SieveOracle(kind)
            cols.append(sv.transform(row, X))
            expo.append(sv.exposure(row, X))
    return np.nan_to_num(np.concatenate(cols, axis=1)), np.concatenate(expo, axis=1)


def build_slice(fr, semiring):
    fruit = fr.Fruit("generic words")
    fruit.add(fr.preparation.INC(zero_padding=False))
    fruit.add(fr.ISS([fr.words.Word(s) for s in SLICE_WORDS], mode=fr.ISSMode.EXTENDED,
                     semiring=getattr(fr.semiring, semiring)()))
    fruit.add(fr.sieving.NPI, fr.sieving.MPI, fr.sieving.END)
    return fruit


@pytest.mark.parametrize("semiring", ["Reals", "Arctic", "Bayesian"])
def test_fruit_slice(fr, semiring):
    X = slice_input(semiring)
    ref, expo = oracle_features(X, semiring, SLICE_WORDS)
    assert expo.sum() == 0        # (the reference alone: no element on a threshold)
    fruit = build_slice(fr, semiring)
    fruit.fit(X)
    feats = fruit.transform(X)
    assert feats.shape == ref.shape == (X.shape[0], 3 * 5)
    np.testing.assert_array_equal(feats[:, 0::3], ref[:, 0::3])                      # NPI: counts
    np.testing.assert_allclose(feats[:, 1::3], ref[:, 1::3], rtol=RTOL, atol=1e-9)   # MPI
    np.testing.assert_allclose(feats[:, 2::3], ref[:, 2::3], rtol=RTOL, atol=1e-9)   # END
    slc = fruit.get_slice(0)
    pipe = slc._fused(X.shape[2], D=X.shape[1])
    if semiring == "Bayesian":
        assert pipe is None       # rows that need the unshift materialise
    else:
        assert pipe is not None and pipe.last_launch()["family"].startswith("fused")
        assert pipe.plan.weighting == 0


def test_chained_iss_first_stage_generic(fr):
    X = slice_input("Reals")[:3, :, :40]
    first = ["[ABS(1)][DIM(2)]", "[ReLU(2)]"]
    fruit = fr.Fruit("chain")
    fruit.add(fr.ISS([fr.words.Word(s) for s in first]))
    fruit.add(fr.ISS([fr.words.SimpleWord("[1][1]"), fr.words.SimpleWord("[11]")]))
    fruit.add(fr.sieving.END)
    fruit.fit(X)
    feats = fruit.transform(X)
    stage1 = wref.iss_transform(X, first)
    want = []
    for row in stage1:
        its = orc.iss_transform(row[:, None, :], ["[1][1]", "[11]"])
        want += [r[:, -1] for r in its]
    np.testing.assert_allclose(feats, np.stack(want, axis=1), rtol=RTOL, atol=1e-9)


def test_callbacks_see_the_generic_rows(fr):
    X = slice_input("Reals")[:3, :, :40]

    class Collect(fr.callback.AbstractCallback):
        def __init__(self):
            self.rows = []

        def on_iterated_sum(self, Z):
            self.rows.append(np.array(Z))

    fruit = build_slice(fr, "Bayesian")
    Xb = np.abs(X) + 0.5
    fruit.fit(Xb)
    cb = Collect()
    feats = fruit.transform(Xb, callbacks=[cb])
    ref = wref.iss_transform(orc.inc_transform(Xb, 1, 1, False), SLICE_WORDS, "EXTENDED", "Bayesian")
    assert len(cb.rows) == ref.shape[0]
    rowwise_close(np.stack(cb.rows), ref)
    np.testing.assert_allclose(feats, fruit.transform(Xb), rtol=RTOL, atol=1e-9)
