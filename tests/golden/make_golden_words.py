#!/usr/bin/env python3
"""Generate tests/golden/golden_words.{npz,json}: the reference's iterated sums of GENERIC words
(fruits/iss/words/letters.py, the slow path of fruits/iss/semiring.py:54-75), alone and next to
simple words, on fixed seeded inputs - and the data of the two scenarios of the reference's
tests/signature/test_general.py.

TEST INFRASTRUCTURE - runs only where the reference tree is at hand, never on the GPU box.  The
reference is imported with the two loader accommodations of make_golden.py (a ``numba`` stand-in
whose ``njit`` returns the function unchanged and whose ``prange`` is ``range``; ``np.NINF``
for numpy >= 2); they change no arithmetic.  Only DATA is written: the inputs are regenerated
from their seeds (conftest.gen_input, or ``x`` arrays for the literal ones).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_words.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FRUITS_REFERENCE", "/root/reference")


def _install_loader_shims():
    if not hasattr(np, "NINF"):
        np.NINF = -np.inf
    try:
        import numba  # noqa: F401
        return
    except ImportError:
        pass
    nb = types.ModuleType("numba")

    def njit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f

    nb.njit = njit
    nb.jit = njit
    nb.prange = range
    sys.modules["numba"] = nb


_install_loader_shims()
sys.path.insert(0, REF)
import fruits  # noqa: E402  (the reference)

arrays = {}
manifest = {"iss": [], "literal": {}}


def put(name, arr):
    assert name not in arrays, name
    arrays[name] = np.ascontiguousarray(arr)
    return name


def gen_input(spec):     # (conftest.gen_input, plus the shifted uniform of the Bayesian cases)
    rng = np.random.default_rng(spec["seed"])
    if spec["dist"] == "uniform":
        return rng.random(tuple(spec["shape"])) + spec.get("offset", 0.0)
    return rng.standard_normal(tuple(spec["shape"]))


# the custom letters of the cases (tests/words_ref.py, LETTERS, restates them)
@fruits.words.letter(name="ReLU")
def _relu(X, i):
    return X[i, :] * (X[i, :] > 0)


@fruits.words.letter
def SQ(X, i):
    return X[i, :] * X[i, :]


def make_word(s):
    if "(" in s and any(c.isalpha() for c in s) or "[]" in s:
        return fruits.words.Word(s)
    return fruits.words.SimpleWord(s)


def make_weighting(spec):
    if spec is None:
        return None
    kw = {k: v for k, v in spec.items() if k != "kind"}
    return getattr(fruits.iss.weighting, spec["kind"])(**kw)


def iss_case(name, words, x_gen, semiring="Reals", mode="SINGLE", weighting=None, alphas=None):
    X = gen_input(x_gen)
    ws = [make_word(s) for s in words]
    for w, a in zip(ws, alphas or []):
        if a is not None:
            w.alpha = a
    iss = fruits.ISS(ws, mode=getattr(fruits.ISSMode, mode),
                     semiring=getattr(fruits.semiring, semiring)(),
                     weighting=make_weighting(weighting))
    out = iss.fit_transform(X)
    K = iss.n_iterated_sums()
    assert out.shape == (K, X.shape[0], X.shape[2])
    manifest["iss"].append({
        "name": name, "words": words, "x_gen": x_gen, "semiring": semiring, "mode": mode,
        "weighting": weighting, "alphas": alphas, "K": int(K),
        "labels": [iss.label(i) for i in range(K)],
        "depths": ([iss._cache_plan.unique_el_depth(i) for i in range(len(ws))]
                   if mode == "EXTENDED" else [1] * len(ws)),
        "out": put(f"iss/{name}", out)})


# word lengths 1, 2, 3 and 5, shared prefixes, an empty extended letter, a custom letter
WORDS = ["[ABS(1)DIM(2)][ABS(1)]", "[ABS(1)DIM(2)][DIM(3)][DIM(1)DIM(1)]", "[DIM(2)]",
         "[ABS(1)DIM(2)][ABS(1)][ReLU(2)][DIM(3)][ABS(2)]", "[DIM(1)][][DIM(2)]",
         "[SQ(3)ReLU(1)][ABS(2)]"]
DATA = {"Reals": [("U", {"dist": "uniform"}), ("N", {"dist": "normal"})],
        "Arctic": [("U", {"dist": "uniform"}), ("N", {"dist": "normal"})],
        "Bayesian": [("U05", {"dist": "uniform", "offset": 0.5})]}
for semiring, dists in DATA.items():
    for tag, dist in dists:
        for T in (5, 65):
            if tag == "N" and T == 65:
                continue
            # (T = 65: the SINGLE rows are among the EXTENDED ones - kept out, the file stays small)
            for mode in ("SINGLE", "EXTENDED") if T == 5 else ("EXTENDED",):
                iss_case(f"{semiring}_{tag}_T{T}_{mode}", WORDS,
                         dict(dist, seed=100 + T, shape=[4, 3, T]), semiring, mode)
    # a word longer than the series: its deep rows are all zero
    iss_case(f"{semiring}_long_word", ["[DIM(1)][ABS(2)][DIM(1)][DIM(2)]", "[ABS(1)]"],
             dict(dists[0][1], seed=7, shape=[4, 2, 3]), semiring, "EXTENDED")

# generic words next to weighted simple ones: the generic rows ignore the weighting
MIXED = ["[ABS(1)][DIM(2)]", "[12]", "[1][2]", "[ReLU(1)DIM(2)][ABS(1)]", "[1][2][2]"]
for wname, wspec in (("Indices", {"kind": "Indices"}), ("L1", {"kind": "L1"}),
                     ("Indices_total", {"kind": "Indices", "total": True})):
    for mode in ("SINGLE", "EXTENDED"):
        iss_case(f"mixed_{wname}_{mode}", MIXED, {"dist": "uniform", "seed": 21, "shape": [4, 2, 20]},
                 "Reals", mode, wspec, alphas=[None, None, [0.5, 2.0], None, [1.0, 0.25, 3.0]])
iss_case("mixed_Arctic_Indices", MIXED, {"dist": "normal", "seed": 22, "shape": [4, 2, 20]},
         "Arctic", "EXTENDED", {"kind": "Indices"})
iss_case("mixed_Bayesian_plain", MIXED, {"dist": "uniform", "offset": 0.5, "seed": 23, "shape": [4, 2, 20]},
         "Bayesian", "EXTENDED")
iss_case("mixed_Reals_plain", MIXED, {"dist": "normal", "seed": 24, "shape": [4, 2, 20]},
         "Reals", "EXTENDED")

# ---- the two scenarios of the reference's tests/signature/test_general.py ------------------
# Its data - the input X_1 and the numbers it expects next to it - are kept as fixtures; the
# words are written as strings and built like every other case here.
X1 = np.array([[[-4, 0.8, 0, 5, -3], [2.0, 1, 0, 0, -7]],
               [[5.0, 8, 2, 6, 0], [-5, -1, -4, -0.5, -8]]])
X1_EXPECTED = np.array([[[0, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
                        [[-64, -63.488, -63.488, 61.512, 34.512], [125, 637, 645, 861, 861]]])
X1_WORDS = ["[ReLU(1)][ReLU(2)]", "[111]"]
x1_out = fruits.ISS([make_word(s) for s in X1_WORDS]).fit_transform(X1)
np.testing.assert_allclose(x1_out, X1_EXPECTED)
manifest["literal"]["x1"] = {"words": X1_WORDS, "x": put("literal/x1", X1),
                             "expected": put("literal/x1_expected", X1_EXPECTED),
                             "out": put("literal/x1_out", x1_out)}

# slow path = fast path: two simple words rewritten with custom letters that pick a dimension
SIMPLE_PAIR = ["[11122][122222][11]", "[22][112][2221]"]
PICKERS = ["dim_letter", "single_dim_letter"]
for picker in PICKERS:
    fruits.words.letter(name=picker)(lambda X, i: X[i, :])


def spelled(simple, picker):
    """The string of the generic word that spells the simple word ``simple`` with ``picker``."""
    table = np.array(list(fruits.words.SimpleWord(simple)))
    return "".join("[" + "".join(f"{picker}({d + 1})" * int(n) for d, n in enumerate(row)) + "]"
                   for row in table)


pair_strings = [spelled(s, p) for s, p in zip(SIMPLE_PAIR, PICKERS)]
pair_x = {"dist": "uniform", "seed": 5, "shape": [6, 2, 40]}
slow = fruits.ISS([fruits.words.Word(s) for s in pair_strings]).fit_transform(gen_input(pair_x))
fast = fruits.ISS([fruits.words.SimpleWord(s) for s in SIMPLE_PAIR]).fit_transform(gen_input(pair_x))
np.testing.assert_allclose(slow, fast)
manifest["literal"]["fast_slow"] = {
    "x_gen": pair_x, "letters": PICKERS, "simple": SIMPLE_PAIR, "strings": pair_strings,
    "slow": put("literal/slow", slow), "fast": put("literal/fast", fast)}

np.savez(os.path.join(HERE, "golden_words.npz"), **arrays)
with open(os.path.join(HERE, "golden_words.json"), "w") as f:
    json.dump(manifest, f, indent=1)
print(f"{len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes, "
      f"{len(manifest['iss'])} iss cases")
