#!/usr/bin/env python3
"""Generate tests/golden/golden_filters.{npz,json}: the reference's RDW / SPE / RPE / CTS / QTC
preparateurs (fruits/preparation/transform.py:571-613, 749-1015), the filters DIL / WIN / DOT / PDD
(fruits/preparation/filter.py), DIM / NEW around some of them and three whole fruits that start
with them.

TEST INFRASTRUCTURE - runs only where the reference tree is at hand, never on the GPU box.  The
reference is imported with the two loader accommodations of make_golden_prep.py (a ``numba``
stand-in whose ``njit`` returns the function unchanged and whose ``prange`` is ``range``;
``np.NINF`` for numpy >= 2); they change no arithmetic.  Only DATA is written.

The inputs are multiples of 1/2 in [-2, 2] (they and every masked, shifted or clipped copy of them
compress well, and their path lengths are exact in any summation order); the classes that round
(SPE, RPE, RDW) run on smaller batches.  Shapes: every T of (1, 2, 5, 511, 512, 513, 1031) - one
lane pair, rows off 16-byte alignment, both sides of a tile edge, two tiles - with N in (1, 3) and
D in (1, 2, 3) spread over them.

A case with ``"cache_x"`` ran attached to a cache of THAT input (``p._cache``, then
``p._transform``): the batch and the cache differ in their number of series.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_filters.py
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
from fruits.cache import SharedSeedCache  # noqa: E402

arrays = {}
manifest = {"numpy": np.__version__,
            "all_transform": list(fruits.preparation.transform.__all__),
            "all_filter": list(fruits.preparation.filter.__all__),
            "all_wrapper": list(fruits.preparation.wrapper.__all__), "prep": [], "fruit": []}
ARRAY_STATE = ("_indices", "_lengths", "_weights")
SCALAR_STATE = ("_n", "_first", "_width", "_quantile")


def put(name, arr):
    assert name not in arrays, name
    arrays[name] = np.ascontiguousarray(arr)
    return name


def make(spec, pkg):
    cls = getattr(pkg, spec["kind"])
    if spec["kind"] == "DIM":
        d = spec["dim"]
        return cls(make(spec["inner"], pkg), d if isinstance(d, int) else tuple(d))
    if spec["kind"] == "NEW":
        return cls(make(spec["inner"], pkg))
    return cls(*spec.get("args", []), **spec.get("kw", {}))


def innermost(p):
    while hasattr(p, "_preparateur") and p._preparateur is not None:
        p = p._preparateur
    return p


def prep_case(name, x_key, spec, seed=0, cache_x=None):
    X = arrays[x_key]
    entry = {"name": name, "x": x_key, "spec": spec, "seed": seed}
    if cache_x is not None:
        entry["cache_x"] = cache_x
    p = make(spec, fruits.preparation)
    try:
        eq = bool(p == p.copy())
    except ValueError:
        eq = "ValueError"
    entry.update({"str": str(p), "copy_str": str(p.copy()),
                  "requires_fitting": bool(p.requires_fitting), "eq_copy": eq})
    try:
        np.random.seed(seed)
        p.fit(X)
        state = {}
        inner = innermost(p)
        for a in ARRAY_STATE:
            if hasattr(inner, a):
                state[a] = put(f"state/{name}/{a}", np.asarray(getattr(inner, a)))
        for a in SCALAR_STATE:
            if hasattr(inner, a):
                v = getattr(inner, a)
                state[a] = float(v) if a == "_quantile" else int(v)
        entry["state"] = state
        with np.errstate(all="ignore"):
            if cache_x is None:
                out = p.transform(X)
            else:
                p._cache = SharedSeedCache(arrays[cache_x])
                out = p._transform(X)
    except (ValueError, RuntimeError, IndexError) as err:
        entry["reference_raises"] = type(err).__name__
        entry["raises_at"] = "transform" if "state" in entry else "fit"
    else:
        entry["out"] = put(f"out/{name}", out)
    manifest["prep"].append(entry)
    return p


def S(kind, *args, **kw):
    return {"kind": kind, "args": list(args), "kw": kw}


rng = np.random.default_rng(61)


def halves(shape):
    return rng.integers(-4, 5, size=shape) / 2.0


# sweep A (masks, shifts, clips), sweep B (two dimensions: RPE), sweep C (SPE, RDW)
TS = (1, 2, 5, 511, 512, 513, 1031)
A = dict(zip(TS, ((3, 3), (1, 2), (3, 1), (3, 2), (1, 3), (1, 2), (3, 1))))
B = dict(zip(TS, ((3, 2), (1, 2), (3, 2), (1, 2), (1, 2), (1, 2), (1, 2))))
C = dict(zip(TS, ((3, 1), (1, 3), (3, 2), (1, 1), (1, 2), (3, 1), (1, 1))))
for T in TS:
    put(f"A_{T}", halves((A[T][0], A[T][1], T)))
    put(f"B_{T}", halves((B[T][0], 2, T)))
    put(f"C_{T}", halves((C[T][0], C[T][1], T)))
    # a batch of three series, the middle one constant (no path length: 0 / 0 in SPE, the
    # whole series inside every window of WIN)
    flat = halves((3, 2 if T < 500 else 1, T))
    flat[1, :, :] = 1.5
    put(f"K_{T}", flat)
    put(f"P_{T}", np.abs(halves((C[T][0], C[T][1], T))) + 0.5)      # positive: RDW

for T in TS:
    a = f"A_{T}"
    prep_case(f"dil_none_{T}", a, S("DIL"), seed=T)
    prep_case(f"dil_03_{T}", a, S("DIL", 0.3), seed=T + 1)
    prep_case(f"dil_1_{T}", a, S("DIL", 1.0), seed=T + 2)
    prep_case(f"dot_2_{T}", a, S("DOT", 2))
    prep_case(f"dot_frac_{T}", a, S("DOT", 0.1, 0.05))
    prep_case(f"dot_5_0_{T}", a, S("DOT", 5, 0))
    prep_case(f"dot_big_{T}", a, S("DOT", T + 3))
    prep_case(f"pdd_{T}", a, S("PDD"))
    prep_case(f"pdd_1_05_{T}", a, S("PDD", 1.0, 0.5))
    prep_case(f"pdd_w0_{T}", a, S("PDD", 0.5, 0.2))
    k = f"K_{T}"
    prep_case(f"win_all_{T}", k, S("WIN", 0.0, 1.0))
    prep_case(f"win_mid_{T}", k, S("WIN", 0.25, 0.75))
    prep_case(f"win_empty_{T}", k, S("WIN", 0.6, 0.4))
    for tag, s in (("1", 1), ("3", 3), ("Tm1", T - 1), ("T", T), ("Tp5", T + 5), ("q", 0.25)):
        if tag == "Tm1" and T == 1:
            continue       # (s = 0: the raising case below)
        prep_case(f"cts_{tag}_{T}", a, S("CTS", s))
        prep_case(f"cts_{tag}_{T}_pseudo", a, S("CTS", s, pseudo_shift=True))
    nan = arrays[a].copy()
    nan[0, 0, T // 2] = np.nan
    put(f"AN_{T}", nan)
    prep_case(f"qtc_07_{T}", a, S("QTC", 0.7))
    prep_case(f"qtc_02_lower_{T}", a, S("QTC", 0.2, lower=True))
    prep_case(f"qtc_05_bound_{T}", a, S("QTC", 0.5, bound=-1.0))
    if T in (5, 513):
        prep_case(f"qtc_07_nan_{T}", f"AN_{T}", S("QTC", 0.7))
    prep_case(f"rpe_05_{T}", f"B_{T}", S("RPE", 0.5))
    if T in (2, 5):
        prep_case(f"rpe_03_long_{T}", f"B_{T}", S("RPE", 0.3, max_length=2000))
    c = f"C_{T}"
    prep_case(f"spe_mul_{T}", c, S("SPE", 0.5))
    if T in (5, 511):
        prep_case(f"spe_add_{T}", c, S("SPE", 0.5, operation="additive"))
    if T in (2, 5):
        prep_case(f"spe_long_{T}", c, S("SPE", 0.3, max_length=2000))
    if T != 511 and T != 1031:
        prep_case(f"spe_l1_{T}", k, S("SPE", 0.5, step_transform="L1"))
    if T in (5, 511):
        prep_case(f"spe_l2_add_{T}", k, S("SPE", 0.4, operation="additive", step_transform="L2"))
    if T in (2, 5):
        prep_case(f"spe_l1_long_{T}", k, S("SPE", 0.5, step_transform="L1", max_length=300))
    prep_case(f"rdw_uniform_{T}", f"P_{T}", S("RDW", "uniform"), seed=T + 3)
    if T in (5, 511):
        prep_case(f"rdw_dirichlet_{T}", f"P_{T}", S("RDW", "dirichlet"), seed=T + 4)

prep_case("cts_0", "A_5", S("CTS", 0))
prep_case("cts_0_pseudo", "A_5", S("CTS", 0, pseudo_shift=True))
prep_case("rpe_three_dims", "A_1", S("RPE", 0.5))
# a one-series batch against the cache of three series: three series come out
put("K1_513", arrays["K_513"][2:3])
prep_case("spe_l1_one_against_three", "K1_513", S("SPE", 0.5, step_transform="L1"),
          cache_x="K_513")
put("K2_5", arrays["K_5"][:2])
prep_case("spe_l1_two_against_three", "K2_5", S("SPE", 0.5, step_transform="L1"), cache_x="K_5")
prep_case("win_two_of_three", "K2_5", S("WIN", 0.25, 0.75), cache_x="K_5")
put("K6_5", np.concatenate([arrays["K_5"], arrays["K_5"]]))
prep_case("win_six_against_three", "K6_5", S("WIN", 0.25, 0.75), cache_x="K_5")
# RDW: a negative entry (NaN out), a dimension that is zero everywhere (the +1e-5 branch)
neg = arrays["P_5"].copy()
neg[1, 0, 2] = -1.5
put("PN_5", neg)
prep_case("rdw_dirichlet_negative", "PN_5", S("RDW", "dirichlet"), seed=71)
zero = np.abs(halves((3, 3, 5))) + 0.5
zero[:, 1, :] = 0.0
put("PZ_5", zero)
prep_case("rdw_dirichlet_zero_dim", "PZ_5", S("RDW", "dirichlet"), seed=72)

# masks over NaN / infinity / -1.0 on dropped positions, -0.0 on a kept one
for T in (5, 513):
    for tag, spec, seed in (("dil", S("DIL", 0.3), T + 1), ("dot", S("DOT", 2), 0),
                            ("pdd", S("PDD", 1.0, 0.5), 0),
                            ("cts", S("CTS", 3, pseudo_shift=True), 0)):
        probe = make(spec, fruits.preparation)
        np.random.seed(seed)
        probe.fit(arrays[f"A_{T}"])
        kept = probe.transform(np.ones((1, 1, T)))[0, 0] != 0
        dropped = np.flatnonzero(~kept)
        X = arrays[f"A_{T}"].copy()
        for pos, v in zip(dropped[:3], (np.nan, np.inf, -1.0)):
            X[:, :, pos] = v
        X[-1, -1, dropped[-1]] = -np.inf
        X[0, 0, np.flatnonzero(kept)[0]] = -0.0
        put(f"planted/{tag}_{T}", X)
        prep_case(f"planted_{tag}_{T}", f"planted/{tag}_{T}", spec, seed=seed)

# wrappers
for T in (5, 513):
    x = f"K_{T}" if T == 5 else f"B_{T}"
    prep_case(f"dim_dot_{T}", x, {"kind": "DIM", "inner": S("DOT", 3), "dim": 1})
    prep_case(f"dim_spe_{T}", x, {"kind": "DIM", "inner": S("SPE", 0.5), "dim": [1, 0]})
    prep_case(f"dim_qtc_{T}", x, {"kind": "DIM", "inner": S("QTC", 0.6), "dim": 0})
    prep_case(f"new_dot_{T}", x, {"kind": "NEW", "inner": S("DOT", 3)})
    prep_case(f"new_spe_{T}", x, {"kind": "NEW", "inner": S("SPE", 0.5, operation="additive")})
    prep_case(f"new_qtc_{T}", x, {"kind": "NEW", "inner": S("QTC", 0.4, lower=True)})


# whole fruits (fit_sample_size = 1.0: the fit sample is the whole input)
def build_fruit(spec, pkg):
    fr = pkg.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fr.cut()
        for p in sl.get("preps", []):
            fr.add(make(p, pkg.preparation))
        for i in sl["iss"]:
            ws = [pkg.words.SimpleWord(s) for s in i["words"]]
            fr.add(pkg.ISS(ws, mode=getattr(pkg.ISSMode, i["mode"])))
        for s in sl["sieves"]:
            fr.add(getattr(pkg.sieving, s["kind"])())
        fr.get_slice().fit_sample_size = 1.0
    return fr


def fruit_case(name, x_key, spec, seed):
    X = arrays[x_key]
    fr = build_fruit(spec, fruits)
    np.random.seed(seed)
    fr.fit(X)
    out = fr.transform(X)
    cache = SharedSeedCache(X)
    prepared = X
    for p in fr.get_slice()._preparateurs:
        p._cache = cache
        prepared = p._transform(prepared)
    manifest["fruit"].append({
        "name": name, "x": x_key, "spec": spec, "seed": seed, "nfeatures": int(fr.nfeatures()),
        "labels": [fr.label(i) for i in range(fr.nfeatures())],
        "summary": fr.summary(), "prepared": put(f"fruit/{name}/prepared", prepared),
        "out": put(f"fruit/{name}", out)})


put("F_12_2_64", np.random.default_rng(65).standard_normal((12, 2, 64)).cumsum(axis=2))
W22 = [str(w) for w in fruits.words.of_weight(2, dim=2)]
TAIL = {"iss": [{"words": W22, "mode": "EXTENDED"}], "sieves": [{"kind": "NPI"}, {"kind": "END"}]}
# PDD(1.0, 0.25) at T = 64: one strip, the first 16 points (PDD() itself has width int(32 / 57) = 0
# there: the identity).  A strip at the front on purpose: the iterated sums of zeros are exactly
# zero in any order of summation.  Behind a strip INSIDE the series INC makes the running sum of
# a dimension return to zero up to the rounding of the differences, so the increments of the
# iterated sums that follow are products with rounding noise - near-ties at NPI's threshold 0 in
# the reference itself at every such point, and the share of series whose counts may differ is
# no longer the small number the fruit bars are written for.  The strips inside a series are
# covered bit for bit by the pdd_* cases above.
fruit_case("pdd_inc", "F_12_2_64", {"name": "pdd", "slices": [
    {"preps": [S("PDD", 1.0, 0.25), S("INC")], **TAIL}]}, seed=41)
fruit_case("win_inc", "F_12_2_64", {"name": "win", "slices": [
    {"preps": [S("WIN", 0.1, 0.9), S("INC")], **TAIL}]}, seed=42)
fruit_case("spe_l1_inc", "F_12_2_64", {"name": "spe", "slices": [
    {"preps": [S("SPE", 0.5, step_transform="L1"), S("INC")], **TAIL}]}, seed=43)

np.savez_compressed(os.path.join(HERE, "golden_filters.npz"), **arrays)
with open(os.path.join(HERE, "golden_filters.json"), "w") as f:
    json.dump(manifest, f, indent=1)
print(f"wrote {len(arrays)} arrays, {len(manifest['prep'])} preparateur cases, "
      f"{sum('reference_raises' in c for c in manifest['prep'])} of them raising, "
      f"{len(manifest['fruit'])} fruits")
