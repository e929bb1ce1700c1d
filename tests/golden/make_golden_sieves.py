#!/usr/bin/env python3
"""Generate tests/golden/golden_sieves.{npz,json}: the reference's MAX / MIN / XPI / LPI sieves
(fruits/sieving/segment.py:107-200, increment.py:166-239) and three whole fruits that use them.

TEST INFRASTRUCTURE - runs only where the reference tree is at hand, never on the GPU box.  The
reference is imported with the two loader accommodations of make_golden.py (a ``numba`` stand-in
whose ``njit`` returns the function unchanged and whose ``prange`` is ``range``; ``np.NINF``
for numpy >= 2); they change no arithmetic.  Only DATA is written.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sieves.py
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
manifest = {"sieve": [], "fruit": []}


def put(name, arr):
    assert name not in arrays, name
    arrays[name] = np.ascontiguousarray(arr)
    return name


def jsonable(kw):
    return {k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in kw.items()}


def sieve_case(name, kind, x_key, **kw):
    """fit_transform on one (N, T) array; a reference that raises is recorded as such."""
    X = arrays[x_key]
    sv = getattr(fruits.sieving, kind)(**kw)
    entry = {"name": name, "kind": kind, "x": x_key, "kw": jsonable(kw),
             "labels": [sv.label(i) for i in range(sv.nfeatures())],
             "str": str(sv), "summary": sv.summary(), "nfeatures": int(sv.nfeatures()),
             "requires_fitting": bool(sv.requires_fitting),
             "copy_str": str(sv.copy())}
    try:
        out = sv.fit_transform(X)
    except ValueError:
        entry["reference_raises"] = "ValueError"
    else:
        entry["out"] = put(f"sieve/{name}", out)
        entry["quantiles"] = [float(q) if np.isfinite(q) else str(q) for q in sv._quantiles]
    manifest["sieve"].append(entry)


X_1 = np.array([
    [[-4, 0.8, 0, 5, -3], [2.0, 1, 0, 0, -7]],
    [[5.0, 8, 2, 6, 0], [-5, -1, -4, -0.5, -8]],
])
put("X_1_0", X_1[0])
put("X_1_1", X_1[1])
put("R_8_50", np.random.default_rng(41).standard_normal((8, 50)).cumsum(axis=1))
put("R_5_33", np.random.default_rng(42).standard_normal((5, 33)))
# runs and empty bands on purpose: a sign pattern with long positive stretches
put("P_6_40", np.where(np.random.default_rng(43).random((6, 40)) < 0.7, 1.0, -1.0)
    * np.random.default_rng(44).random((6, 40)))

# the inputs of the reference's tests/sieving/test_explicit.py
for x in ("X_1_0", "X_1_1"):
    for kind in ("MAX", "MIN"):
        k = kind.lower()
        sieve_case(f"{k}_{x}", kind, x)
        sieve_case(f"{k}_{x}_cut3", kind, x, cut=3)
        sieve_case(f"{k}_{x}_cut05", kind, x, cut=0.5)
        sieve_case(f"{k}_{x}_group1", kind, x, cut=[-1, 3, 1])
        sieve_case(f"{k}_{x}_group2", kind, x, cut=[-1, 0.2, 0.7, 0.5])
    sieve_case(f"xpi_{x}", "XPI", x)
    sieve_case(f"lpi_{x}", "LPI", x)

for x in ("R_8_50", "R_5_33", "P_6_40"):
    T = arrays[x].shape[1]
    for kind in ("MAX", "MIN"):
        k = kind.lower()
        sieve_case(f"{k}_{x}", kind, x)
        sieve_case(f"{k}_{x}_group", kind, x, cut=[0, 10, 10, -1, T // 2])
        sieve_case(f"{k}_{x}_coq", kind, x, cut=[0.3, 0.6, -1])
        sieve_case(f"{k}_{x}_coq_l1", kind, x, cut=[0.5, -1], coquantile_norm="L1")
        sieve_case(f"{k}_{x}_q4", kind, x, q=(0.25, 0.5, 0.75, 1.0))
        sieve_case(f"{k}_{x}_q3", kind, x, q=(-1.0, 0.0, 1.0), cut=[7, -1])
        # empty bands of non-empty segments: the reference raises (np.max of an empty array)
        sieve_case(f"{k}_{x}_empty", kind, x, q=(-1.0, 0.05, 1.0), cut=[1, -1])
    for kind in ("XPI", "LPI"):
        k = kind.lower()
        for inc in (0, 1, 2, -1):
            sieve_case(f"{k}_{x}_inc{inc}", kind, x, inc=inc)
            sieve_case(f"{k}_{x}_inc{inc}_q", kind, x, inc=inc, q=(0.25, 0.5, 0.75, 1.0),
                       cut=[0, 10, 10, -1, T // 2])
            sieve_case(f"{k}_{x}_inc{inc}_q3", kind, x, inc=inc, q=(-1.0, 0.0, 1.0))
        sieve_case(f"{k}_{x}_coq", kind, x, cut=[0.3, 0.6, -1])
        sieve_case(f"{k}_{x}_coq_l1", kind, x, cut=[0.5, -1], coquantile_norm="L1", inc=0)


# whole fruits (fit_sample_size = 1.0: the fit sample is the whole input, no random draw)
def build_fruit(spec):
    fr = fruits.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fr.cut()
        for p in sl.get("preps", []):
            fr.add(getattr(fruits.preparation, p["kind"])())
        for i in sl["iss"]:
            ws = [fruits.words.SimpleWord(s) for s in i["words"]]
            if i.get("kind") == "CosWISS":
                fr.add(fruits.CosWISS(freqs=i["freqs"], words=ws, exponent=i.get("exponent", 2)))
                continue
            fr.add(fruits.ISS(ws, mode=getattr(fruits.ISSMode, i["mode"]),
                              semiring=getattr(fruits.semiring, i.get("semiring", "Reals"))()))
        for s in sl["sieves"]:
            kw = {k: (tuple(v) if k == "q" else v) for k, v in s.items() if k != "kind"}
            fr.add(getattr(fruits.sieving, s["kind"])(**kw))
        fr.get_slice().fit_sample_size = 1.0
    return fr


def fruit_case(name, x_key, spec):
    X = arrays[x_key]
    fr = build_fruit(spec)
    fr.fit(X)
    out = fr.transform(X)
    manifest["fruit"].append({
        "name": name, "x": x_key, "spec": spec, "nfeatures": int(fr.nfeatures()),
        "labels": [fr.label(i) for i in range(fr.nfeatures())],
        "summary": fr.summary(), "out": put(f"fruit/{name}", out)})


put("F_12_2_64", np.random.default_rng(45).standard_normal((12, 2, 64)))
put("F_10_1_80", np.random.default_rng(46).standard_normal((10, 1, 80)))
W22 = [str(w) for w in fruits.words.of_weight(2, dim=2)]
fruit_case("reals_all", "F_12_2_64", {"name": "reals", "slices": [
    {"preps": [{"kind": "INC"}], "iss": [{"words": W22, "mode": "EXTENDED"}],
     "sieves": [{"kind": "MAX"}, {"kind": "MIN", "cut": [0.5, -1]},
                {"kind": "XPI", "q": [0.5, 1.0]}, {"kind": "LPI"}, {"kind": "NPI"},
                {"kind": "END"}]}]})
fruit_case("arctic_max_xpi", "F_10_1_80", {"name": "arctic", "slices": [
    {"iss": [{"words": ["[1]", "[11]", "[1][1]", "[1][11]"], "mode": "EXTENDED",
              "semiring": "Arctic"}],
     "sieves": [{"kind": "MAX", "cut": [0.5, -1]}, {"kind": "XPI", "q": [0.25, 0.75, 1.0]}]}]})
fruit_case("coswiss_min_xpi", "F_12_2_64", {"name": "cos", "slices": [
    {"preps": [{"kind": "INC"}],
     "iss": [{"kind": "CosWISS", "words": ["[1]", "[2]", "[1][2]", "[11][2]"],
              "freqs": [0.5, 2.0]}],
     "sieves": [{"kind": "MIN"}, {"kind": "XPI", "inc": 0}]}]})

np.savez_compressed(os.path.join(HERE, "golden_sieves.npz"), **arrays)
with open(os.path.join(HERE, "golden_sieves.json"), "w") as f:
    json.dump(manifest, f, indent=1)
print(f"wrote {len(arrays)} arrays, {len(manifest['sieve'])} sieve cases, "
      f"{sum('reference_raises' in c for c in manifest['sieve'])} of them raising, "
      f"{len(manifest['fruit'])} fruits")
