#!/usr/bin/env python3
"""Generate tests/golden/golden_curvature.{npz,json}: the reference's CUR / AVG / STD sieves
(fruits/sieving/segment.py:228-358), its sieve wrappers INC / INT (fruits/sieving/wrapper.py) and
two whole fruits that use them.

TEST INFRASTRUCTURE - runs only where the reference tree is at hand, never on the GPU box.  The
reference is imported with the two loader accommodations of make_golden.py (a ``numba`` stand-in
whose ``njit`` returns the function unchanged and whose ``prange`` is ``range``; ``np.NINF``
for numpy >= 2); they change no arithmetic.  Only DATA is written.

A sieve is written down as a nested spec, ``{"kind": "INC", "sieve": {...}, "kw": {...}}`` for a
wrapper and ``{"kind": "CUR", "kw": {...}}`` for a plain sieve; the tests build theirs from it.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_curvature.py
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
from fruits.cache import _increments  # noqa: E402

arrays = {}
manifest = {"sieve": [], "fruit": []}


def put(name, arr):
    assert name not in arrays, name
    arrays[name] = np.ascontiguousarray(arr)
    return name


def S(kind, sieve=None, **kw):
    """A sieve spec (JSON)."""
    spec = {"kind": kind, "kw": {k: (list(v) if isinstance(v, (tuple, list)) else v)
                                 for k, v in kw.items()}}
    if sieve is not None:
        spec["sieve"] = sieve
    return spec


def make(spec, package=fruits):
    kw = {k: (tuple(v) if k == "q" else v) for k, v in spec["kw"].items()}
    cls = getattr(package.sieving, spec["kind"])
    if "sieve" in spec:
        return cls(make(spec["sieve"], package), **kw)
    return cls(**kw)


def sieve_case(name, x_key, spec):
    """fit_transform on one (N, T) array."""
    X = arrays[x_key]
    sv = make(spec)
    entry = {"name": name, "spec": spec, "x": x_key,
             "labels": [sv.label(i) for i in range(sv.nfeatures())],
             "str": str(sv), "summary": sv.summary(), "nfeatures": int(sv.nfeatures()),
             "requires_fitting": bool(sv.requires_fitting),
             "copy_str": str(sv.copy())}
    entry["out"] = put(f"sieve/{name}", sv.fit_transform(X))
    leaf = sv
    while hasattr(leaf, "_sieve"):
        leaf = leaf._sieve
    entry["quantiles"] = ([float(q) if np.isfinite(q) else str(q) for q in leaf._quantiles]
                          if hasattr(leaf, "_quantiles") else None)
    manifest["sieve"].append(entry)


# the inputs of make_golden_sieves.py
X_1 = np.array([
    [[-4, 0.8, 0, 5, -3], [2.0, 1, 0, 0, -7]],
    [[5.0, 8, 2, 6, 0], [-5, -1, -4, -0.5, -8]],
])
put("X_1_0", X_1[0])
put("X_1_1", X_1[1])
put("R_8_50", np.random.default_rng(41).standard_normal((8, 50)).cumsum(axis=1))
put("R_5_33", np.random.default_rng(42).standard_normal((5, 33)))
put("P_6_40", np.where(np.random.default_rng(43).random((6, 40)) < 0.7, 1.0, -1.0)
    * np.random.default_rng(44).random((6, 40)))

for kind in ("CUR", "AVG", "STD"):
    k = kind.lower()
    for x in ("X_1_0", "X_1_1"):
        sieve_case(f"{k}_{x}", x, S(kind))
        sieve_case(f"{k}_{x}_cut3", x, S(kind, cut=3))
        sieve_case(f"{k}_{x}_group1", x, S(kind, cut=[-1, 3, 1]))
        sieve_case(f"{k}_{x}_q3", x, S(kind, q=(-1.0, 0.0, 1.0)))
    for x in ("R_8_50", "R_5_33", "P_6_40"):
        T = arrays[x].shape[1]
        sieve_case(f"{k}_{x}", x, S(kind))
        sieve_case(f"{k}_{x}_group", x, S(kind, cut=[0, 10, 10, -1, T // 2]))
        sieve_case(f"{k}_{x}_coq", x, S(kind, cut=[0.3, 0.6, -1]))
        sieve_case(f"{k}_{x}_coq_l1", x, S(kind, cut=[0.5, -1], coquantile_norm="L1"))
        sieve_case(f"{k}_{x}_q4", x, S(kind, q=(0.25, 0.5, 0.75, 1.0)))
        sieve_case(f"{k}_{x}_q4_group", x, S(kind, q=(0.25, 0.5, 0.75, 1.0),
                                             cut=[0, 10, 10, -1, T // 2]))
        sieve_case(f"{k}_{x}_q3", x, S(kind, q=(-1.0, 0.0, 1.0), cut=[7, -1]))

WRAPPED = {
    "inc_npi": S("INC", S("NPI")),
    "inc_max_d2_s3": S("INC", S("MAX"), depth=2, shift=3),
    "inc_end_d0": S("INC", S("END"), depth=0),
    "int_mpi0": S("INT", S("MPI", inc=0)),
    "int_cur": S("INT", S("CUR", q=(0.5, 1.0))),
    "inc_int_npi": S("INC", S("INT", S("NPI", q=(0.3, 1.0)))),
    "inc_lpi": S("INC", S("LPI")),
}
for x in ("X_1_0", "R_8_50", "R_5_33", "P_6_40"):
    for name, spec in WRAPPED.items():
        sieve_case(f"{name}_{x}", x, spec)


# whole fruits (fit_sample_size = 1.0: the fit sample is the whole input, no random draw)
def build_fruit(spec):
    fr = fruits.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fr.cut()
        for p in sl.get("preps", []):
            fr.add(getattr(fruits.preparation, p["kind"])())
        for i in sl["iss"]:
            ws = [fruits.words.SimpleWord(s) for s in i["words"]]
            fr.add(fruits.ISS(ws, mode=getattr(fruits.ISSMode, i["mode"]),
                              semiring=getattr(fruits.semiring, i.get("semiring", "Reals"))()))
        for s in sl["sieves"]:
            fr.add(make(s))
        fr.get_slice().fit_sample_size = 1.0
    return fr


def seen_rows(sv, row):
    """(leaf sieve, the rows whose elements it compares with its thresholds)."""
    if isinstance(sv, fruits.sieving.INC):
        inc = row[:, np.newaxis, :]
        for _ in range(sv._depth):
            inc = _increments(row[:, np.newaxis, :], sv._shift)
        return seen_rows(sv._sieve, inc[:, 0, :])
    if isinstance(sv, fruits.sieving.INT):
        return seen_rows(sv._sieve, np.cumsum(row, axis=1))
    if isinstance(sv, (fruits.sieving.CUR, fruits.sieving.AVG, fruits.sieving.STD)):
        return sv, _increments(_increments(row[:, np.newaxis, :], 1), 1)[:, 0, :]
    if hasattr(sv, "_pre_transform"):
        return sv, sv._pre_transform(row)
    return sv, row


def assert_margins(fr, X, counts_too):
    """No element a banded sieve compares lies within 1e-9 * max|row| of a finite fitted
    threshold: rounding-level differences between a fused and a sequential evaluation cannot
    move an element across a band.  Demanded of every banded CUR / AVG / STD feature; with
    ``counts_too`` of the counting sieves as well (a zero that the zero padding or an absorbed
    summand makes exactly is the same zero everywhere: not counted against threshold 0)."""
    checked = 0
    for slc in fr:
        data = X
        for prep in slc.get_preparateurs():
            data = prep.transform(data)
        for i, itsum in enumerate(slc._iterate_iss(data)):
            for sv in slc._sieves_extended[i]:
                leaf, rows = seen_rows(sv, itsum)
                cur = isinstance(leaf, (fruits.sieving.CUR, fruits.sieving.AVG, fruits.sieving.STD))
                npi = isinstance(leaf, fruits.sieving.NPI)
                if not (cur or (counts_too and npi)) or not hasattr(leaf, "_quantiles"):
                    continue
                for th in leaf._quantiles:
                    if not np.isfinite(th):
                        continue
                    gap = np.abs(rows - th)
                    if th == 0.0:
                        gap = np.where(rows == 0.0, np.inf, gap)
                    bound = 1e-9 * np.abs(itsum).max(axis=1, keepdims=True)
                    assert (gap > bound).all(), (str(sv), i, float(th), float(gap.min()))
                    checked += 1
    return checked


def fruit_case(name, x_key, spec, counts_too):
    X = arrays[x_key]
    fr = build_fruit(spec)
    fr.fit(X)
    out = fr.transform(X)
    margins = assert_margins(fr, X, counts_too)
    manifest["fruit"].append({
        "name": name, "x": x_key, "spec": spec, "nfeatures": int(fr.nfeatures()),
        "labels": [fr.label(i) for i in range(fr.nfeatures())],
        "summary": fr.summary(), "out": put(f"fruit/{name}", out), "margins_checked": margins})


put("F_12_2_64", np.random.default_rng(47).standard_normal((12, 2, 64)))
put("F_10_1_80", np.random.default_rng(48).standard_normal((10, 1, 80)))
W22 = [str(w) for w in fruits.words.of_weight(2, dim=2)]
fruit_case("reals_curvature", "F_12_2_64", {"name": "reals", "slices": [
    {"preps": [{"kind": "INC"}], "iss": [{"words": W22, "mode": "EXTENDED"}],
     "sieves": [S("CUR", q=(0.5, 1.0)), S("AVG"), S("STD", cut=[0.5, -1]),
                S("INC", S("NPI")), S("INT", S("NPI", inc=0, q=(0.3, 1.0))),
                S("INT", S("MAX")), S("END")]}]}, counts_too=True)
fruit_case("arctic_curvature", "F_10_1_80", {"name": "arctic", "slices": [
    {"iss": [{"words": ["[1]", "[11]", "[1][1]", "[1][11]"], "mode": "EXTENDED",
              "semiring": "Arctic"}],
     "sieves": [S("CUR", q=(0.25, 0.75, 1.0)), S("INC", S("MPI"))]}]}, counts_too=False)

if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "golden_curvature.npz"), **arrays)
    with open(os.path.join(HERE, "golden_curvature.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(f"wrote {len(arrays)} arrays, {len(manifest['sieve'])} sieve cases, "
          f"{len(manifest['fruit'])} fruits "
          f"({[c['margins_checked'] for c in manifest['fruit']]} thresholds with a margin)")
