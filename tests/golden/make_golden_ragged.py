#!/usr/bin/env python3
"""Generate tests/golden/golden_ragged.{npz,json}: whole fruits of the reference on series of
their own lengths - after ONE seeded fit on the dense batch, the reference transforms series by
series, series n truncated to ``lengths[n]``.  Row n of the device's
``fruit.transform(X, lengths=lengths)`` has to be that row.

TEST INFRASTRUCTURE - runs only where the reference tree is at hand, never on the GPU box.  The
reference is imported with the two loader accommodations of make_golden.py (a ``numba`` stand-in
whose ``njit`` returns the function unchanged and whose ``prange`` is ``range``; ``np.NINF``
for numpy >= 2); they change no arithmetic.  Only DATA is written.

Margins: the device compares the counting columns (NPI, XPI, LPI, PPV, CPV) EXACTLY, so no
element of a counting sieve's row - the increments for NPI / XPI / LPI, the row itself for PPV /
CPV - may lie within 1e-10 of one of that copy's finite thresholds in the reference's own rows
(the margin of tests/test_sieves_band.py).  A data seed that violates it is passed over for the
next one; the seed used is recorded.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ragged.py
"""
import json
import os
import sys
import types
import warnings

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

N, D, T = 8, 2, 600
LENGTHS = [4, 9, 64, 129, 257, 513, 599, 600]
MARGIN = 1e-10
COUNTING = ("NPI", "XPI", "LPI", "PPV", "CPV")


def S(kind, **kw):
    return {"kind": kind, "kw": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}}


def make_sieve(spec, package=fruits):
    kw = {k: (tuple(v) if k == "q" else v) for k, v in spec["kw"].items()}
    return getattr(package.sieving, spec["kind"])(**kw)


def build_fruit(spec, package=fruits):
    fr = package.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fr.cut()
        for p in sl.get("preps", []):
            cls = getattr(package.preparation, p["kind"])
            if "inner" in p:
                fr.add(cls(getattr(package.preparation, p["inner"])()))
            else:
                fr.add(cls(**p.get("kw", {})))
        for i in sl["iss"]:
            ws = [package.words.SimpleWord(s) for s in i["words"]]
            weighting = None
            if "weighting" in i:
                weighting = getattr(package.iss.weighting, i["weighting"])()
            fr.add(package.ISS(ws, mode=getattr(package.ISSMode, i["mode"]),
                               semiring=getattr(package.semiring, i.get("semiring", "Reals"))(),
                               weighting=weighting))
        for s in sl["sieves"]:
            fr.add(make_sieve(s, package))
        fr.get_slice().fit_sample_size = 1.0
    return fr


# thresholds fitted on the data (no constant 0: an iterated sum of a word of L letters is exactly
# 0 at its first L - 1 positions, and so are its increments - ties with a threshold 0 by
# construction, in every series)
SIEVES = [S("NPI", q=(0.3, 0.8)), S("MPI", q=(0.2, 0.9), cut=[3, -1]), S("MAX"), S("MIN", cut=[-3, -1]),
          S("XPI", q=(0.1, 0.6)), S("LPI", q=(0.4, 1.0)), S("CUR"), S("END"),
          S("PPV", quantile=[0.3, 0.7]), S("CPV", quantile=[0.25, 0.75], segments=True)]
# (max-plus rows are staircases: their increments are exactly 0 almost everywhere and a fitted
# threshold lands ON a plateau - ties by construction, which the margin rules out; the Arctic and
# Bayesian slices therefore count with unbounded bands and carry the value sieves)
UNBOUNDED = [S("NPI", q=(-1.0, 1.0)), S("MPI", q=(-1.0, 1.0), cut=[3, -1]), S("MAX"),
             S("MIN", cut=[-3, -1]), S("CUR"), S("END")]
W22 = [str(w) for w in fruits.words.of_weight(2, dim=2)]
WORDS = ["[1]", "[2]", "[1][2]", "[11][2]"]
FRUITS = [
    {"name": "reals_indices", "slices": [
        {"preps": [{"kind": "NEW", "inner": "INC"}, {"kind": "STD"}],
         "iss": [{"words": W22, "mode": "EXTENDED", "weighting": "Indices"}], "sieves": SIEVES}]},
    {"name": "arctic", "slices": [
        {"preps": [{"kind": "INC"}],
         "iss": [{"words": WORDS, "mode": "EXTENDED", "semiring": "Arctic"}], "sieves": UNBOUNDED}]},
    {"name": "bayesian", "slices": [
        {"preps": [{"kind": "STD"}],
         "iss": [{"words": WORDS, "mode": "EXTENDED", "semiring": "Bayesian"}], "sieves": UNBOUNDED}]},
]


def margin_ok(fr, X, lengths):
    """No element of a counting sieve's row within MARGIN of one of its finite thresholds, in any
    truncated series."""
    for slc in fr:
        for n, L in enumerate(lengths):
            data = X[n:n + 1, :, :L]
            for prep in slc.get_preparateurs():
                data = prep.transform(data)
            for i, itsum in enumerate(slc._iterate_iss(data)):
                for sv in (slc._sieves_extended[i] if slc._sieves_extended else slc.get_sieves()):
                    kind = type(sv).__name__
                    if kind not in COUNTING:
                        continue
                    if kind not in ("PPV", "CPV") and not sv.requires_fitting:
                        assert all(q in (-1, 1) for q in sv._q), sv._q     # (no finite threshold)
                        continue
                    if kind in ("PPV", "CPV"):
                        rows, th = itsum, np.asarray(sv._q, dtype=np.float64)
                    else:
                        rows, th = sv._pre_transform(itsum), np.asarray(sv._quantiles, dtype=np.float64)
                    th = th[np.isfinite(th)]
                    if th.size and np.abs(rows[..., np.newaxis] - th).min() <= MARGIN:
                        return False
    return True


def generate():
    lengths = np.asarray(LENGTHS, dtype=np.int64)
    for data_seed in range(71, 91):
        X = np.random.default_rng(data_seed).standard_normal((N, D, T))
        arrays = {"X": X, "lengths": lengths}
        manifest = {"data_seed": data_seed, "shape": [N, D, T], "lengths": LENGTHS, "margin": MARGIN,
                    "counting": list(COUNTING), "fruit": []}
        good = True
        for k, spec in enumerate(FRUITS):
            fr = build_fruit(spec)
            fit_seed = 20 + k
            np.random.seed(fit_seed)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fr.fit(X)
                if not margin_ok(fr, X, lengths):
                    good = False
                    break
                out = np.concatenate([fr.transform(np.ascontiguousarray(X[n:n + 1, :, :L]))
                                      for n, L in enumerate(lengths)])
            assert out.shape == (N, fr.nfeatures()) and np.isfinite(out).all()
            arrays[f"out/{spec['name']}"] = out
            manifest["fruit"].append({
                "name": spec["name"], "spec": spec, "seed": fit_seed, "nfeatures": int(fr.nfeatures()),
                "labels": [fr.label(i) for i in range(fr.nfeatures())], "out": f"out/{spec['name']}"})
        if good:
            return arrays, manifest
        print(f"data seed {data_seed}: an element within {MARGIN} of a threshold - next seed")
    raise SystemExit("no seed keeps the margin")


if __name__ == "__main__":
    arrays, manifest = generate()
    np.savez_compressed(os.path.join(HERE, "golden_ragged.npz"), **arrays)
    with open(os.path.join(HERE, "golden_ragged.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(f"wrote {len(arrays)} arrays, {len(manifest['fruit'])} fruits, data seed {manifest['data_seed']}")
