#!/usr/bin/env python3
"""Generate tests/golden/golden_implicit.{npz,json}: the reference's PPV / CPV sieves
(fruits/sieving/implicit.py) - their class surface, their outputs on small inputs with the edge
cases of a closed-below test, and whole fruits that use them.

TEST INFRASTRUCTURE - runs only where the reference tree is at hand, never on the GPU box.  The
reference is imported with the two loader accommodations of make_golden.py (a ``numba`` stand-in
whose ``njit`` returns the function unchanged and whose ``prange`` is ``range``; ``np.NINF``
for numpy >= 2); they change no arithmetic.  Only DATA is written.

A sieve is written down as ``{"kind": "PPV", "kw": {...}}`` (``{"kind": "INC", "sieve": {...}}``
for a wrapper); the tests build theirs from it.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_implicit.py
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
sys.path.insert(0, os.path.dirname(HERE))     # tests/: implicit_ref


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
import implicit_ref as iref  # noqa: E402

arrays = {}
manifest = {"sieve": [], "raises": [], "fruit": []}
EXPOSED_SHARE_CAP = 0.10


def put(name, arr):
    assert name not in arrays, name
    arrays[name] = np.ascontiguousarray(arr)
    return name


def S(kind, sieve=None, **kw):
    spec = {"kind": kind, "kw": {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}}
    if sieve is not None:
        spec["sieve"] = sieve
    return spec


def make(spec, package=fruits):
    kw = {k: (tuple(v) if k == "q" else v) for k, v in spec["kw"].items()}
    cls = getattr(package.sieving, spec["kind"])
    if "sieve" in spec:
        return cls(make(spec["sieve"], package), **kw)
    return cls(**kw)


def sieve_case(name, x_key, spec, seed=0):
    """The class surface and a seeded fit_transform on one (N, T) array."""
    X = arrays[x_key]
    sv = make(spec)
    entry = {"name": name, "spec": spec, "x": x_key, "seed": seed,
             "labels": [sv.label(i) for i in range(sv.nfeatures())],
             "str": str(sv), "summary": sv.summary(), "nfeatures": int(sv.nfeatures()),
             "requires_fitting": bool(sv.requires_fitting), "copy_str": str(sv.copy()),
             "copy_summary": sv.copy().summary(),
             "pairs": [[float(a), bool(b)] for a, b in sv._q_c_input]}
    np.random.seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sv.fit(X)
        entry["state_after_fit"] = int(np.random.get_state()[1][:4].sum())
        entry["pos_after_fit"] = int(np.random.get_state()[2])
        entry["out"] = put(f"sieve/{name}", sv.transform(X))
    entry["thresholds"] = put(f"sieve_q/{name}", np.asarray(sv._q, dtype=np.float64))
    manifest["sieve"].append(entry)


def raises_case(name, kind, args, kw):
    try:
        getattr(fruits.sieving, kind)(*args, **kw)
    except ValueError as e:
        manifest["raises"].append({"name": name, "kind": kind, "args": args, "kw": kw,
                                   "message": str(e)})
        return
    raise AssertionError(name)


# ---------------------------------------------------------------- inputs
X_1 = np.array([
    [[-4, 0.8, 0, 5, -3], [2.0, 1, 0, 0, -7]],
    [[5.0, 8, 2, 6, 0], [-5, -1, -4, -0.5, -8]],
])
put("X_1_0", X_1[0])
put("X_1_1", X_1[1])
for T in (1, 2, 7, 64):
    put(f"E_{T}", iref.edge_rows(T, np.random.default_rng(100 + T)))
put("R_6_40", np.random.default_rng(51).standard_normal((6, 40)).cumsum(axis=1))

# ---------------------------------------------------------------- the cases of tests/sieving/test_implicit.py
sieve_case("t_ppv_1", "X_1_0", S("PPV", quantile=0, constant=True))
sieve_case("t_ppv_2", "X_1_1", S("PPV", quantile=0.5, constant=False, sample_size=1))
sieve_case("t_cpv_1", "X_1_0", S("CPV", quantile=0, constant=True))
sieve_case("t_group_1", "X_1_1", S("PPV", quantile=[0.5, 0.1, 0.7], constant=False, sample_size=1,
                                   segments=False))
sieve_case("t_group_2", "X_1_1", S("PPV", quantile=[0.5, 0.1, 0.7], constant=False, sample_size=1,
                                   segments=True))
sieve_case("t_group_3", "X_1_1", S("PPV", quantile=[-5, 0, 2], constant=True, sample_size=1,
                                   segments=False))
sieve_case("t_group_4", "X_1_1", S("PPV", quantile=[0, -5, 2], constant=True, sample_size=1,
                                   segments=True))
raises_case("r_prob_range", "PPV", [], {"quantile": [0.5, 0.1, -1], "constant": [False, True, False]})
raises_case("r_prob_range_cpv", "CPV", [], {"quantile": [0.5, 2], "constant": False})
raises_case("r_lengths", "PPV", [], {"quantile": [0.5, 0.1], "constant": [False]})
raises_case("r_single_list", "PPV", [], {"quantile": 0.5, "constant": [False, True]})
raises_case("r_sample_zero", "PPV", [], {"sample_size": 0})
raises_case("r_sample_big", "CPV", [], {"sample_size": 1.5})
raises_case("r_segments_one", "PPV", [], {"quantile": [0.5], "segments": True})
raises_case("r_segments_scalar", "CPV", [], {"quantile": 0.5, "segments": True})

# ---------------------------------------------------------------- edge cases
for kind in ("PPV", "CPV"):
    k = kind.lower()
    for x in ("E_1", "E_2", "E_7", "E_64"):
        # thresholds ON data values: >= against >, < against <=
        sieve_case(f"{k}_{x}_on_values", x, S(kind, quantile=[-2, -1, 0, 1, 2], constant=True))
        sieve_case(f"{k}_{x}_segments", x, S(kind, quantile=[-1, 0, 2], constant=True, segments=True))
        sieve_case(f"{k}_{x}_default", x, S(kind))
        # pairs by position of list(set(...)), then sorted; a fitted threshold above a constant
        # one: an empty band
        sieve_case(f"{k}_{x}_mixed_segments", x, S(kind, quantile=[0.9, 1.0], constant=[False, True],
                                                   segments=True))
        sieve_case(f"{k}_{x}_dup_segments", x, S(kind, quantile=[1, 0, 1, -2], constant=True,
                                                 segments=True))
    sieve_case(f"{k}_real", "R_6_40", S(kind, quantile=[0.2, 0.5, 0.9]))
    sieve_case(f"{k}_real_segments", "R_6_40", S(kind, quantile=[0.1, 0.5, 0.8, 1.0],
                                                 constant=[False, False, False, True], segments=True))
    sieve_case(f"{k}_real_sampled", "R_6_40", S(kind, quantile=[0.3, 0.7], sample_size=0.5), seed=7)


# ---------------------------------------------------------------- whole fruits
def build_fruit(spec, package=fruits):
    fr = package.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fr.cut()
        for p in sl.get("preps", []):
            fr.add(getattr(package.preparation, p["kind"])(**p.get("kw", {})))
        for i in sl["iss"]:
            ws = [package.words.SimpleWord(s) for s in i["words"]]
            fr.add(package.ISS(ws, mode=getattr(package.ISSMode, i["mode"]),
                               semiring=getattr(package.semiring, i.get("semiring", "Reals"))()))
        for s in sl["sieves"]:
            fr.add(make(s, package))
        fr.get_slice().fit_sample_size = 1.0
    return fr


def fruit_case(name, x_key, spec, seed):
    X = arrays[x_key]
    fr = build_fruit(spec)
    np.random.seed(seed)
    fr.fit(X)
    state = np.random.get_state()
    out = fr.transform(X)
    # the fitted thresholds of every PPV / CPV copy, and the share of entries per column with an
    # element within 1e-10 of one of them (implicit_ref.exposure): the reference alone has to
    # stay within the cap the device test holds the features to
    thresholds, expo = [], []
    for si, slc in enumerate(fr):
        data = X
        for prep in slc.get_preparateurs():
            data = prep.transform(data)
        per_slice = []
        for i, itsum in enumerate(slc._iterate_iss(data)):
            row = []
            for j, sv in enumerate(slc._sieves_extended[i]):
                if isinstance(sv, fruits.sieving.PPV):
                    key = put(f"fruit_q/{name}/{si}/{i}/{j}", np.asarray(sv._q, dtype=np.float64))
                    row.append(key)
                    expo.append(iref.exposure(itsum, np.asarray(sv._q), sv._segments))
                else:
                    row.append(None)
                    expo.append(np.zeros((X.shape[0], sv.nfeatures()), dtype=np.int64))
            per_slice.append(row)
        thresholds.append(per_slice)
    expo = np.concatenate(expo, axis=1)
    assert expo.shape == out.shape, (expo.shape, out.shape)
    share = (expo > 0).mean(axis=0)
    bad = np.nonzero(share > EXPOSED_SHARE_CAP)[0]
    assert not len(bad), (name, [(fr.label(int(c)), float(share[c])) for c in bad[:12]], len(bad))
    manifest["fruit"].append({
        "name": name, "x": x_key, "spec": spec, "seed": seed, "nfeatures": int(fr.nfeatures()),
        "labels": [fr.label(i) for i in range(fr.nfeatures())], "summary": fr.summary(),
        "out": put(f"fruit/{name}", out), "thresholds": thresholds,
        "exposed_share_max": float(share.max()), "exposed_entries": int((expo > 0).sum()),
        "state_pos": int(state[2]),
        "state_key": put(f"fruit_state/{name}", np.asarray(state[1], dtype=np.uint32))})


put("F_12_2_120", np.random.default_rng(61).standard_normal((12, 2, 120)))
put("F_11_2_100", np.random.default_rng(62).standard_normal((11, 2, 100)))
W42 = [str(w) for w in fruits.words.of_weight(4, dim=2)]
W22 = [str(w) for w in fruits.words.of_weight(2, dim=2)]
W12 = [str(w) for w in fruits.words.of_weight(1, dim=2)]
# The fruit of the reference's tests/core/test_fruit.py:11-28, its PPV sieves in place.  Its
# constant threshold 0 is 0.5 here, and no other constant threshold of these fruits is 0: an
# iterated sum of a word of L letters is exactly 0 at its first L - 1 positions, which the
# exposure rule counts as ties with a threshold 0 in every series (the integer tests of
# test_implicit_gpu.py put thresholds on data values instead).
fruit_case("test_fruit", "F_12_2_120", {"name": "", "slices": [
    {"preps": [{"kind": "INC", "kw": {"zero_padding": False}}],
     "iss": [{"words": W42, "mode": "SINGLE"}],
     "sieves": [S("PPV", quantile=0.5, constant=True),
                S("PPV", quantile=0.2, constant=False, sample_size=1),
                S("PPV", quantile=[0.2, 5], constant=[False, True], sample_size=1, segments=True),
                S("MAX", cut=[0.1, 0.5, 0.9]), S("MIN", cut=[0.1, 0.5, 0.9])]}]}, seed=11)
fruit_case("cpv_one_slice", "F_12_2_120", {"name": "cpv", "slices": [
    {"preps": [{"kind": "INC"}], "iss": [{"words": W22, "mode": "EXTENDED"}],
     "sieves": [S("CPV", quantile=0.5), S("PPV", quantile=[0.2, 0.5, 0.9]),
                S("CPV", quantile=[0.25, 2], constant=True, segments=True),
                S("MAX"), S("END")]}]}, seed=12)
fruit_case("cpv_two_slices", "F_11_2_100", {"name": "two", "slices": [
    {"preps": [{"kind": "INC"}], "iss": [{"words": W22, "mode": "EXTENDED"}],
     "sieves": [S("NPI", q=(0.3, 1.0)), S("CPV", quantile=[0.35, 0.75], segments=True),
                S("PPV", quantile=[0.25, 0.125], constant=[False, True])]},
    {"iss": [{"words": W12 + ["[1][2]", "[12][1]"], "mode": "SINGLE"}],
     "sieves": [S("PPV", quantile=0.6), S("CPV", quantile=[0.4, 0.8]), S("END")]}]}, seed=13)
fruit_case("ppv_sampled", "F_11_2_100", {"name": "sampled", "slices": [
    {"preps": [{"kind": "INC"}], "iss": [{"words": W22, "mode": "SINGLE"}],
     "sieves": [S("PPV", quantile=[0.3, 0.7], sample_size=0.5), S("CPV", quantile=0.5, sample_size=0.5),
                S("END")]}]}, seed=14)

if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "golden_implicit.npz"), **arrays)
    with open(os.path.join(HERE, "golden_implicit.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print(f"wrote {len(arrays)} arrays, {len(manifest['sieve'])} sieve cases, "
          f"{len(manifest['raises'])} refusals, {len(manifest['fruit'])} fruits "
          f"(exposed share per fruit {[c['exposed_share_max'] for c in manifest['fruit']]})")
