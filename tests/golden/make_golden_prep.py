#!/usr/bin/env python3
"""Generate tests/golden/golden_prep.{npz,json}: the reference's NRM / MAV / LAG / FFN / RIN / JLD
preparateurs (fruits/preparation/transform.py:161-568, 616-746), DIM / NEW around them
(wrapper.py) and three whole fruits that start with them.

TEST INFRASTRUCTURE - runs only where the reference tree is at hand, never on the GPU box.  The
reference is imported with the two loader accommodations of make_golden_sieves.py (a ``numba``
stand-in whose ``njit`` returns the function unchanged and whose ``prange`` is ``range``;
``np.NINF`` for numpy >= 2); they change no arithmetic.  Only DATA is written.

A preparateur is described by a spec ``{"kind", "kw"[, "inner", "dim"]}``; two keyword values
are encoded: ``{"callable": "third"}`` (``lambda T: T // 3``) and ``{"array": key}``.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_prep.py
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
manifest = {"numpy": np.__version__, "all_transform": list(fruits.preparation.transform.__all__),
            "all_wrapper": list(fruits.preparation.wrapper.__all__), "prep": [], "fruit": []}
STATE = ("_kernel", "_ndim_per_kernel", "_dims_per_kernel", "_bias_weights", "_weights1", "_biases",
         "_weights2", "_w")
CALLABLES = {"third": lambda T: T // 3}


def put(name, arr):
    assert name not in arrays, name
    arrays[name] = np.ascontiguousarray(arr)
    return name


def make(spec, pkg):
    """Builds the preparateur of a spec from ``pkg`` (a ``preparation`` package)."""
    kw = {}
    for k, v in spec.get("kw", {}).items():
        if isinstance(v, dict) and "callable" in v:
            v = CALLABLES[v["callable"]]
        elif isinstance(v, dict) and "array" in v:
            v = arrays[v["array"]]
        kw[k] = v
    cls = getattr(pkg, spec["kind"])
    if spec["kind"] == "DIM":
        d = spec["dim"]
        return cls(make(spec["inner"], pkg), d if isinstance(d, int) else tuple(d))
    if spec["kind"] == "NEW":
        return cls(make(spec["inner"], pkg)) if "inner" in spec else cls()
    return cls(**kw)


def innermost(p):
    while hasattr(p, "_preparateur") and p._preparateur is not None:
        p = p._preparateur
    return p


def prep_case(name, x_key, spec, seed=0):
    X = arrays[x_key]
    entry = {"name": name, "x": x_key, "spec": spec, "seed": seed}
    try:
        p = make(spec, fruits.preparation)
    except (ValueError, TypeError) as err:
        entry["reference_raises"] = type(err).__name__
        entry["raises_at"] = "init"
        manifest["prep"].append(entry)
        return
    try:
        eq = bool(p == p.copy())
    except ValueError:      # (RIN compares a given kernel array with ==, transform.py:560)
        eq = "ValueError"
    entry.update({"str": str(p), "copy_str": str(p.copy()),
                  "requires_fitting": bool(p.requires_fitting), "eq_copy": eq})
    try:
        np.random.seed(seed)
        p.fit(X)
        state = {}
        inner = innermost(p)
        for a in STATE:
            if hasattr(inner, a):
                v = getattr(inner, a)
                state[a] = int(v) if a == "_w" else put(f"state/{name}/{a}", v)
        entry["state"] = state
        out = p.transform(X)
    except (ValueError, RuntimeError) as err:
        entry["reference_raises"] = type(err).__name__
        entry["raises_at"] = "transform" if "state" in entry else "fit"
    else:
        entry["out"] = put(f"out/{name}", out)
    manifest["prep"].append(entry)


def S(kind, **kw):
    return {"kind": kind, "kw": kw}


# the vectors of the reference's tests/preparation/test_transform.py
put("X_1", np.array([
    [[-4, 0.8, 0, 5, -3], [2.0, 1, 0, 0, -7]],
    [[5.0, 8, 2, 6, 0], [-5, -1, -4, -0.5, -8]],
]))
rng = np.random.default_rng(51)
put("R_12_4_96", rng.standard_normal((12, 4, 96)).cumsum(axis=2))
put("R_4_4_40", rng.standard_normal((4, 4, 40)).cumsum(axis=2))
put("R_3_3_33", rng.standard_normal((3, 3, 33)))
put("R_4_2_1", rng.standard_normal((4, 2, 1)))
put("R_4_2_2", rng.standard_normal((4, 2, 2)))
const = rng.standard_normal((6, 3, 20))
const[1, 2, :] = 0.75          # a constant row
const[4, :, :] = -2.5          # a constant series
put("C_6_3_20", const)
put("K_4_3", np.random.default_rng(52).standard_normal((4, 3)))
put("K_2_2", np.array([[0.5, -1.0], [2.0, 0.25]]))

for x in ("X_1", "R_4_4_40", "R_3_3_33"):
    T = arrays[x].shape[2]
    D = arrays[x].shape[1]
    prep_case(f"nrm_{x}", x, S("NRM"))
    prep_case(f"nrm_{x}_scale", x, S("NRM", scale_dim=True))
    prep_case(f"lag_{x}", x, S("LAG"))
    prep_case(f"mav_{x}", x, S("MAV"))
    prep_case(f"mav_{x}_w2", x, S("MAV", width=2))
    prep_case(f"mav_{x}_w1", x, S("MAV", width=1))
    prep_case(f"mav_{x}_wT", x, S("MAV", width=T))
    prep_case(f"mav_{x}_f", x, S("MAV", width=0.3))
    prep_case(f"mav_{x}_neg", x, S("MAV", width=-1))
    for tag, w in (("1", 1), ("4", 4), ("Tm1", T - 1), ("Tp5", T + 5)):
        prep_case(f"rin_{x}_w{tag}", x, S("RIN", width=w), seed=w)
    prep_case(f"rin_{x}_call", x, S("RIN", width={"callable": "third"}), seed=7)
    prep_case(f"rin_{x}_adapt", x, S("RIN", width=3, adaptive_width=True), seed=8)
    prep_case(f"rin_{x}_out1", x, S("RIN", width=2, out_dim=1), seed=9)
    prep_case(f"rin_{x}_out2", x, S("RIN", width=2, out_dim=2), seed=10)
    prep_case(f"rin_{x}_out9", x, S("RIN", width=2, out_dim=9), seed=10)
    prep_case(f"rin_{x}_sum1", x, S("RIN", width=4, force_sum_one=True), seed=11)
    prep_case(f"jld_{x}_1", x, S("JLD", dim=1), seed=12)
    prep_case(f"jld_{x}_3", x, S("JLD", dim=3, bias=True), seed=13)
    prep_case(f"jld_{x}_dist", x, S("JLD", dim=2, distribute=True, bias=True), seed=14)
    prep_case(f"jld_{x}_dist9", x, S("JLD", dim=9, distribute=True), seed=14)
    if x == "X_1":
        prep_case(f"jld_{x}_float", x, S("JLD", dim=0.9), seed=15)
    for c in (True, False):
        for r in (True, False):
            prep_case(f"ffn_{x}_c{int(c)}r{int(r)}", x, S("FFN", d_out=2, center=c, relu_out=r),
                      seed=16 + 2 * c + r)
    prep_case(f"ffn_{x}_h5", x, S("FFN", d_out=3, d_hidden=5), seed=21)
    prep_case(f"dim_{x}_0", x, {"kind": "DIM", "inner": S("RIN", width=2), "dim": 0}, seed=22)
    prep_case(f"dim_{x}_10", x, {"kind": "DIM", "inner": S("JLD", dim=1), "dim": [1, 0]}, seed=23)
    prep_case(f"dim_{x}_new_inc", x, {"kind": "DIM", "inner": {"kind": "NEW", "inner": S("INC")},
                                      "dim": 0}, seed=24)
    prep_case(f"new_{x}_rin", x, {"kind": "NEW", "inner": S("RIN")}, seed=25)
    prep_case(f"dim_{x}_all_nrm", x, {"kind": "DIM", "inner": S("NRM", scale_dim=True),
                                      "dim": list(range(D))}, seed=26)
prep_case("rin_kernel", "R_12_4_96", S("RIN", kernel={"array": "K_4_3"}))
prep_case("rin_kernel_adapt", "R_12_4_96", S("RIN", kernel={"array": "K_4_3"}, adaptive_width=True))
prep_case("rin_kernel_x1", "X_1", S("RIN", kernel={"array": "K_2_2"}))
prep_case("lag_T1", "R_4_2_1", S("LAG"))
prep_case("lag_T2", "R_4_2_2", S("LAG"))
prep_case("nrm_T1", "R_4_2_1", S("NRM"))
prep_case("nrm_const", "C_6_3_20", S("NRM"))
prep_case("nrm_const_scale", "C_6_3_20", S("NRM", scale_dim=True))
prep_case("mav_float_bad", "X_1", S("MAV", width=1.5))
prep_case("jld_float_bad", "X_1", S("JLD", dim=1.5))


# whole fruits (fit_sample_size = 1.0: the fit sample is the whole input)
def build_fruit(spec, pkg):
    fr = pkg.Fruit(spec.get("name", ""))
    for sl in spec["slices"]:
        fr.cut()
        for p in sl.get("preps", []):
            fr.add(make(p, pkg.preparation))
        for i in sl["iss"]:
            ws = [pkg.words.SimpleWord(s) for s in i["words"]]
            fr.add(pkg.ISS(ws, mode=getattr(pkg.ISSMode, i["mode"]),
                           semiring=getattr(pkg.semiring, i.get("semiring", "Reals"))()))
        for s in sl["sieves"]:
            kw = {k: (tuple(v) if k == "q" else v) for k, v in s.items() if k != "kind"}
            fr.add(getattr(pkg.sieving, s["kind"])(**kw))
        fr.get_slice().fit_sample_size = 1.0
    return fr


def fruit_case(name, x_key, spec, seed):
    X = arrays[x_key]
    fr = build_fruit(spec, fruits)
    np.random.seed(seed)
    fr.fit(X)
    out = fr.transform(X)
    prepared = X
    for p in fr.get_slice()._preparateurs:
        prepared = p.transform(prepared)
    manifest["fruit"].append({
        "name": name, "x": x_key, "spec": spec, "seed": seed, "nfeatures": int(fr.nfeatures()),
        "labels": [fr.label(i) for i in range(fr.nfeatures())],
        "summary": fr.summary(), "prepared": put(f"fruit/{name}/prepared", prepared),
        "out": put(f"fruit/{name}", out)})


put("F_12_3_64", np.random.default_rng(55).standard_normal((12, 3, 64)).cumsum(axis=2))
put("F_10_1_48", np.random.default_rng(56).standard_normal((10, 1, 48)))
W23 = [str(w) for w in fruits.words.of_weight(2, dim=3)]
W22 = [str(w) for w in fruits.words.of_weight(2, dim=2)]
fruit_case("rin_reals", "F_12_3_64", {"name": "rin", "slices": [
    {"preps": [S("RIN", width=4)], "iss": [{"words": W23, "mode": "EXTENDED"}],
     "sieves": [{"kind": "NPI"}, {"kind": "MPI"}, {"kind": "END"}]}]}, seed=31)
fruit_case("nrm_lag_arctic", "F_10_1_48", {"name": "leadlag", "slices": [
    {"preps": [S("NRM"), S("LAG")],
     "iss": [{"words": ["[1]", "[2]", "[1][2]", "[11][2]"], "mode": "EXTENDED",
              "semiring": "Arctic"}],
     "sieves": [{"kind": "MAX", "cut": [20, -1]}, {"kind": "END", "cut": [10, -1]}]}]}, seed=32)
fruit_case("dim_jld_ffn", "F_12_3_64", {"name": "mixed", "slices": [
    {"preps": [{"kind": "DIM", "inner": S("MAV", width=5), "dim": 0},
               S("JLD", dim=2, bias=True), S("FFN", d_out=2)],
     "iss": [{"words": W22, "mode": "EXTENDED"}],
     "sieves": [{"kind": "XPI"}, {"kind": "NPI", "q": [0.25, 0.5, 0.75, 1.0]}]}]}, seed=33)

np.savez_compressed(os.path.join(HERE, "golden_prep.npz"), **arrays)
with open(os.path.join(HERE, "golden_prep.json"), "w") as f:
    json.dump(manifest, f, indent=1)
print(f"wrote {len(arrays)} arrays, {len(manifest['prep'])} preparateur cases, "
      f"{sum('reference_raises' in c for c in manifest['prep'])} of them raising, "
      f"{len(manifest['fruit'])} fruits")
