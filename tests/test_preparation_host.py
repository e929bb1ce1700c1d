"""NRM / MAV / LAG / FFN / RIN / JLD and DIM on the host: the public surface and the seeded fits
against the reference's recorded behaviour (tests/golden/golden_prep.*), and a numpy restatement
of the transforms (fruits/preparation/transform.py:184-198, 233-239, 291-298, 362-376, 447-468,
536-543, 651-670; wrapper.py:40-44) that reproduces every golden output - the GPU tests
(test_preparation_gpu.py) use it for shapes no golden covers."""
import json
import os

import numpy as np
import pytest

import fruits_amd
from fruits_amd import _native as nat
from fruits_amd import preparation as prep

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_prep.json")) as f:
    MANIFEST = json.load(f)
ARRAYS = np.load(os.path.join(HERE, "golden", "golden_prep.npz"))
CASES = MANIFEST["prep"]
SAME_NUMPY_MAJOR = MANIFEST["numpy"].split(".")[0] == np.__version__.split(".")[0]
CALLABLES = {"third": lambda T: T // 3}
STATE = ("_kernel", "_ndim_per_kernel", "_dims_per_kernel", "_bias_weights", "_weights1", "_biases",
         "_weights2", "_w")
U = 2.0 ** -53


def make(spec, pkg=prep):
    kw = {}
    for k, v in spec.get("kw", {}).items():
        if isinstance(v, dict) and "callable" in v:
            v = CALLABLES[v["callable"]]
        elif isinstance(v, dict) and "array" in v:
            v = ARRAYS[v["array"]]
        kw[k] = v
    cls = getattr(pkg, spec["kind"])
    if spec["kind"] == "DIM":
        d = spec["dim"]
        return cls(make(spec["inner"], pkg), d if isinstance(d, int) else tuple(d))
    if spec["kind"] == "NEW":
        return cls(make(spec["inner"], pkg)) if "inner" in spec else cls()
    return cls(**kw)


def innermost(p):
    while getattr(p, "_preparateur", None) is not None:
        p = p._preparateur
    return p


def transplant(case):
    """The case's preparateur with the reference's fitted state."""
    p = make(case["spec"])
    inner = innermost(p)
    for a, v in case.get("state", {}).items():
        setattr(inner, a, v if a == "_w" else ARRAYS[v])
    return p


def has_dim(spec):
    return spec["kind"] == "DIM" or ("inner" in spec and has_dim(spec["inner"]))


# ---------------------------------------------------------------- the restatement
# Every function returns (out, terms, n): ``terms`` the sum of the absolute values of an
# element's summands and ``n`` the number of summands of that element, an array that broadcasts
# over (1, O, 1) (None where the result is exact data movement or a correctly rounded elementwise
# expression).
def np_rin(X, kernel, ndim, dims, adaptive):
    w = kernel.shape[1]
    Xp = np.pad(X, ((0, 0), (0, 0), (w, 0))) if adaptive else X
    N, _, T = Xp.shape
    out = np.zeros((N, len(ndim), T))
    terms = np.zeros_like(out)
    start = 0
    for o, cnt in enumerate(ndim):
        for j in range(start, start + cnt):
            for l in range(w):      # s += -X[i, dims[j], k-w+l] * kernel[j, l]   (:463-464)
                prod = Xp[:, dims[j], l:T - w + l] * kernel[j, l]
                out[:, o, w:] -= prod
                terms[:, o, w:] += np.abs(prod)
            out[:, o, w:] += Xp[:, j, w:]       # X[i, j, k]: dimension j, not dims[j]   (:465)
            terms[:, o, w:] += np.abs(Xp[:, j, w:])
        start += cnt
    n = (np.asarray(ndim, dtype=np.float64) * (w + 1))[None, :, None]     # w products + the self term per slot
    if adaptive:
        return out[:, :, w:], terms[:, :, w:], n
    return out, terms, n


def np_mav(X, w):
    out = np.zeros_like(X)
    terms = np.zeros_like(X)
    T = X.shape[2]
    for l in range(w):
        out[:, :, w - 1:] += X[:, :, l:T - w + 1 + l]
        terms[:, :, w - 1:] += np.abs(X[:, :, l:T - w + 1 + l])
    return out / w, terms / w, np.full((1, X.shape[1], 1), float(w))


def np_jld(X, kernel, bias, ndim, dims):
    out = np.zeros((X.shape[0], len(ndim), X.shape[2]))
    terms = np.zeros_like(out)
    start = 0
    for o, cnt in enumerate(ndim):
        for j in range(start, start + cnt):
            out[:, o, :] += X[:, dims[j], :] * kernel[j] + bias[o]      # (:666-668)
            terms[:, o, :] += np.abs(X[:, dims[j], :] * kernel[j]) + abs(bias[o])
        start += cnt
    return out, terms, (2.0 * np.asarray(ndim, dtype=np.float64))[None, :, None]    # product + bias per slot


def np_ffn(X, W1, b, W2, center, relu_out):
    Z = X - X.mean(axis=2, keepdims=True) if center else X
    hidden = np.einsum("hd,ndt->nht", W1, Z) + b[None, :, None]
    hidden = hidden * (hidden > 0)          # the relu as a multiply: keeps -0.0 and NaN
    y = np.einsum("oh,nht->not", W2, hidden)
    return y * (y > 0) if relu_out else y


def np_nrm(X, scale_dim):
    mn, mx = np.min(X, axis=2), np.max(X, axis=2)
    if scale_dim:
        mn = np.repeat(np.min(mn, axis=1)[:, None], X.shape[1], axis=1)
        mx = np.repeat(np.max(mx, axis=1)[:, None], X.shape[1], axis=1)
    out = np.zeros_like(X)
    mask = mn != mx
    out[mask] = (X[mask] - mn[mask][:, None]) / (mx[mask] - mn[mask])[:, None]
    return out


def np_lag(X):
    s = np.arange(2 * X.shape[2] - 1)
    out = np.zeros((X.shape[0], 2 * X.shape[1], s.size))
    out[:, 0::2, :] = X[:, :, (s + 1) // 2]
    out[:, 1::2, :] = X[:, :, s // 2]
    return out


def np_apply(p, X, detail=False):
    """The transform of a FITTED fruits_amd preparateur (its state, numpy arithmetic)."""
    kind = type(p).__name__
    terms = n = None
    if kind == "NRM":
        out = np_nrm(X, p._scale_dim)
    elif kind == "LAG":
        out = np_lag(X)
    elif kind == "MAV":
        if p._w > X.shape[2]:
            out = np.zeros_like(X)
        else:
            out, terms, n = np_mav(X, p._w)
    elif kind == "RIN":
        if not p._adaptive_width and p._kernel.shape[1] >= X.shape[2]:
            out = np.zeros((X.shape[0], len(p._ndim_per_kernel), X.shape[2]))
        else:
            out, terms, n = np_rin(X, p._kernel, p._ndim_per_kernel, p._dims_per_kernel,
                                   p._adaptive_width)
    elif kind == "JLD":
        out, terms, n = np_jld(X, p._kernel, p._bias_weights, p._ndim_per_kernel,
                               p._dims_per_kernel)
    elif kind == "FFN":
        out = np_ffn(X, p._weights1, p._biases, p._weights2, p._center, p._relu_out)
    elif kind == "INC":
        assert p._depth == 1 and p._zero_padding and p._shift == 1
        out = np.zeros_like(X)
        out[:, :, 1:] = X[:, :, 1:] - X[:, :, :-1]
    elif kind == "NEW":
        extra = X if p._preparateur is None else np_apply(p._preparateur, X)
        out = np.concatenate((X, extra), axis=1)
    elif kind == "DIM":
        tr = np_apply(p._preparateur, X[:, p._dim, :])
        out = np.concatenate((np.delete(X, p._dim, axis=1), tr), axis=1)
    else:
        raise NotImplementedError(kind)
    return (out, terms, n) if detail else out


# ---------------------------------------------------------------- surface
def _no_address(text):
    """A callable width prints its address."""
    import re
    return re.sub(r" at 0x[0-9a-f]+", "", text)


def test_all_exports():
    names = {"NRM", "MAV", "LAG", "FFN", "RIN", "JLD", "INC", "STD"}
    assert names <= set(prep.transform.__all__)
    assert names <= set(MANIFEST["all_transform"])
    assert sorted(prep.wrapper.__all__) == sorted(MANIFEST["all_wrapper"])
    for n in names | {"DIM", "NEW"}:
        assert hasattr(fruits_amd.preparation, n)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_surface(case):
    if case.get("raises_at") == "init":
        with pytest.raises(ValueError if case["reference_raises"] == "ValueError" else TypeError):
            make(case["spec"])
        return
    p = make(case["spec"])
    if not has_dim(case["spec"]) or SAME_NUMPY_MAJOR:     # (DIM prints numpy scalars)
        assert _no_address(str(p)) == _no_address(case["str"])
        assert _no_address(str(p.copy())) == _no_address(case["copy_str"])
        assert p.label() == str(p)
    assert p.requires_fitting == case["requires_fitting"]
    if case["eq_copy"] == "ValueError":
        with pytest.raises(ValueError):
            p == p.copy()
    else:
        assert (p == p.copy()) == case["eq_copy"]
    assert type(p.copy()) is type(p) and p.copy() is not p


def test_literal_strings():
    assert str(prep.NRM()) == "NRM(False)" and str(prep.LAG()) == "LAG()"
    assert str(prep.MAV()) == "MAV(5)" and str(prep.FFN()) == "FFN(1, None, True, False)"
    assert str(prep.RIN()) == "RIN(1, False, -1, False, None)"
    assert str(prep.JLD()) == "JLD(0.99, False, False)"
    assert prep.NRM(True) == prep.NRM(True) and prep.NRM(True) != prep.NRM()
    assert prep.MAV(3) == prep.MAV(3) and prep.MAV(3) != prep.MAV(4)
    assert prep.LAG() == prep.LAG() and prep.RIN(2) == prep.RIN(2) and prep.RIN(2) != prep.RIN(3)
    assert prep.JLD(2) == prep.JLD(2) and prep.JLD(2, bias=True) != prep.JLD(2)
    assert not (prep.FFN() == prep.FFN())        # (the reference defines no FFN.__eq__)
    assert not prep.NRM().requires_fitting and not prep.LAG().requires_fitting
    assert prep.DIM(prep.LAG(), 0).requires_fitting is False
    assert prep.DIM(prep.RIN(), 0).requires_fitting is True


# ---------------------------------------------------------------- seeded fits
@pytest.mark.parametrize("case", [c for c in CASES if c.get("raises_at") != "init"],
                         ids=lambda c: c["name"])
def test_seeded_fit_reproduces_reference_state(case):
    p = make(case["spec"])
    X = ARRAYS[case["x"]]
    np.random.seed(case["seed"])
    if case.get("raises_at") == "fit":
        with pytest.raises(ValueError):
            p.fit(X)
        return
    p.fit(X)
    inner = innermost(p)
    assert {a for a in STATE if hasattr(inner, a)} == set(case["state"])
    for a, v in case["state"].items():
        got = getattr(inner, a)
        if a == "_w":
            assert got == v
            continue
        ref = ARRAYS[v]
        assert got.dtype == ref.dtype and got.shape == ref.shape, a
        np.testing.assert_array_equal(got, ref, err_msg=a)
    if case.get("raises_at") == "transform":     # MAV(-1): no width, transform.py:250-260
        with pytest.raises(RuntimeError):
            p.transform(X)


def test_fit_looks_at_the_shape_only():
    """A fruit hands these fits a stand-in of the PREPARED shape, never the data."""
    for p in (prep.MAV(0.5), prep.FFN(2), prep.RIN(3), prep.JLD(2), prep.DIM(prep.RIN(2), (0, 2)),
              prep.NEW(prep.JLD(1))):
        assert p._fit_needs_shape() and not p._fit_needs_data()
        np.random.seed(5)
        p.fit(np.broadcast_to(0.0, (9, 3, 20)))
        a = {k: v for k, v in vars(innermost(p)).items() if k in STATE}
        q = p.copy()
        np.random.seed(5)
        q.fit(np.random.default_rng(1).standard_normal((9, 3, 20)))
        b = {k: v for k, v in vars(innermost(q)).items() if k in STATE}
        assert a.keys() == b.keys() and a
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
    for p in (prep.NRM(), prep.LAG(), prep.DIM(prep.LAG(), 0)):
        assert not p._fit_needs_shape() and not p._fit_needs_data()


def test_unfitted_errors():
    X = np.zeros((2, 2, 6))
    for p, err in ((prep.MAV(), RuntimeError), (prep.FFN(), RuntimeError),
                   (prep.RIN(), RuntimeError), (prep.JLD(2), AttributeError),
                   (prep.DIM(prep.RIN(), 0), RuntimeError), (prep.NEW(prep.FFN()), RuntimeError)):
        with pytest.raises(err):
            p.transform(X)


# ---------------------------------------------------------------- the restatement is the reference
@pytest.mark.parametrize("case", [c for c in CASES if "out" in c], ids=lambda c: c["name"])
def test_numpy_restatement_matches_reference(case):
    p = transplant(case)
    got = np_apply(p, ARRAYS[case["x"]])
    ref = ARRAYS[case["out"]]
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(ref).max()))


def test_no_device_means_native_error():
    if nat.device_count() > 0:
        out = prep.LAG().fit_transform(np.zeros((2, 1, 4)))
        assert out.shape == (2, 2, 7)
        return
    X = np.random.default_rng(0).standard_normal((3, 2, 12))
    for p in (prep.NRM(), prep.MAV(3), prep.LAG(), prep.FFN(), prep.RIN(2), prep.JLD(2),
              prep.DIM(prep.RIN(), 0), prep.NEW(prep.RIN())):
        with pytest.raises(nat.NativeError):
            p.fit_transform(X)


def test_kernels_use_no_scratch(tmp_path):
    """The four preparateur kernels keep everything in registers and LDS: their kernel
    descriptors ask for no private segment."""
    import re
    import subprocess
    from fruits_amd import build
    try:
        cc = build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc is not installed")
    asm = str(tmp_path / "kernels_prep.s")
    subprocess.check_call([cc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                           "--cuda-device-only", "-S", "-x", "hip",
                           os.path.join(build.CSRC, "kernels_prep.hip"), "-o", asm])
    text = open(asm).read()
    for name in ("prep_fir_kernel", "prep_project_kernel", "prep_normalize_kernel",
                 "prep_leadlag_kernel"):
        sizes = re.findall(r"\.amdhsa_kernel \S*" + name
                           + r"[\s\S]*?\.amdhsa_private_segment_fixed_size (\d+)", text)
        assert sizes == ["0"], (name, sizes)


def test_pickle_keeps_the_fitted_state_only():
    """A fitted preparateur travels between ranks as a pickle: its state goes along, the
    device copies of it do not."""
    import pickle
    for p in (prep.RIN(3, out_dim=2), prep.JLD(2, bias=True), prep.FFN(2), prep.MAV(0.25),
              prep.DIM(prep.RIN(2), (0, 2))):
        np.random.seed(2)
        p.fit(np.broadcast_to(0.0, (5, 3, 30)))
        innermost(p)._programs = {"cuda:0": "device copies"}
        q = pickle.loads(pickle.dumps(p))
        a, b = vars(innermost(p)), vars(innermost(q))
        assert b.get("_programs", {}) == {}
        for k in STATE:
            assert (k in a) == (k in b)
            if k in a:
                np.testing.assert_array_equal(a[k], b[k])
        assert str(q) == str(p)
