"""PPV / CPV (fruits/sieving/implicit.py) without a device: the class surface against strings
recorded from the reference (tests/golden/golden_implicit.json, make_golden_implicit.py), the
numpy restatement the device tests compare with against the reference's recorded outputs, the
host fit's draws from numpy's global generator, the argument checks of fr_sieve_implicit, and
which slices fuse."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fruits_amd as fr
from fruits_amd import _native as nat
from fruits_amd.sieving import CPV, END, INC, NPI, PPV

import implicit_ref as iref

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "golden_implicit.json")) as _f:
    MANIFEST = json.load(_f)
ARRAYS = np.load(os.path.join(HERE, "golden", "golden_implicit.npz"))
KINDS = {"PPV": PPV, "CPV": CPV}


def make_sieve(spec):
    return KINDS[spec["kind"]](**spec["kw"])


# ---------------------------------------------------------------- class surface
@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_surface(case):
    sv = make_sieve(case["spec"])
    assert str(sv) == case["str"]
    assert sv.summary() == case["summary"]
    assert sv.nfeatures() == case["nfeatures"]
    assert [sv.label(i) for i in range(sv.nfeatures())] == case["labels"]
    assert sv.requires_fitting == case["requires_fitting"]
    # (the pairing of list(set(quantile)) with `constant` by position, then sorted)
    assert [[float(a), bool(b)] for a, b in sv._q_c_input] == case["pairs"]
    dup = sv.copy()
    assert type(dup) is type(sv) and dup is not sv
    assert str(dup) == case["copy_str"] and dup.summary() == case["copy_summary"]
    assert not hasattr(dup, "_q")


@pytest.mark.parametrize("case", MANIFEST["raises"], ids=lambda c: c["name"])
def test_refusals(case):
    with pytest.raises(ValueError) as err:
        KINDS[case["kind"]](*case["args"], **case["kw"])
    assert str(err.value) == case["message"]


def test_surface_literal():
    assert str(PPV()) == "PPV(quantile=[0.5], constant=[False], sample_size=1.0, segments=False)"
    assert CPV([0, 2], True, segments=True).summary() == \
        "CPV [sampling=1.0, segments] -> 1:\n   > 0 | True\n   > 2 | True"
    assert PPV([0.2, 0.5, 0.9]).nfeatures() == 3
    assert PPV([-1, 0, 3], True, segments=True).nfeatures() == 2
    assert set(KINDS) <= set(fr.sieving.__dict__)
    assert nat.FR_SIEVE_PPV == 16 and nat.FR_SIEVE_CPV == 17


def test_transform_before_fit():
    # (even when every threshold is a constant)
    X = np.zeros((2, 5))
    with pytest.raises(RuntimeError, match=r"^Missing call of PPV\.fit\(\)$"):
        PPV(0, True).transform(X)
    with pytest.raises(RuntimeError, match=r"^Missing call of CPV\.fit\(\)$"):
        CPV([0.2, 3], [False, True]).transform(X)


# ---------------------------------------------------------------- restatement == reference
@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_restatement_matches_reference(case):
    X = ARRAYS[case["x"]]
    got = iref.transform(case["spec"]["kind"], X, ARRAYS[case["thresholds"]],
                         bool(case["spec"]["kw"].get("segments", False)))
    np.testing.assert_array_equal(got, ARRAYS[case["out"]])


def test_restatement_quirks():
    X = np.array([[1.0, 0.0, 1.0, np.nan, np.inf, -np.inf, 1.0, 1.0]])
    np.testing.assert_array_equal(iref.ppv(X, [1.0]), [[5 / 8]])          # NaN out, +inf in
    np.testing.assert_array_equal(iref.cpv(X, [1.0]), [[2 * 3 / 8]])      # the one at t = 0: no edge
    np.testing.assert_array_equal(iref.ppv(X, [1.0, np.inf], True), [[4 / 8]])   # [1, inf): +inf out
    np.testing.assert_array_equal(iref.ppv(X, [1.0, 0.0], True), [[0.0]])  # unsorted: empty
    np.testing.assert_array_equal(iref.cpv(np.array([[3.0]]), [1.0]), [[0.0]])   # T = 1
    np.testing.assert_array_equal(iref.cpv(np.array([[0.0, 3.0, 0.0]]), [1.0]), [[2 / 4]])  # odd T


# ---------------------------------------------------------------- the host fit
@pytest.mark.parametrize("case", MANIFEST["sieve"], ids=lambda c: c["name"])
def test_host_fit_draws_like_the_reference(case):
    """``fit`` on a host array is the reference's numpy procedure: the same thresholds, bit for
    bit, and numpy's global generator left where the reference leaves it."""
    sv = make_sieve(case["spec"])
    X = ARRAYS[case["x"]]
    np.random.seed(case["seed"])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (np.quantile of rows with NaN / inf)
        sv.fit(X)
    state = np.random.get_state()
    np.testing.assert_array_equal(np.asarray(sv._q, dtype=np.float64), ARRAYS[case["thresholds"]])
    assert int(state[2]) == case["pos_after_fit"]
    assert int(state[1][:4].sum()) == case["state_after_fit"]


# ---------------------------------------------------------------- the C entry's refusals
def test_entry_refusals():
    """Every argument check of fr_sieve_implicit runs before any HIP call (the style of
    test_host.py's table): the return code and the exact text of fr_last_error()."""
    L = nat.lib()
    i32, i64 = C.c_int32, C.c_int64
    p, q, null = C.c_void_p(0x1000), C.c_void_p(0x2000), None     # never dereferenced
    OK, ARG, LIMIT = 0, nat.FR_E_ARG, nat.FR_E_LIMIT

    def call(kind=nat.FR_SIEVE_PPV, N=3, T=8, dq=p, Q=2, segments=0, A=p, out=q):
        return L.fr_sieve_implicit(i32(kind), A, i64(N), i64(T), i64(T), dq, i32(Q), i32(segments),
                                   out, i64(Q), null)

    cases = [
        (lambda: call(kind=nat.FR_SIEVE_NPI), ARG, "fr_sieve_implicit: unknown kind"),
        (lambda: call(kind=nat.FR_SIEVE_CUR + 1), ARG, "fr_sieve_implicit: unknown kind"),
        (lambda: call(kind=18), ARG, "fr_sieve_implicit: unknown kind"),
        (lambda: call(kind=nat.FR_SIEVE_PPV | nat.FR_SIEVE_SERIES_CUTS), ARG, "fr_sieve_implicit: unknown kind"),
        (lambda: call(N=-1), ARG, "fr_sieve_implicit: bad shape"),
        (lambda: call(T=0), ARG, "fr_sieve_implicit: bad shape"),
        (lambda: call(N=1 << 31), ARG, "fr_sieve_implicit: bad shape"),
        (lambda: call(Q=0), ARG, "fr_sieve_implicit: bad quantiles"),
        (lambda: call(Q=1, segments=1), ARG, "fr_sieve_implicit: bad quantiles"),
        (lambda: call(dq=null), ARG, "fr_sieve_implicit: bad quantiles"),
        (lambda: call(Q=257), LIMIT, "fr_sieve_implicit: at most 256 features per sieve"),
        (lambda: call(Q=257, segments=1, N=0), OK, None),
        (lambda: call(N=0, A=null, out=null), OK, None),
        (lambda: call(kind=nat.FR_SIEVE_CPV, N=0), OK, None),
        (lambda: call(A=null), ARG, "fr_sieve_implicit: null device pointer"),
        (lambda: call(kind=nat.FR_SIEVE_CPV, out=null), ARG, "fr_sieve_implicit: null device pointer"),
        # fr_sieve itself knows neither kind
        (lambda: L.fr_sieve(i32(nat.FR_SIEVE_PPV), p, i64(3), i64(8), i64(8), i32(0), p, i64(1), i32(2),
                            p, i32(2), q, i64(1), null), ARG, "fr_sieve: unknown kind"),
    ]
    for i, (fn, code, text) in enumerate(cases):
        rc = fn()
        assert rc == code, (i, rc, nat.last_error())
        if text is not None:
            assert nat.last_error() == text, (i, nat.last_error())


# ---------------------------------------------------------------- which slices fuse
def _slice(sieves, semiring=None):
    fruit = fr.Fruit("s")
    fruit.add(fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED,
                     semiring=semiring or fr.semiring.Reals()))
    fruit.add(*sieves)
    return fruit.get_slice()


def test_fusable(monkeypatch):
    monkeypatch.delenv("FRUITS_AMD_FUSED", raising=False)
    assert _slice([PPV(0, True), CPV(0.5), NPI(), END()])._fusable()
    assert _slice([PPV([-1, 0, 3], True, segments=True)])._fusable()
    assert _slice([CPV()], fr.semiring.Arctic())._fusable()
    # no wrappers around them: the slice materialises
    assert not _slice([INC(PPV())])._fusable()
    assert not _slice([NPI(), INC(CPV(), depth=0)])._fusable()
    # the Arctic argmax kernel forms NPI / MPI / END only
    assert not _slice([PPV()], fr.semiring.Arctic(argmax=True))._fusable()
    assert not _slice([NPI(), CPV()], fr.semiring.Arctic(argmax=True))._fusable()
    monkeypatch.setenv("FRUITS_AMD_FUSED", "0")
    assert not _slice([PPV()])._fusable()
