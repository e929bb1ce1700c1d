"""CPU-only tests of generic words: letters, extended letters, Word, replace_letters, the cache
plan on their strings, the lowering to virtual rows, the restatement tests/words_ref.py against
the reference's recorded outputs, and the argument checks of fr_letter_rows / fr_rows_unshift."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import words_ref as wref
from conftest import GOLDEN_DIR, gen_input
import fruits_amd as fr
from fruits_amd import _native as nat
from fruits_amd.iss import lowering as low
from fruits_amd.iss.words import letters as letters_mod

ARR = np.load(os.path.join(GOLDEN_DIR, "golden_words.npz"))
with open(os.path.join(GOLDEN_DIR, "golden_words.json")) as f:
    MAN = json.load(f)

DIM, ABS, EXT, ONE = low.ROW_DIM, low.ROW_ABS, low.ROW_EXT, low.ROW_ONE


def x_of(case):
    spec = case["x_gen"]
    return gen_input(spec) + spec.get("offset", 0.0)


wref.register(fr)      # the custom letters of the golden cases
is_generic = wref.is_generic


def make_word(s: str):
    return fr.words.Word(s) if is_generic(s) else fr.words.SimpleWord(s)


# ---------------------------------------------------------------- letters and words
def test_extended_letter_surface():
    el = fr.words.ExtendedLetter("ABS(1)DIM(2)")
    assert str(el) == "[ABS(1)DIM(2)]" and len(el) == 2
    assert el.named() == [("ABS", 0), ("DIM", 1)]
    X = np.array([[-1.0, 2.0, -3.0], [4.0, -5.0, 6.0]])
    np.testing.assert_array_equal(el[0](X), [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(el[1](X), [4.0, -5.0, 6.0])
    assert [f(X).tolist() for f in el] == [[1.0, 2.0, 3.0], [4.0, -5.0, 6.0]]
    el.append("DIM", 0)
    assert str(el) == "[ABS(1)DIM(2)DIM(1)]" and len(el) == 3
    dup = el.copy()
    dup.append("ABS", 1)
    assert str(dup) == "[ABS(1)DIM(2)DIM(1)ABS(2)]" and str(el) == "[ABS(1)DIM(2)DIM(1)]"
    assert str(fr.words.ExtendedLetter()) == "[]" and len(fr.words.ExtendedLetter()) == 0
    with pytest.raises(RuntimeError, match="does not exist"):
        fr.words.ExtendedLetter("NOPE(1)")


def test_letter_decorator_and_registry():
    assert fr.words.letters.get_available()[:2] == ["DIM", "ABS"]
    assert fr.words.letters is letters_mod and fr.words.letter is letters_mod.letter

    @fr.words.letter
    def host_test_bare(X, i):
        return X[i, :] + 1.0

    @fr.words.letter(name="host_test_named")
    def whatever(X, i):
        return 2.0 * X[i, :]

    names = fr.words.letters.get_available()
    assert "host_test_bare" in names and "host_test_named" in names and "whatever" not in names
    X = np.arange(6.0).reshape(2, 3)
    np.testing.assert_array_equal(host_test_bare(1)(X), [4.0, 5.0, 6.0])
    np.testing.assert_array_equal(fr.words.ExtendedLetter("host_test_named(1)")[0](X), [0.0, 2.0, 4.0])
    with pytest.raises(RuntimeError, match="already exists"):
        fr.words.letter(name="host_test_named")(lambda X, i: X[i, :])
    with pytest.raises(RuntimeError, match="already exists"):
        fr.words.letter(name="DIM")(lambda X, i: X[i, :])
    with pytest.raises(RuntimeError, match="Too many arguments"):
        fr.words.letter(whatever, whatever)
    with pytest.raises(ValueError, match="specify the 'name' argument"):
        fr.words.letter()


def test_word_surface():
    s = "[ABS(1)DIM(2)][ABS(1)]"
    w = fr.words.Word(s)
    assert str(w) == s and len(w) == 2
    assert [str(el) for el in w] == ["[ABS(1)DIM(2)]", "[ABS(1)]"]
    w.multiply("[DIM(3)]")
    w.multiply(fr.words.ExtendedLetter("ReLU(1)"))
    w.multiply(fr.words.Word("[][ABS(2)]"))
    assert str(w) == s + "[DIM(3)][ReLU(1)][][ABS(2)]" and len(w) == 6
    dup = w.copy()
    assert str(dup) == str(w) and type(dup) is fr.words.Word
    dup.multiply("[DIM(1)]")
    assert len(w) == 6 and len(dup) == 7
    for bad in (3, None, ["[DIM(1)]"]):
        with pytest.raises(TypeError, match="Cannot multiply Word"):
            w.multiply(bad)
    # (a string without brackets names no letters: the reference's test_general.py relies on it)
    assert len(fr.words.Word("relu collection")) == 0 and len(fr.words.Word()) == 0
    assert (w == dup) is False and (w == w) is False
    np.testing.assert_array_equal(fr.words.Word("[DIM(1)][DIM(1)]").alpha, np.ones(2, np.float32))
    # SimpleWord keeps its behaviour
    sw = fr.words.SimpleWord("[11][122]")
    assert sw.table().tolist() == [[2, 0], [1, 2]] and str(sw.copy()) == "[11][122]"
    with pytest.raises(NotImplementedError):
        sw.multiply(fr.words.ExtendedLetter("DIM(1)"))


def test_replace_letters():
    word = fr.words.SimpleWord("[112][2]")
    out = fr.words.replace_letters(word, iter(["ABS", "ReLU"]))
    assert type(out) is fr.words.Word
    assert str(out) == "[ABS(1)ReLU(1)DIM(2)][DIM(2)]"      # the generator ran dry: DIM
    assert str(fr.words.replace_letters(word, ("DIM" for _ in range(1)))) == "[DIM(1)DIM(1)DIM(2)][DIM(2)]"
    assert str(fr.words.replace_letters(word, iter(["ABS"] * 9))) == "[ABS(1)ABS(1)ABS(2)][ABS(2)]"


# ---------------------------------------------------------------- cache plan, labels
@pytest.mark.parametrize("case", MAN["iss"], ids=lambda c: c["name"])
def test_cache_plan_and_labels(case):
    words = [make_word(s) for s in case["words"]]
    weighting = None
    if case["weighting"] is not None:
        kw = {k: v for k, v in case["weighting"].items() if k != "kind"}
        weighting = getattr(fr.iss.weighting, case["weighting"]["kind"])(**kw)
    iss = fr.ISS(words, mode=getattr(fr.ISSMode, case["mode"]),
                 semiring=getattr(fr.semiring, case["semiring"])(), weighting=weighting)
    assert iss.n_iterated_sums() == case["K"]
    assert [iss._depth(i) for i in range(len(words))] == case["depths"]
    assert [iss.label(i) for i in range(case["K"])] == case["labels"]
    assert wref.cache_plan(case["words"]) == case["depths"] or case["mode"] == "SINGLE"
    iss._check_supported()
    dup = iss._copy()
    assert [dup.label(i) for i in range(case["K"])] == case["labels"]


def test_generic_and_simple_strings_never_share_a_prefix():
    plan = fr.iss.CachePlan([fr.words.Word("[DIM(1)]"), fr.words.SimpleWord("[1][2]"),
                             fr.words.Word("[DIM(1)][DIM(2)]")])
    assert [plan.unique_el_depth(i) for i in range(3)] == [1, 2, 1]


def test_argmax_with_generic_words_is_refused():
    iss = fr.ISS([fr.words.Word("[DIM(1)][ABS(1)]")], mode=fr.ISSMode.EXTENDED,
                 semiring=fr.semiring.Arctic(argmax=True))
    with pytest.raises(NotImplementedError, match="slow path"):
        iss._check_supported()
    with pytest.raises(ValueError, match="simple words"):
        fr.CosWISS([fr.words.Word("[DIM(1)]")], freqs=[1.0])


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", [c for c in MAN["iss"] if all(is_generic(s) for s in c["words"])],
                         ids=lambda c: c["name"])
def test_words_ref_matches_the_reference(case):
    X = x_of(case)
    ref = ARR[case["out"]]
    got = wref.iss_transform(X, case["words"], case["mode"], case["semiring"])
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    for row, head in zip(ref, wref.head_lengths(case["words"], case["mode"], case["semiring"])):
        assert np.all(row[:, :head] == 0.0)


def test_words_ref_on_the_literal_cases():
    x1 = MAN["literal"]["x1"]
    got = wref.iss_transform(ARR[x1["x"]], ["[ReLU(1)][ReLU(2)]"])
    np.testing.assert_allclose(got[0], ARR[x1["out"]][0], rtol=1e-12)
    fs = MAN["literal"]["fast_slow"]
    strings = [s.replace("single_dim_letter", "DIM").replace("dim_letter", "DIM") for s in fs["strings"]]
    got = wref.iss_transform(gen_input(fs["x_gen"]), strings)
    np.testing.assert_allclose(got, ARR[fs["slow"]], rtol=1e-12)
    np.testing.assert_allclose(got, ARR[fs["fast"]], rtol=1e-9)


# ---------------------------------------------------------------- lowering
def test_lowering_reals_tables_and_rows():
    words = [fr.words.Word("[ABS(1)DIM(2)][ABS(1)]"), fr.words.Word("[DIM(2)DIM(2)][ReLU(1)ABS(1)]")]
    lw = low.lower(words, fr.semiring.Reals(), 3)
    # deduplicated, in order of first use; no shifts over Reals
    assert lw.rows == [(ABS, 0, 0), (DIM, 1, 0), (EXT, 0, 0)]
    assert [(n, d) for n, d, _ in lw.ext] == [("ReLU", 0)]
    assert lw.tables[0].tolist() == [[1, 1, 0], [1, 0, 0]]
    assert lw.tables[1].tolist() == [[0, 2, 0], [1, 0, 1]]
    assert all(t.dtype == np.int32 for t in lw.tables) and lw.spec.dtype == np.int32
    assert lw.out_shifts.tolist() == [0, 0] and not lw.shifted and not lw.one_is_zero
    assert low.lower(words, fr.semiring.Reals(), 3, [2, 1]).out_shifts.tolist() == [0, 0, 0]


def test_lowering_bayesian_shifts_by_position():
    """The generic slow path is strict, the max-times kernel is not: letter m reads its rows
    m steps ahead and the row of prefix p comes out p - 1 steps early."""
    words = [fr.words.Word("[ABS(1)DIM(2)][ABS(1)][ABS(1)]"), fr.words.Word("[ABS(1)DIM(2)][DIM(2)]")]
    lw = low.lower(words, fr.semiring.Bayesian(), 2, [3, 1])
    assert lw.rows == [(ABS, 0, 0), (DIM, 1, 0), (ABS, 0, 1), (ABS, 0, 2), (DIM, 1, 1)]
    assert lw.tables[0].tolist() == [[1, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0]]
    assert lw.tables[1].tolist() == [[1, 1, 0, 0, 0], [0, 0, 0, 0, 1]]   # the shared prefix: same columns
    assert lw.out_shifts.tolist() == [0, 1, 2, 1] and lw.shifted and not lw.one_is_zero


def test_lowering_arctic_does_not_shift():
    """Arctic's own slow path (fruits/iss/semiring.py:428-446) is the non-strict recursion."""
    words = [fr.words.Word("[ABS(1)DIM(2)][ABS(1)][ABS(1)]"), fr.words.Word("[ABS(1)DIM(2)][DIM(2)]")]
    lw = low.lower(words, fr.semiring.Arctic(), 2, [3, 1])
    assert lw.rows == [(ABS, 0, 0), (DIM, 1, 0)]
    assert lw.tables[0].tolist() == [[1, 1], [1, 0], [1, 0]] and lw.tables[1].tolist() == [[1, 1], [0, 1]]
    assert lw.out_shifts.tolist() == [0, 0, 0, 0] and not lw.shifted and lw.one_is_zero


def test_lowering_empty_extended_letter():
    w = fr.words.Word("[DIM(1)][][DIM(1)]")
    lw = low.lower([w], fr.semiring.Bayesian(), 1)
    assert lw.rows == [(DIM, 0, 0), (ONE, 0, 1), (DIM, 0, 2)]
    assert lw.tables[0].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    for semiring in (fr.semiring.Reals(), fr.semiring.Arctic()):
        lr = low.lower([w], semiring, 1)
        assert lr.rows == [(DIM, 0, 0), (ONE, 0, 0)] and lr.tables[0].tolist() == [[1, 0], [0, 1], [1, 0]]
        assert lr.one_is_zero == isinstance(semiring, fr.semiring.Arctic)


def test_lowering_mixed_list_and_simple_only():
    words = [fr.words.SimpleWord("[-12][22]"), fr.words.Word("[ABS(2)][DIM(2)]")]
    lw = low.lower(words, fr.semiring.Bayesian(), 2, [2, 2])
    assert lw.rows == [(DIM, 0, 0), (DIM, 1, 0), (ABS, 1, 0), (DIM, 1, 1)]
    assert lw.tables[0].tolist() == [[-1, 1, 0, 0], [0, 2, 0, 0]]      # signs kept, shift 0
    assert lw.tables[1].tolist() == [[0, 0, 1, 0], [0, 0, 0, 1]]
    assert lw.out_shifts.tolist() == [0, 0, 0, 1]
    assert low.lower([fr.words.SimpleWord("[1][2]")], fr.semiring.Arctic(), 2) is None
    with pytest.raises(IndexError, match="references dimension 3"):
        low.lower([fr.words.Word("[DIM(3)]")], fr.semiring.Reals(), 2)
    with pytest.raises(IndexError, match="references dimension 3"):
        low.lower([fr.words.SimpleWord("[3]"), fr.words.Word("[DIM(1)]")], fr.semiring.Reals(), 2)


def test_simple_word_lists_keep_their_plans():
    """No generic word: nothing is lowered - the plan's key and its tables are what they were."""
    iss = fr.ISS(fr.words.of_weight(2, dim=2), mode=fr.ISSMode.EXTENDED)
    assert not iss._has_generic and not iss.needs_unshift()
    plan = iss._plan(0, len(iss.words))
    (key,) = iss._plans.keys()
    assert key[0] == tuple(range(len(iss.words))) and "lowered" not in key
    assert plan.rows == iss.n_iterated_sums() and plan.max_dim == 2


def test_lowered_plan_compiles_and_is_cached_by_rows_and_dimensions():
    iss = fr.ISS([fr.words.Word("[ABS(1)DIM(2)][ABS(1)]"), fr.words.SimpleWord("[1][2]")],
                 mode=fr.ISSMode.EXTENDED, semiring=fr.semiring.Bayesian())
    assert iss.needs_unshift()
    lw, plan = iss._lowered((0, 1), 2)
    assert plan.rows == 4 and plan.max_dim == len(lw.rows) == 4 and plan.weighting == nat.FR_W_NONE
    assert iss._lowered((0, 1), 2)[1] is plan and iss._plan_indices((0, 1), D=2) is plan
    assert iss._lowered((0, 1), 2)[0] is lw      # lowered once per (words, D), kept with the plan
    assert iss._lowered((0, 1), 3)[1] is not plan
    with pytest.raises(ValueError, match="depends on the input's dimensions"):
        iss._plan_indices((0, 1))
    # a weighted ISS: generic and simple words run as separate plans
    wi = fr.ISS(iss.words + [fr.words.Word("[DIM(1)]")], weighting=fr.iss.weighting.Indices())
    assert wi._class_runs((0, 1, 2)) == [(0,), (1,), (2,)] and wi._class_runs((2, 0)) == [(2, 0)]
    assert wi._plan_indices((1,)).weighting != nat.FR_W_NONE
    assert wi._plan_indices((0, 2), D=2).weighting == nat.FR_W_NONE


def test_letter_values_are_validated():
    @fr.words.letter(name="host_test_short")
    def short(X, i):
        return X[i, :-1]

    lw = low.lower([fr.words.Word("[host_test_short(1)]")], fr.semiring.Reals(), 1)
    with pytest.raises(ValueError, match="one value per time step"):
        low.letter_values(lw, np.zeros((2, 1, 5)))
    lw = low.lower([fr.words.Word("[ReLU(2)][ReLU(2)SQ(1)]")], fr.semiring.Reals(), 2)
    Z = np.random.default_rng(0).standard_normal((3, 2, 7))
    vals = low.letter_values(lw, Z)
    np.testing.assert_array_equal(vals[:, 0], Z[:, 1] * (Z[:, 1] > 0))
    np.testing.assert_array_equal(vals[:, 1], Z[:, 0] * Z[:, 0])


# ---------------------------------------------------------------- the two entries' refusals
def test_letter_entries_refuse_bad_arguments():
    """Every argument check of fr_letter_rows / fr_rows_unshift runs before any HIP call: the
    return code and the exact text of fr_last_error()."""
    L = nat.lib()
    i32, i64 = C.c_int32, C.c_int64
    p, q, null = C.c_void_p(0x10000), C.c_void_p(0x80000), None    # never dereferenced
    OK, ARG, DIMC = 0, nat.FR_E_ARG, nat.FR_E_DIM

    def ints(*v):
        return (i32 * len(v))(*v)

    def rows(N=2, D=3, T=8, ext=null, H=0, d_spec=p, h_spec=ints(0, 0, 0, 1, 2, 1), Dv=2, X=p, out=q):
        return L.fr_letter_rows(X, i64(N), i64(D), i64(T), ext, i64(H), d_spec, h_spec, i32(Dv),
                                i32(0), out, null)

    def unshift(K=2, N=3, T=8, d_shift=p, h_shift=ints(0, 1), A=p, out=q):
        return L.fr_rows_unshift(A, i64(K), i64(N), i64(T), d_shift, h_shift, out, null)

    near = C.c_void_p(0x10000 + 8 * 10)      # inside the 2 x 3 x 8 doubles at p
    cases = [
        (lambda: rows(T=0), ARG, "fr_letter_rows: bad shape"),
        (lambda: rows(D=0), ARG, "fr_letter_rows: bad shape"),
        (lambda: rows(N=-1), ARG, "fr_letter_rows: bad shape"),
        (lambda: rows(Dv=0), ARG, "fr_letter_rows: bad shape"),
        (lambda: rows(H=-1), ARG, "fr_letter_rows: bad shape"),
        (lambda: rows(h_spec=null), ARG, "fr_letter_rows: null host table"),
        (lambda: rows(h_spec=ints(0, 0, 0, 4, 0, 0)), ARG, "fr_letter_rows: row 1 has an unknown kind"),
        (lambda: rows(h_spec=ints(-1, 0, 0, 0, 0, 0)), ARG, "fr_letter_rows: row 0 has an unknown kind"),
        (lambda: rows(h_spec=ints(0, 0, 0, 1, 0, -1)), ARG, "fr_letter_rows: row 1 has a negative shift"),
        (lambda: rows(h_spec=ints(0, 3, 0, 1, 0, 0)), DIMC, "fr_letter_rows: row 0 names source 3 of 3"),
        (lambda: rows(h_spec=ints(0, 0, 0, 1, -1, 0)), DIMC, "fr_letter_rows: row 1 names source -1 of 3"),
        (lambda: rows(h_spec=ints(2, 0, 0, 0, 0, 0)), ARG,
         "fr_letter_rows: row 0 reads letter values but there are none"),
        (lambda: rows(h_spec=ints(2, 0, 0, 0, 0, 0), ext=p, H=0), ARG,
         "fr_letter_rows: row 0 reads letter values but there are none"),
        (lambda: rows(h_spec=ints(2, 2, 0, 0, 0, 0), ext=C.c_void_p(0x40000), H=2), DIMC,
         "fr_letter_rows: row 0 names source 2 of 2"),
        (lambda: rows(N=0), OK, None),
        (lambda: rows(h_spec=ints(3, 99, 5, 0, 0, 99), N=0), OK, None),   # ONE ignores its source
        (lambda: rows(X=null), ARG, "fr_letter_rows: null or aliased device pointer"),
        (lambda: rows(out=null), ARG, "fr_letter_rows: null or aliased device pointer"),
        (lambda: rows(d_spec=null), ARG, "fr_letter_rows: null or aliased device pointer"),
        (lambda: rows(out=p), ARG, "fr_letter_rows: null or aliased device pointer"),
        (lambda: rows(out=near), ARG, "fr_letter_rows: null or aliased device pointer"),
        (lambda: rows(h_spec=ints(2, 0, 0, 0, 0, 0), ext=q, H=1), ARG,
         "fr_letter_rows: null or aliased device pointer"),
        (lambda: unshift(T=0), ARG, "fr_rows_unshift: bad shape"),
        (lambda: unshift(K=-1), ARG, "fr_rows_unshift: bad shape"),
        (lambda: unshift(N=-1), ARG, "fr_rows_unshift: bad shape"),
        (lambda: unshift(h_shift=null), ARG, "fr_rows_unshift: null host table"),
        (lambda: unshift(h_shift=ints(0, -2)), ARG, "fr_rows_unshift: row 1 has a negative shift"),
        (lambda: unshift(K=0, h_shift=null), OK, None),
        (lambda: unshift(N=0), OK, None),
        (lambda: unshift(A=null), ARG, "fr_rows_unshift: null or aliased device pointer"),
        (lambda: unshift(out=null), ARG, "fr_rows_unshift: null or aliased device pointer"),
        (lambda: unshift(d_shift=null), ARG, "fr_rows_unshift: null or aliased device pointer"),
        (lambda: unshift(out=p), ARG, "fr_rows_unshift: null or aliased device pointer"),
        (lambda: unshift(out=near), ARG, "fr_rows_unshift: null or aliased device pointer"),
    ]
    for i, (call, code, text) in enumerate(cases):
        rc = call()
        assert rc == code, (i, rc, nat.last_error())
        if text is not None:
            assert nat.last_error() == text, (i, nat.last_error())
    assert L.fr_version() >= 136
