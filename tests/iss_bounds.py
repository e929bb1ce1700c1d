"""A derived, elementwise rounding bound for the Reals iterated sums and for CosWISS.

A Reals iterated sum - and every term of a CosWISS row - is a sum of products of input values
with positive ``exp`` weights or with ``sin`` / ``cos`` table entries.  Call that computation R
and let A be the same computation with every factor replaced by its magnitude
(``magnitude=True`` of oracle/ref_numpy.py).  Whatever the order of the additions - the
reference's sequential ``cumsum``, a parallel scan with chunk carries, a factorised CosWISS -

    |fl(R) - R|[k, n, t]  <=  c * n_ops * u * A[k, n, t],        u = 2^-53,  c = 2

where ``n_ops`` counts the roundings on the longest path of one term (``n_ops`` /
``n_ops_coswiss`` below carry the count and its derivation).  c = 2 covers gamma_n =
n u / (1 - n u) against n u and the 2^-64 of the extended-precision side the result is compared
with.  No measured number enters: R and A come from ``dtype=np.longdouble`` runs of the oracle
on the inputs (and, for a weighted plan, on the lookup) the code under test was given.

A fused launch leaves features, not rows: ``probe_positions`` says where to read the rows
through ``END``, ``feature_reference`` carries the elementwise bound over to the features the
fused epilogue forms (``MAX`` / ``MIN`` selections, ``MPI`` band means of the rows and of their
first increments), ``check_features`` asserts it (tests/test_fused_bounds_gpu.py).

Not a conftest: the modules that need it import it by name.  The largest ``err / bound`` of
every family that went through ``check_bound`` / ``check_features`` is kept in ``RATIOS``; ``print_ratios`` (called
by a module fixture's teardown) prints them as ``ISS-RATIO family: ...`` and clears them.
"""
import math

import numpy as np

from oracle import ref_numpy as orc

U = 2.0 ** -53
C = 2.0
HP = np.longdouble
RATIOS = {}

# the words of the CPU check the bound was validated with (unweighted, Indices and L1, total and
# non-total; dimensions 1 ... 3): every family adds its own set
WORDS = ["[1][2][3]", "[11][2]", "[1][-2]", "[12][2][33][1]"]


def _prefix_counts(rows, depth):
    """(L, W) of the last ``depth`` prefixes of a parsed word, shortest first: the order of
    the rows iss_transform returns for it."""
    out = []
    for length in range(len(rows) - depth + 1, len(rows) + 1):
        out.append((length, sum(abs(e) for letter in rows[:length] for e in letter)))
    return out


def n_ops(word_strings, T, mode="EXTENDED", alphas=None, lookup=None):
    """Roundings on the longest path of one term of a Reals iterated sum, one count per output
    row of ``orc.iss_transform(X, word_strings, mode, ...)`` (an int64 array (K,)), from
    oracle/ref_numpy.py iterated_sum_fast.  A row is the iterated sum of a prefix of a word;
    with L letters and W elementary letters (the sum of the |exponents|) in that prefix and
    series of T elements a term passes through

    * every one of the L cumulative sums: at most T-1 additions each, sequentially (cumsum),
      fewer in a scan tree                                                    L (T-1)
    * one multiplication or division per elementary letter (_letters)         W

    and, with a weighting (alpha, lookup g) - both bodies, total or not, per letter:

    * a multiplication by exp(+g alpha_k) in front of the cumulative sum and one by
      exp(-g alpha_k) behind it (total: on the way out / to the next letter; non-total: at
      the next letter, none behind the last)                                  2 L
    * those two exp factors themselves: the argument g * alpha is a rounded product, which
      moves exp by a relative |g alpha| u <= ceil(alpha_max g_max) u, and exp is taken to
      1 ulp <= 2 u                                         2 L (2 + ceil(alpha_max g_max))

        n_ops = L (T-1) + W + 2 L (3 + ceil(alpha_max g_max))      weighted
        n_ops = L (T-1) + W                                        unweighted

    Without a weighting alpha and g are zero and exp(0) = 1 is exact: those factors round
    nothing.  The count is taken at the full length T for every t (a shorter prefix of the
    series has a shorter path: the bound is only looser there); alpha_max and g_max are the
    largest of the whole call.
    """
    plan = orc.cache_plan(word_strings) if mode == "EXTENDED" else [1] * len(word_strings)
    extra = 0
    if lookup is not None:
        a_max = 1.0
        if alphas is not None:
            a_max = max([1.0 if a is None else float(np.max(np.abs(a))) for a in alphas])
        g_max = float(np.max(np.abs(lookup))) if np.size(lookup) else 0.0
        extra = 2 * (3 + math.ceil(a_max * g_max))
    out = []
    for s, depth in zip(word_strings, plan):
        for L, W in _prefix_counts(orc.parse_word(s), depth):
            out.append(L * max(T - 1, 0) + W + L * extra)
    return np.array(out, dtype=np.int64)


def n_ops_coswiss(word_strings, n_freqs, T, exponent, total):
    """The counts for the rows of ``orc.coswiss_transform`` ((W*F,), word-major), from its code:
    the L (T-1) additions and W letter operations of ``n_ops``; per letter - and once more behind
    the last letter with total weighting, p = L + 1 "letters" then, else p = L - up to 2 S table
    multiplications (the sin and cos powers of a term add up to at most 2 S at a letter)
    2 S p; and the sum over the (S+1)^(p-1) expanded terms with their integer coefficients
    (S+1)^(p-1) + 1:

        n_ops = L (T-1) + W + 2 S p + (S+1)^(p-1) + 1

    (The factorised form of the sum adds S+1 terms per letter instead, (S+1)(p-1) <=
    (S+1)^(p-1).)  The table entries' own error is what the padded magnitude tables answer
    for (orc.coswiss_trig)."""
    out = []
    for s in word_strings:
        rows = orc.parse_word(s)
        (L, W), = _prefix_counts(rows, 1)
        p = L + 1 if total else L
        n = L * max(T - 1, 0) + W + 2 * exponent * p + (exponent + 1) ** (p - 1) + 1
        out += [n] * n_freqs
    return np.array(out, dtype=np.int64)


def bound(n, A):
    """c * n_ops * u * A in extended precision; ``n`` a number or one count per row (K,) of
    A (K, N, T)."""
    n = np.asarray(n, dtype=HP)
    if n.ndim == 1:
        n = n[:, None, None]
    return HP(C * U) * n * np.asarray(A, dtype=HP)


def reals_reference(X, word_strings, mode="EXTENDED", alphas=None, lookup=None, total=False):
    """(hp, A, n): the long-double oracle, its magnitude run and the operation count of a Reals
    ISS over ``X`` (K, N, T).  ``lookup`` is the lookup the code under test used ((1|N, T))."""
    X = np.asarray(X, dtype=np.float64)
    if lookup is not None:
        lookup = np.broadcast_to(np.asarray(lookup, dtype=np.float64), (X.shape[0], X.shape[2]))
    hp = orc.iss_transform(X, word_strings, mode, alphas, lookup, total, dtype=HP)
    # (|X| == X: the magnitude run would repeat the very same operations)
    A = hp if (X >= 0).all() else orc.iss_transform(X, word_strings, mode, alphas, lookup, total,
                                                    dtype=HP, magnitude=True)
    return hp, A, n_ops(word_strings, X.shape[2], mode, alphas, lookup)


def coswiss_reference(X, word_strings, freqs, exponent, total):
    """(hp, A, n) of a CosWISS transform (W*F, N, T)."""
    X = np.asarray(X, dtype=np.float64)
    hp = orc.coswiss_transform(X, word_strings, freqs, exponent, total, dtype=HP)
    A = orc.coswiss_transform(X, word_strings, freqs, exponent, total, dtype=HP, magnitude=True)
    return hp, A, n_ops_coswiss(word_strings, len(freqs), X.shape[2], exponent, total)


def series_subset(N, most=96, whole=0):
    """At most ``most`` series of a batch of N: the first ``whole`` of them - one complete slab
    of a test that runs its batch in slabs of ``whole`` series - and the others spread evenly
    over the rest, the last series among them.  The long-double oracle costs a hundred times
    the float64 one, so a large batch is held to the bound on these series ONLY: the others
    keep the bar the calling test had before."""
    if N <= most:
        return np.arange(N)
    rest = most - whole
    return np.unique(np.r_[np.arange(whole), np.arange(whole, N, -(-(N - whole) // (rest - 1))), N - 1])


def check_reals(got, X, word_strings, mode="EXTENDED", alphas=None, lookup=None, total=False,
                what="", family=None, most=96, whole=0):
    """``check_bound`` of a Reals result ``got`` (K, N, T) over ``series_subset(N, most, whole)``."""
    idx = series_subset(X.shape[0], most, whole)
    if lookup is not None and lookup.shape[0] != 1:
        lookup = lookup[idx]
    hp, A, n = reals_reference(X[idx], word_strings, mode, alphas, lookup, total)
    return check_bound(np.asarray(got)[:, idx], hp, A, n, what, family)


def check_coswiss(got, X, word_strings, freqs, exponent, total, what="", family=None, most=96,
                  whole=0):
    idx = series_subset(X.shape[0], most, whole)
    hp, A, n = coswiss_reference(X[idx], word_strings, freqs, exponent, total)
    return check_bound(np.asarray(got)[:, idx], hp, A, n, what, family)


def ratio(got, hp, A, n):
    """Elementwise |got - hp| / bound (0 where both vanish; inf where A == 0 and got != hp)."""
    err = np.abs(np.asarray(got).astype(HP) - hp)
    b = bound(n, A)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0.0))
    return r.astype(np.float64)


def check_bound(got, hp, A, n, what, family=None):
    """Asserts elementwise ``|got - hp| <= c n u A``; where ``A == 0`` (the leading t < L-1
    zeros of a word of L letters) ``got`` must be exactly ``hp``.  Records the largest
    ``err / bound`` under ``family``; returns it."""
    got = np.asarray(got)
    assert got.shape == hp.shape == A.shape, (what, got.shape, hp.shape, A.shape)
    assert np.isfinite(got).all(), what
    zero = A == 0
    assert np.array_equal(got[zero], hp[zero].astype(np.float64)), (what, "A == 0 but got != hp")
    r = ratio(got, hp, A, n)
    worst = float(r.max()) if r.size else 0.0
    if family is not None:
        RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    if not worst <= 1.0:
        at = np.unravel_index(int(np.argmax(r)), r.shape)
        row_ops = int(n[at[0]]) if np.ndim(n) else int(n)
        raise AssertionError(
            f"{what}: |got - hp| exceeds c*n_ops*u*A (n_ops = {row_ops}) by a factor {worst:.3g} at "
            f"(k, n, t) = {tuple(int(i) for i in at)}: got {got[at]!r}, hp {float(hp[at])!r}, "
            f"A {float(A[at])!r}; {int((r > 1).sum())} of {r.size} entries outside")
    return worst


def violates(got, hp, A, n):
    """Whether ``got`` lies outside the bound somewhere (the sensitivity checks)."""
    return bool((ratio(got, hp, A, n) > 1.0).any())


# ------------------------------------------------------------------ features of a fused launch
# A fused launch never writes the rows: what it leaves are features.  The bounds below carry the
# elementwise bound b = bound(n, A) of the rows over to the features the fused epilogue forms.
_PROBES = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 127, 128, 129, 255, 256, 257, 383, 384, 511, 512, 513,
           767, 768, 1023, 1024, 1025, 2047, 2048, 2049)
FEATURE_KINDS = ("END", "MAX", "MIN", "MPI0", "MPI1")


def probe_positions(T):
    """The sorted 0-based positions in [0, T) where the parts of a scan meet: the lane boundaries
    for 2 and 4 elements per lane (1 ... 8), the wave boundaries of both chunk sizes (a wave of 64
    lanes: 128 / 256 elements; 63, 64), the piece boundaries of the wave-per-series kernel (128,
    256, 384), the chunk boundaries (512 / 1024 and their multiples up to 2048), each with its
    neighbours, and T // 3, T // 2 and the two last elements of the series.  An ``END`` sieve reads
    position p with the cut p + 1."""
    return sorted({p for p in _PROBES + (T // 3, T // 2, T - 2, T - 1) if 0 <= p < T})


def segments(T, cut):
    """[(lo, hi)] - the element sets [lo, hi) of a segment sieve with the integer cuts ``cut`` on
    series of T elements (oracle/ref_numpy.py transformed_cuts: sorted, a leading 0)."""
    c = orc.transformed_cuts(1, T, list(cut) if isinstance(cut, (list, tuple)) else cut)[0]
    return [(int(c[j]), int(c[j + 1])) for j in range(len(c) - 1)]


def open_band(A):
    """The finite threshold pair (-2 max A, +2 max A) of a band that takes every element: every
    |value| and every |increment| <= 2 max|row| lies strictly inside, none near a threshold
    (any row within the bound of hp has |row| <= (1 + c n u) A)."""
    w = 2.0 * float(np.max(A)) if np.size(A) else 1.0
    return np.array([-w, w]) if w > 0 else np.array([-1.0, 1.0])


def feature_reference(kind, hp, A, n, cut):
    """(ref, bnd): what a feature of the rows is compared with and the bound on the difference, both
    (K, N, C) in extended precision, one column per segment of ``cut``; from (hp, A, n) of
    ``reals_reference`` / ``coswiss_reference``.  Write b = bound(n, A) (elementwise: |row - hp|
    <= b), S = [lo, hi) for the elements of a segment, m = |S|.  An empty segment gives 0 on every
    side (oracle/ref_numpy.py band_value): ref 0, bound 0.  The bands are open (``open_band``):
    every element of S takes part, on the device as in the reference.

    ``END``   the row at hi - 1: ref hp[hi-1], bound b[hi-1] - the element itself.
    ``MAX`` / ``MIN``   ref max / min of hp over S.  With |row_t - hp_t| <= b_t for every t in S,
              max row <= max (hp_t + b_t) <= max hp + max b and max row >= row at hp's argmax
              >= max hp - max b (MIN alike): bound max_{t in S} b_t.  A selection rounds nothing.
    ``MPI0``  the mean of the row over S: ref mean hp_t.  The device sums m rounded elements in
              some order - m - 1 additions, each of relative u on a partial sum of magnitude <=
              sum |row_t| - and divides once: m roundings on sum |row_t| / m <= (1 + c n u) mean
              A_t; plus the elements' own error, mean b_t:
                  bound = mean b_t + c m u mean A_t
              (c = 2 takes gamma_m against m u and the factor 1 + c n u, as in ``bound``).
    ``MPI1``  the mean over S of the zero-padded first increments d_t = row_t - row_(t-1), d_0 = 0:
              ref the mean of hp's.  The device takes d_t as the difference of two emitted values
              - error b_t + b_(t-1), and one rounding of the subtraction, u |d_t| <= u (A_t +
              A_(t-1)) - or as the summand of the row's last cumulative sum before it is added:
              that summand's term paths are those of row_t without the additions of that sum, so
              its error is below b_t.  Either way |d_t - d_t(hp)| <= b_t + b_(t-1) + u (A_t +
              A_(t-1)), and the mean adds m roundings on mean |d_t| <= mean (A_t + A_(t-1)):
                  bound = mean (b_t + b_(t-1)) + c (m + 1) u mean (A_t + A_(t-1))
              The padded d_0 is the constant 0 on both sides: its terms are b = A = 0.
    """
    hp = np.asarray(hp, dtype=HP)
    A = np.asarray(A, dtype=HP)
    b = bound(n, A)
    if kind == "MPI1":
        d, bd, Ad = np.zeros_like(hp), np.zeros_like(hp), np.zeros_like(hp)
        d[..., 1:] = hp[..., 1:] - hp[..., :-1]
        bd[..., 1:] = b[..., 1:] + b[..., :-1]
        Ad[..., 1:] = A[..., 1:] + A[..., :-1]
    segs = segments(hp.shape[-1], cut)
    ref = np.zeros(hp.shape[:-1] + (len(segs),), dtype=HP)
    bnd = np.zeros_like(ref)
    for j, (lo, hi) in enumerate(segs):
        m = hi - lo
        if m <= 0:
            continue
        if kind == "END":
            ref[..., j], bnd[..., j] = hp[..., hi - 1], b[..., hi - 1]
        elif kind in ("MAX", "MIN"):
            ref[..., j] = (np.max if kind == "MAX" else np.min)(hp[..., lo:hi], axis=-1)
            bnd[..., j] = np.max(b[..., lo:hi], axis=-1)
        elif kind == "MPI0":
            ref[..., j] = np.mean(hp[..., lo:hi], axis=-1)
            bnd[..., j] = np.mean(b[..., lo:hi], axis=-1) + HP(C * m * U) * np.mean(A[..., lo:hi], axis=-1)
        elif kind == "MPI1":
            ref[..., j] = np.mean(d[..., lo:hi], axis=-1)
            bnd[..., j] = (np.mean(bd[..., lo:hi], axis=-1)
                           + HP(C * (m + 1) * U) * np.mean(Ad[..., lo:hi], axis=-1))
        else:
            raise ValueError("no feature bound for %r" % (kind,))
    return ref, bnd


def oracle_features(kind, rows, cut, band):
    """The float64 numpy oracle's features ((K, N, C)) of float64 rows (K, N, T): its sieve
    backends with the thresholds ``band`` (the sensitivity and CPU checks; ``END`` takes none)."""
    rows = np.asarray(rows, dtype=np.float64)
    K, N, T = rows.shape
    cuts = orc.transformed_cuts(N, T, list(cut) if isinstance(cut, (list, tuple)) else cut)
    out = []
    for k in range(K):
        if kind == "END":
            out.append(orc.end_transform(rows[k], cuts))
        elif kind in ("MAX", "MIN"):
            out.append(orc.BACKENDS[kind](rows[k], cuts, band))
        else:
            out.append(orc.mpi_backend(orc.pre_transform(rows[k], int(kind[3:])), cuts, band))
    return np.stack(out)


def feature_ratio(got, ref, bnd):
    """Elementwise |got - ref| / bnd (0 where both vanish; inf where bnd == 0 and got != ref)."""
    err = np.abs(np.asarray(got).astype(HP) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), np.where(err > 0, np.inf, 0.0))
    return r.astype(np.float64)


def check_features(got, ref, bnd, what, family=None):
    """``check_bound`` for features: asserts elementwise ``|got - ref| <= bnd`` with (ref, bnd) of
    ``feature_reference``; where the bound is 0 (an empty segment, the leading zeros of a row) the
    values must be equal.  Records the largest ``err / bound`` under ``family``; returns it."""
    got = np.asarray(got)
    assert got.shape == ref.shape == bnd.shape, (what, got.shape, ref.shape, bnd.shape)
    assert np.isfinite(got).all(), what
    zero = bnd == 0
    assert np.array_equal(got[zero], ref[zero].astype(np.float64)), (what, "bound == 0 but got != ref")
    r = feature_ratio(got, ref, bnd)
    worst = float(r.max()) if r.size else 0.0
    if family is not None:
        RATIOS[family] = max(RATIOS.get(family, 0.0), worst)
    if not worst <= 1.0:
        at = np.unravel_index(int(np.argmax(r)), r.shape)
        raise AssertionError(
            f"{what}: |got - ref| exceeds the derived bound by a factor {worst:.3g} at "
            f"(k, n, column) = {tuple(int(i) for i in at)}: got {got[at]!r}, ref {float(ref[at])!r}, "
            f"bound {float(bnd[at])!r}; {int((r > 1).sum())} of {r.size} entries outside")
    return worst


def positive_precondition(hp, A):
    """The precondition of a sensitivity case: the magnitude run is no more than 10 x the value,
    row by row (``rowmax(A) <= 10 rowmax|hp|``) - a relative perturbation of the result is then
    one of A as well.  Returns the largest ratio."""
    a = A.reshape(-1, A.shape[-1]).max(axis=1)
    h = np.abs(hp).reshape(-1, hp.shape[-1]).max(axis=1)
    assert np.all(a <= 10 * h), float(np.max(a / np.where(h > 0, h, 1)))
    return float(np.max(a / np.where(h > 0, h, 1))) if a.size else 0.0


def print_ratios():
    """Prints the families recorded since the last call and forgets them: every test module's
    fixture calls this at its end, each family is recorded by one module."""
    for k, v in sorted(RATIOS.items()):
        print(f"ISS-RATIO {k}: largest |gpu - hp| / (c n_ops u A) = {v:.3g}")
    RATIOS.clear()


# ------------------------------------------------------------------ the cases of the GPU tests
# (tests/test_iss_bounds_gpu.py runs them on the device; tests/test_iss_bounds_host.py holds the
# float64 oracles to the same bound on the same inputs)
LENGTHS = (1, 2, 63, 300, 1024, 1025, 3000)      # the packed limit, one chunk, a multi-chunk carry
WEIGHTINGS = {
    "none": None,
    "indices": {"kind": "Indices", "scale": 2.0},
    "indices_total": {"kind": "Indices", "scale": 2.0, "total": True},
    "l1": {"kind": "L1", "scale": 3.0},
    "l1_total": {"kind": "L1", "scale": 3.0, "total": True},
}
_W12 = ["[1]", "[2]", "[11]", "[12]", "[22]", "[1][1]", "[1][2]", "[2][1]", "[2][2]"]
# a word set of more than 32 nodes in two dimensions (the lean walk's plans): of_weight(<= 3, 2)
_W32 = orc.of_weight_strings(1, 2) + orc.of_weight_strings(2, 2) + orc.of_weight_strings(3, 2)
FAMILY_WORDS = {
    "interpreter": (3, WORDS + ["[2][3]", "[3][-1][2]"]),
    "lean": (2, _W32 + ["[11][2]", "[1][-2]", "[12][2][11][1]"]),
    "packed": (3, WORDS + ["[3][1]", "[2][-3]"]),
    "static_aot": (3, orc.of_weight_strings(2, 3)),        # of_weight(2, 3): 18 rows EXTENDED
    # (the static scheduler takes positive exponents only: the CPU check's words but "[1][-2]")
    "static_jit": (3, [w for w in WORDS if "-" not in w] + ["[2][3][1]", "[33]"]),
}
COS_LENGTHS = (50, 100, 450, 1030, 2051)
COS_EXPONENTS = (1, 2, 4, 6)
COS_WORDS = ["[1]", "[2][1]", "[1][2][2]", "[12][1][-2][1]"]      # test_coswiss_long_series'
COS_FREQS = [0.15, 0.5]


def coswiss_words(T, exponent):
    """The words of a CosWISS case: test_coswiss_long_series' (two of them beyond T = 2000, as
    there); from exponent 4 on without the four-letter word - the oracle evaluates the
    (S+1)^L expanded terms one by one."""
    return COS_WORDS[:2] if T > 2000 else (COS_WORDS if exponent <= 2 else COS_WORDS[:3])


def reals_input(dist, N, D, T, seed=0):
    """``normal``: zero-mean N(0, 1); ``uniform``: the positive case, U[0, 1)."""
    rng = np.random.default_rng([seed, N, D, T, 0 if dist == "normal" else 1])
    return rng.standard_normal((N, D, T)) if dist == "normal" else rng.random((N, D, T))


def coswiss_input(dist, N, T):
    """``positive``: the input of test_coswiss_vs_oracle (U[0, 1) + 0.25); ``zero_mean``: that of
    test_coswiss_long_series (N(0, 1/T), the second dimension positive: it is divided by)."""
    rng = np.random.default_rng([T, N, 0 if dist == "positive" else 1])
    if dist == "positive":
        return rng.random((N, 2, T)) + 0.25
    X = rng.standard_normal((N, 2, T)) / np.sqrt(T)
    X[:, 1] = np.abs(X[:, 1]) + 0.5
    return X
