"""References for the backward pass of the cosine weighted iterated sums (fruits_amd.nn.cos_iss,
DESIGN.md 4.14.7).

Not a conftest: the modules that need it import it by name.

The scalar that is differentiated is ``sum over n, k, t of G[n, k, t] * Y[n, k, t]`` with ``Y`` the
rows of ``CosWISS.transform`` - word-major, ``F`` rows per word - and ``G`` in the layout of
``fruits_amd.nn.cos_iss``'s result, (N, W * F, T).  The sin / cos tables are constants.

* ``grad_cos_bruteforce``: the gradient straight from the definition - every index tuple, every
  term of the expansion of the cosine powers - in exact rational arithmetic; tiny cases only.
* ``coswiss_forward`` / ``coswiss_grad``: the factorised recursion and its adjoint, sequential, in
  ``np.longdouble``.
* ``n_ops_cos`` / ``n_ops_grad_cos``: the roundings on the longest path of one term.
"""
import math
from fractions import Fraction
from itertools import combinations, product

import numpy as np

from iss_grad_ref import HP, _ipow, _letter, _shift, _suffix, orc


def word_letters(word_strings):
    """Per word its letters, a letter a tuple of exponents."""
    return [[tuple(row) for row in orc.parse_word(s)] for s in word_strings]


def binomials(S):
    return [math.comb(S, m) for m in range(S + 1)]


def trig_tables(T, freqs, dtype=HP):
    """(F, T) sin and cos of the angle pi t / (f (T - 1)) in ``dtype``, the frequency rounded to
    float32 first (oracle.ref_numpy.coswiss_trig).  T = 1: 0 / 0, NaN as in the reference."""
    with np.errstate(all="ignore"):
        pairs = [orc.coswiss_trig(T, f, dtype) for f in freqs]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# ------------------------------------------------------------------ the definition, exactly
def grad_cos_bruteforce(X, G, word_strings, tables, S, total):
    """d/dX of ``sum G * Y`` from the definition

        Y_(w,f)[t] = sum over i_1 < ... < i_p <= t of prod_k z_k[i_k]
                     * prod_(k < p) c(i_k, i_(k+1))^S  [* c(i_p, t)^S with total weighting]
        c(a, b)^S = sum_m C(S, m) (sin_a sin_b)^(S-m) (cos_a cos_b)^m

    with ``tables = (sin, cos)``, (F, T) arrays whose values are taken as given exact rationals:
    every index tuple and every combination of expansion terms is visited and the product rule
    applied to it, in ``fractions.Fraction``.  For ``T <= 5``, up to 3 letters and ``S <= 3``.
    Returns an (N, D, T) object array of Fractions."""
    X = np.asarray(X, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    N, D, T = X.shape
    words = word_letters(word_strings)
    sin_t, cos_t = (np.asarray(t, dtype=np.float64) for t in tables)
    F = sin_t.shape[0]
    assert T <= 5 and S <= 3 and all(len(w) <= 3 for w in words), "grad_cos_bruteforce is for tiny cases"
    assert G.shape == (N, len(words) * F, T)
    b = binomials(S)
    out = np.empty((N, D, T), dtype=object)
    for n in range(N):
        x = [[Fraction(float(X[n, d, t])) for t in range(T)] for d in range(D)]
        dx = [[Fraction(0)] * T for _ in range(D)]

        def letter(el, t, skip=-1):
            v = Fraction(1)
            for d, e in enumerate(el):
                if e != 0 and d != skip:
                    v *= x[d][t] ** e
            return v

        for w, letters in enumerate(words):
            p = len(letters)
            links = p - 1 + (1 if total else 0)
            for f in range(F):
                sn = [Fraction(float(v)) for v in sin_t[f]]
                cs = [Fraction(float(v)) for v in cos_t[f]]
                q = [[sn[t] ** (S - m) * cs[t] ** m for t in range(T)] for m in range(S + 1)]
                for t in range(T):
                    g = Fraction(float(G[n, w * F + f, t]))
                    if g == 0:
                        continue
                    for idx in combinations(range(t + 1), p):
                        ends = list(idx) + [t]
                        weight = Fraction(0)
                        for ms in product(range(S + 1), repeat=links):
                            term = Fraction(1)
                            for j, m in enumerate(ms):
                                term *= b[m] * q[m][ends[j]] * q[m][ends[j + 1]]
                            weight += term
                        zs = [letter(letters[j], idx[j]) for j in range(p)]
                        for j in range(p):
                            rest = Fraction(1)
                            for i in range(p):
                                if i != j:
                                    rest *= zs[i]
                            for d, e in enumerate(letters[j]):
                                if e == 0:
                                    continue
                                dz = e * x[d][idx[j]] ** (e - 1) * letter(letters[j], idx[j], skip=d)
                                dx[d][idx[j]] += g * weight * dz * rest
        for d in range(D):
            for t in range(T):
                out[n, d, t] = dx[d][t]
    return out


# ------------------------------------------------------------------ the recursion and its adjoint
def _prepare(X, word_strings, freqs, S, magnitude, tables, dtype):
    if np.dtype(dtype).type is not np.float64:
        orc.require_extended_precision()
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    T = X.shape[2]
    if tables is None:
        tables = trig_tables(T, freqs, dtype)
    sin_t, cos_t = (np.asarray(t).astype(dtype) for t in tables)
    if magnitude:
        X = np.abs(X)
        sin_t, cos_t = np.ones_like(sin_t), np.ones_like(cos_t)
    # q[f][m] (T): sin^(S-m) cos^m, 1.0 times the sines first, then the cosines (build_q)
    q = []
    for f in range(sin_t.shape[0]):
        rows = []
        for m in range(S + 1):
            v = np.ones(T, dtype=dtype)
            for _ in range(S - m):
                v = v * sin_t[f]
            for _ in range(m):
                v = v * cos_t[f]
            rows.append(v)
        q.append(rows)
    return X, word_letters(word_strings), q


def _unit_forward(X, letters, q, b, total):
    """(u_1 ... u_(L-1), Y) of one (word, frequency) unit for every series: (N, T) arrays."""
    us = []
    s = _letter(X, letters[0])
    for k in range(1, len(letters)):
        u = np.zeros_like(s)
        for m, qm in enumerate(q):
            u = u + b[m] * (_shift(np.cumsum(s * qm, axis=1)) * qm)
        us.append(u)
        s = u * _letter(X, letters[k])
    if not total:
        return us, np.cumsum(s, axis=1)
    Y = np.zeros_like(s)
    for m, qm in enumerate(q):
        Y = Y + b[m] * (np.cumsum(s * qm, axis=1) * qm)
    return us, Y


def coswiss_forward(X, word_strings, freqs, S, total, tables=None, dtype=HP):
    """The rows (N, W * F, T) by the factorised recursion of csrc/coswiss.h, sequential sums."""
    X, words, q = _prepare(X, word_strings, freqs, S, False, tables, dtype)
    b = [dtype(v) for v in binomials(S)]
    return np.stack([_unit_forward(X, letters, q[f], b, total)[1]
                     for letters in words for f in range(len(q))], axis=1)


def coswiss_grad(X, G, word_strings, freqs, S, total, magnitude=False, tables=None, dtype=HP):
    """d/dX of ``sum G * Y`` by the adjoint of the factorised recursion, sequential sums, in
    ``dtype``.  Per (word of L letters, frequency) unit, q_m = sin^(S-m) cos^m, b_m = C(S, m):

        s_0 = z_0;  k >= 1: u_k[t] = sum_m b_m q_m[t] A_(k-1,m)[t-1],  s_k = u_k z_k,  A_(k,m) = cumsum(s_k q_m)
        non-total: a_(L-1)[t] = sum_(t' >= t) G[t'];  total: a_(L-1)[t] = sum_m b_m q_m[t] sum_(t' >= t) q_m[t'] G[t']
        k = L-1 ... 1:  dz_k = a_k u_k,  du_k = a_k z_k,  a_(k-1)[t] = sum_m b_m q_m[t] sum_(t' > t) q_m[t'] du_k[t']
        dz_0 = a_0;     dX_d += dz_k e_kd x_d^(e_kd - 1) prod over d' != d of x_d'^e_kd'

    ``tables=(sin, cos)``: (F, T) arrays instead of the tables of ``freqs``.  ``magnitude=True``:
    X, G and the coefficients e replaced by their magnitudes and every |sin|, |cos| by 1 - a bound
    of the sum of the magnitudes of the terms."""
    X, words, q = _prepare(X, word_strings, freqs, S, magnitude, tables, dtype)
    G = np.asarray(G, dtype=np.float64).astype(dtype)
    if magnitude:
        G = np.abs(G)
    N, D, T = X.shape
    F = len(q)
    assert G.shape == (N, len(words) * F, T)
    b = [dtype(v) for v in binomials(S)]
    dX = np.zeros((N, D, T), dtype=dtype)
    for w, letters in enumerate(words):
        for f in range(F):
            us, _ = _unit_forward(X, letters, q[f], b, total)
            g = G[:, w * F + f]
            if total:
                a = np.zeros_like(g)
                for m, qm in enumerate(q[f]):
                    a = a + b[m] * (_suffix(qm * g) * qm)
            else:
                a = _suffix(g)
            for k in range(len(letters) - 1, -1, -1):
                dz = a * us[k - 1] if k > 0 else a
                for d, e in enumerate(letters[k]):
                    if e == 0:
                        continue
                    coef = dtype(abs(e) if magnitude else e)
                    dpow = coef * _ipow(X[:, d], e - 1) if e > 0 else coef * (1 / _ipow(X[:, d], 1 - e))
                    dX[:, d] = dX[:, d] + dz * (dpow * _letter(X, letters[k], skip=d))
                if k == 0:
                    break
                du = a * _letter(X, letters[k])
                a = np.zeros_like(g)
                for m, qm in enumerate(q[f]):
                    behind = np.zeros_like(g)
                    behind[:, :-1] = _suffix(qm * du)[:, 1:]
                    a = a + b[m] * (behind * qm)
    return dX


# ------------------------------------------------------------------ the rounding counts
def _trig_ulps(freqs, U):
    """Roundings' worth of ABSOLUTE error of one float64 sin / cos table entry against the
    long-double one: the angle pi t / (f (T-1)) is formed with three roundings (the product, the
    denominator, the quotient), each moving sin / cos by at most |angle| 2^-53 <= (pi / f_min) 2^-53,
    and the device library's own sin / cos adds ``U``.  (The rounding of pi itself, 0.36 2^-53 of
    the angle, is left to the factor 2 in front of the bounds.)"""
    fmin = min(float(np.float32(f)) for f in freqs)
    return 3 * math.ceil(math.pi / fmin) + U


def n_ops_cos(word_strings, T, freqs, S, total, U):
    """Roundings on the longest path of one term of a forward row as csrc/coswiss.h computes it:
    ``|device - R| <= 2 n_ops_cos 2^-53 A`` elementwise with R = ``coswiss_forward`` and A the same
    on |X| with every |sin|, |cos| replaced by 1.  A term is one index tuple and one m per link
    (L - 1 links between letters, one more with total weighting):

    * the scans: L (S + 1 of them per letter, a term runs through one) of at most T-1 additions: L (T-1)
    * the letters, one multiplication or division per elementary letter:                 W
    * per link ``s q_m`` in front of the scan, ``A q_m`` and ``b_m *`` behind it, ``u z`` (not for
      the link of total weighting, counted all the same) and the S additions over m:      links (4 + S)
    * the two q_m of a link: S multiplications each, and S table entries each with
      ``_trig_ulps`` - an entry's absolute error against a magnitude of 1:        2 links S (1 + trig)
    """
    words = word_letters(word_strings)
    L = max(len(w) for w in words)
    W = max(sum(abs(e) for el in w for e in el) for w in words)
    links = L - 1 + (1 if total else 0)
    return L * max(T - 1, 0) + W + links * (4 + S) + 2 * links * S * (1 + _trig_ulps(freqs, U))


def n_ops_grad_cos(word_strings, T, freqs, S, total, U, E=1):
    """Roundings on the longest path of one term of ``dX[n, d, t]`` as fr_iss_backward computes it
    for a CosWISS plan (csrc/kernels_grad_cos.hip), in the manner of ``n_ops_grad``: with it,
    ``|device - R| <= 2 n_ops_grad_cos 2^-53 A`` elementwise, R = ``coswiss_grad`` fed long-double
    tables and A = ``coswiss_grad(magnitude=True)``.

    A term belongs to a unit (word of L letters, frequency), to a letter k of the word - the one
    that is differentiated -, to an index tuple and to one m per link (L - 1 links between letters,
    one more with total weighting).  The device forms it as ``dz_k (dpow others)`` with
    ``dz_k = a_k u_k``: u_k comes through the k links below the letter in the ascending sweep, a_k
    through the links above it in the descending one.  On the way:

    * the scans: k prefix scans below, L - 1 - k suffix scans above and the scan of G, each at
      most T-1 additions - lanes, wave totals and carries only ever join disjoint runs of time
      steps, and an exact zero rounds nothing:                                       L (T-1)
    * the letter values: one per elementary letter of the other letters; at letter k ``others``
      and ``dpow`` (at most |e| + 2, iss_grad_ref.n_ops_grad):                        W + 2
    * per link four products and the S additions over m - ascending ``s q_m``, ``A q_m``,
      ``b_m *``, ``u z``; descending ``a z``, ``q_m du``, ``q_m *`` the sum behind, ``b_m *``;
      total weighting's link ``q_m G``, ``q_m *`` the sum, ``b_m *``:                 links (4 + S)
    * ``a_k u_k``, ``dpow others`` and their product:                                 3
    * the E rows of G that name the unit, added onto an exact zero:                   E - 1
    * the gather over the (unit, letter) pairs whose letter holds the dimension, onto an exact
      zero - at most every letter of every unit:                                      F sum_w L_w - 1
    * the two q_m of a link: S multiplications each (1.0 * sin is exact, counted all the same) and
      S table entries each with ``_trig_ulps`` = 3 ceil(pi / f_min) + U roundings' worth of
      absolute error, against the magnitude 1 they have in A:                 2 links S (1 + trig)

        n = L (T-1) + W + 2 + links (4 + S) + 3 + E - 1 + F sum L_w - 1 + 2 links S (1 + trig)

    L and W of the longest / heaviest word.  ``U``: the error of the device library's double sin /
    cos in ulp - not derived here, see DESIGN.md 4.14.7 for where the tests take it from."""
    words = word_letters(word_strings)
    L = max(len(w) for w in words)
    W = max(sum(abs(e) for el in w for e in el) for w in words)
    links = L - 1 + (1 if total else 0)
    pairs = len(freqs) * sum(len(w) for w in words)
    return (L * max(T - 1, 0) + W + 2 + links * (4 + S) + 3 + (E - 1) + pairs - 1
            + 2 * links * S * (1 + _trig_ulps(freqs, U)))
