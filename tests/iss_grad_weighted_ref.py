"""References for the backward pass of the WEIGHTED Reals iterated sums (fruits_amd.nn.weighted_iss,
fr_iss_backward_weighted).  Builds on iss_grad_ref.py.

Not a conftest: the modules that need it import it by name.

The scalar that is differentiated is ``sum over n, k, t of G[n, k, t] * Y[n, k, t]`` with ``Y`` the
weighted iterated sums in the row order of ``oracle.ref_numpy.iss_transform(X, word_strings, mode,
alphas, lookup, total)``; the gradient is taken with respect to ``X`` (N, D, T), the lookup and with
it every exp factor being a constant.  ``alphas``: one float32 array per word, one value per letter.

* ``grad_weighted_bruteforce``: the gradient from the definition, in exact rational arithmetic.
* ``iss_grad_weighted``: the adjoint recursion, sequential, in ``np.longdouble``.
* ``n_ops_grad_weighted``: the roundings on the longest path of one term of the gradient.
"""
import math
from fractions import Fraction
from itertools import combinations

import numpy as np

import iss_grad_ref as gr
from iss_grad_ref import HP, orc


def alpha_key(a):
    """What names an alpha: the float of its float32 value (a node of the trie is keyed by the
    bits of its letter's alpha, csrc/plan.cpp)."""
    return float(np.float32(a))


def output_nodes(word_strings, alphas, mode="SINGLE"):
    """Per output row of ``orc.iss_transform(X, word_strings, mode, alphas, ...)`` the node it is
    the weighted iterated sum of: a tuple of (letter, alpha) pairs - the letters of
    ``iss_grad_ref.output_prefixes`` with the alphas of the word that emits the row."""
    depths = orc.cache_plan(word_strings) if mode == "EXTENDED" else [1] * len(word_strings)
    out = []
    for s, depth, al in zip(word_strings, depths, alphas):
        letters = gr.output_prefixes([s])[0]
        assert len(al) == len(letters), (s, al)
        pairs = tuple((el, alpha_key(a)) for el, a in zip(letters, al))
        for length in range(len(pairs) - depth + 1, len(pairs) + 1):
            out.append(pairs[:length])
    return out


def trie_nodes(rows):
    """The nodes of the prefix trie of the rows, parents in front of their children."""
    return sorted({r[:j] for r in rows for j in range(1, len(r) + 1)}, key=lambda r: (len(r), r))


# ------------------------------------------------------------------ the definition, exactly
def grad_weighted_bruteforce(X, G, word_strings, alphas, Eplus, Eminus, total, mode="SINGLE"):
    """d/dX of ``sum G * Y`` from the definition over all index tuples, in ``fractions.Fraction``:

        non-total:  Y_w[t] = sum over i_1 < ... < i_p <= t of prod_k m_k[i_k]
                             * prod over k < p of E+_{alpha_k}[i_k] E-_{alpha_k}[i_(k+1)]
        total:      that times E+_{alpha_p}[i_p] E-_{alpha_p}[t]

    ``m_k[i] = prod_d X[d, i]^e_kd``.  ``Eplus`` / ``Eminus``: dicts alpha -> (T,) float64 table,
    taken as exact rationals (they need not be reciprocal, nor exponentials at all).  Exact; for
    ``T <= 7`` and up to 3 letters.  Returns an (N, D, T) object array of Fractions."""
    X = np.asarray(X, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    N, D, T = X.shape
    rows = output_nodes(word_strings, alphas, mode)
    assert T <= 7 and all(len(r) <= 3 for r in rows), "grad_weighted_bruteforce is for tiny cases"
    assert G.shape == (N, len(rows), T)
    ep = {a: [Fraction(float(v)) for v in tab] for a, tab in Eplus.items()}
    em = {a: [Fraction(float(v)) for v in tab] for a, tab in Eminus.items()}
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

        for k, row in enumerate(rows):
            p = len(row)
            for t in range(T):
                g = Fraction(float(G[n, k, t]))
                if g == 0:
                    continue
                for idx in combinations(range(t + 1), p):
                    weight = Fraction(1)
                    for j in range(p - 1):
                        weight *= ep[row[j][1]][idx[j]] * em[row[j][1]][idx[j + 1]]
                    if total:
                        weight *= ep[row[-1][1]][idx[-1]] * em[row[-1][1]][t]
                    ms = [letter(row[j][0], idx[j]) for j in range(p)]
                    for j in range(p):
                        rest = weight
                        for i in range(p):
                            if i != j:
                                rest *= ms[i]
                        for d, e in enumerate(row[j][0]):
                            if e == 0:
                                continue
                            dm = e * x[d][idx[j]] ** (e - 1) * letter(row[j][0], idx[j], skip=d)
                            dx[d][idx[j]] += g * dm * rest
        for d in range(D):
            for t in range(T):
                out[n, d, t] = dx[d][t]
    return out


# ------------------------------------------------------------------ the adjoint recursion
def iss_grad_weighted(X, G, word_strings, alphas, lookup, total, mode="SINGLE", magnitude=False,
                      dtype=HP, tables=None):
    """d/dX of ``sum G * Y`` by the adjoint recursion, sequential sums, in ``dtype``.  Over the nodes
    v of the (letters, alphas) prefix trie (parent p, letter m_v, E+_v = exp(g alpha_v), E-_v =
    exp(-g alpha_v) of the node's last letter), the carried sums root first

        y_v = m_v E-_p E+_v shift(C_p)      (depth 1: m_v E+_v),      C_v = cumsum(y_v)

    and the adjoint deepest first (G_v: the rows v is, summed; c: the children of v):

        total:      B_v[s] = G_v[s] E-_v[s] + sum_c (m_c E-_v E+_c A_c)[s+1],   A_v = suffix(B_v)
                    dm_v   = A_v E-_p E+_v shift(C_p)                  (depth 1: A_v E+_v)
        non-total:  Q_v[s] = sum_c (m_c E-_v A_c)[s+1],   A_v = suffix(G_v) + E+_v suffix(Q_v)
                    dm_v   = A_v E-_p shift(C_p)                       (depth 1: A_v)
        dX_d += dm_v * e_vd x_d^(e_vd - 1) prod over d' != d of x_d'^e_vd'

    ``lookup``: g, (1 | N, T).  ``tables=(Eplus, Eminus)``: dicts alpha -> (T,) or (N, T) table that
    replace the exponentials (exact cases).  ``magnitude=True``: X, G and the coefficients e
    replaced by their magnitudes; the weights are positive and stay."""
    if np.dtype(dtype).type is not np.float64:
        orc.require_extended_precision()
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    G = np.asarray(G, dtype=np.float64).astype(dtype)
    if magnitude:
        X, G = np.abs(X), np.abs(G)
    N, D, T = X.shape
    rows = output_nodes(word_strings, alphas, mode)
    assert G.shape == (N, len(rows), T)
    nodes = trie_nodes(rows)
    kids = {v: [c for c in nodes if len(c) == len(v) + 1 and c[:-1] == v] for v in nodes}
    if tables is None:
        g = np.broadcast_to(np.asarray(lookup, dtype=np.float64), (N, T)).astype(dtype)
        keys = {v[-1][1] for v in nodes}
        # (the alpha is a float32, the product and the exponential are taken in ``dtype``)
        Ep = {a: np.exp(g * dtype(np.float32(a))) for a in keys}
        Em = {a: np.exp(-g * dtype(np.float32(a))) for a in keys}
    else:
        Ep = {a: np.broadcast_to(np.asarray(t, dtype=np.float64), (N, T)).astype(dtype)
              for a, t in tables[0].items()}
        Em = {a: np.broadcast_to(np.asarray(t, dtype=np.float64), (N, T)).astype(dtype)
              for a, t in tables[1].items()}
    C = {}
    for v in nodes:
        y = gr._letter(X, v[-1][0]) * Ep[v[-1][1]]
        if len(v) > 1:
            y = y * Em[v[-2][1]] * gr._shift(C[v[:-1]])
        C[v] = np.cumsum(y, axis=1)
    A = {}
    dX = np.zeros((N, D, T), dtype=dtype)
    for v in reversed(nodes):
        a_v = v[-1][1]
        Gv = np.zeros((N, T), dtype=dtype)
        for k, r in enumerate(rows):
            if r == v:
                Gv = Gv + G[:, k]
        Q = np.zeros((N, T), dtype=dtype)
        for c in kids[v]:
            term = gr._letter(X, c[-1][0]) * Em[a_v] * A[c]
            if total:
                term = term * Ep[c[-1][1]]
            Q[:, :-1] = Q[:, :-1] + term[:, 1:]
        if total:
            A[v] = gr._suffix(Gv * Em[a_v] + Q)
            dm = A[v] * Ep[a_v]
        else:
            A[v] = gr._suffix(Gv) + Ep[a_v] * gr._suffix(Q)
            dm = A[v]
        if len(v) > 1:
            dm = dm * Em[v[-2][1]] * gr._shift(C[v[:-1]])
        el = v[-1][0]
        for d, e in enumerate(el):
            if e == 0:
                continue
            coef = dtype(abs(e) if magnitude else e)
            dpow = (coef * gr._ipow(X[:, d], e - 1) if e > 0
                    else coef * (1 / gr._ipow(X[:, d], 1 - e)))
            dX[:, d] = dX[:, d] + dm * (dpow * gr._letter(X, el, skip=d))
    return dX


# ------------------------------------------------------------------ the rounding count
def n_ops_grad_weighted(word_strings, alphas, lookup, T, mode="SINGLE"):
    """Roundings on the longest path of one term of ``dX[n, d, t]`` as fr_iss_backward_weighted
    computes it (csrc/kernels_grad.hip): with it ``|device - R| <= 2 n 2^-53 A`` elementwise, R =
    ``iss_grad_weighted`` and A = ``iss_grad_weighted(magnitude=True)``.

    The count is that of ``iss_grad_ref.n_ops_grad`` - its derivation holds word for word with
    the carried sums C_p in the place of S_p, formed by a prefix scan of at most T-1 additions
    per letter instead of the forward walk -

        L (T-1) + W + 2 + L + 2 + L (E + C - 1) + V - 1

    taken on the (letters, alphas) trie: two prefixes with equal letters and other alphas are two
    nodes, so E (rows one node is), C (children of one node) and V (nodes) are counted there.
    The weighting adds, per letter on a term's path (the term of output row u at node v passes
    the letters of u: those above v in C_p, v's own in dm_v, those below v in the adjoint):

    * multiplications by exp tables: forming C_p multiplies every letter above v by its parent's
      E- and its own E+; the adjoint multiplies every step from a child up to its parent by the
      parent's E- and an E+ (total: the child's, in B; non-total: the parent's, behind the scan
      of Q), the row u itself by E-_u (total), and dm_v by E-_p and (total) E+_v.  That is
      2 (l_v - 1) + 2 (l_u - l_v) + 3 = 2 l_u + 1 <= 4 L: at most one multiplication by an E+
      and one by an E- per letter on the forward side and as many on the adjoint side   4 L
    * every such factor's own error, as tests/iss_bounds.py ``n_ops`` counts it: its argument
      g * alpha is a rounded product, which moves exp by a relative |g alpha| u <=
      ceil(alpha_max g_max) u, and exp is taken to 1 ulp <= 2 u           4 L (2 + ceil(a g))
    * non-total: the addition that joins suffix(G_v) and E+_v suffix(Q_v), one per node on the
      path from u up to v                                                                   L

        n_ops_grad_weighted = [n_ops_grad on the weighted trie] + 4 L (3 + ceil(alpha_max g_max)) + L

    One number for the whole call, at the full length T; alpha_max and g_max are the largest of
    the whole call.  No measured error enters."""
    rows = output_nodes(word_strings, alphas, mode)
    nodes = set(trie_nodes(rows))
    L = max(len(r) for r in rows)
    W = max(sum(abs(e) for el, _ in r for e in el) for r in rows)
    E = max(sum(1 for r in rows if r == v) for v in nodes)
    C = max(sum(1 for c in nodes if len(c) == len(v) + 1 and c[:-1] == v) for v in nodes)
    V = len(nodes)
    a_max = max(abs(a) for r in rows for _, a in r)
    g_max = float(np.max(np.abs(lookup))) if np.size(lookup) else 0.0
    plain = L * max(T - 1, 0) + W + 2 + L + 2 + L * (E + C - 1) + V - 1
    return plain + 4 * L * (3 + math.ceil(a_max * g_max)) + L
