"""References for the backward pass of the max semirings Arctic (max, +) and Bayesian (max, x)
(fruits_amd.nn.max_iss, fr_iss_backward_max).

Not a conftest: the modules that need it import it by name.

The scalar that is differentiated is ``sum over n, k, t of G[n, k, t] * Y[n, k, t]`` with ``Y`` the
iterated sums in the row order of ``oracle.ref_numpy.iss_transform(..., semiring=...)``; ``G`` has
the layout of ``fruits_amd.nn.max_iss``'s result, (N, K, T).

* ``grad_max_bruteforce``: the (sub)gradient straight from the definition, in exact rational
  arithmetic - tiny cases only.
* ``iss_grad_max``: the adjoint recursion over the prefix trie, sequential, in ``np.longdouble``;
  the heads always from the float64 forward pass in the reference's operation order.
* ``n_ops_grad_max``: the roundings on the longest path of one term of the gradient.
* ``smallest_gap``: how far the inputs of a case are from a tie.
"""
from fractions import Fraction
from itertools import combinations_with_replacement

import numpy as np

import iss_grad_ref as gr
from oracle import ref_numpy as orc

HP = np.longdouble
SEMIRINGS = ("Arctic", "Bayesian")


# ------------------------------------------------------------------ the definition, exactly
def grad_max_bruteforce(X, G, word_strings, mode="SINGLE", semiring="Arctic"):
    """d/dX of ``sum G * Y`` from the definition

        Y_w[t] = max over i_1 <= ... <= i_p <= t of m_1[i_1] (x) ... (x) m_p[i_p]

    with ``m_k[i] = sum_d e_kd X[d, i]``, (x) = + (Arctic) or ``m_k[i] = prod_d X[d, i]^e_kd``,
    (x) = * (Bayesian, POSITIVE inputs: elsewhere the reference's recursion is not this maximum).
    Every index tuple of every row and every t is visited in ``fractions.Fraction``; of the
    maximisers the one whose reversed tuple ``(i_p, ..., i_1)`` is lexicographically smallest is
    differentiated - a valid subgradient at a tie.  Exact; for ``T <= 6`` and up to 3 letters.
    Returns an (N, D, T) object array of Fractions."""
    assert semiring in SEMIRINGS
    X = np.asarray(X, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    N, D, T = X.shape
    rows = gr.output_prefixes(word_strings, mode)
    assert T <= 6 and all(len(r) <= 3 for r in rows), "grad_max_bruteforce is for tiny cases"
    assert G.shape == (N, len(rows), T)
    arctic = semiring == "Arctic"
    assert arctic or (X > 0).all(), "the Bayesian definition is for positive inputs"
    out = np.empty((N, D, T), dtype=object)
    for n in range(N):
        x = [[Fraction(float(X[n, d, t])) for t in range(T)] for d in range(D)]
        dx = [[Fraction(0)] * T for _ in range(D)]

        def letter(el, t, skip=-1):
            if arctic:
                return sum((e * x[d][t] for d, e in enumerate(el) if e != 0), Fraction(0))
            v = Fraction(1)
            for d, e in enumerate(el):
                if e != 0 and d != skip:
                    v *= x[d][t] ** e
            return v

        for k, letters in enumerate(rows):
            p = len(letters)
            for t in range(T):
                g = Fraction(float(G[n, k, t]))
                if g == 0:
                    continue
                best, arg = None, None
                for idx in combinations_with_replacement(range(t + 1), p):
                    ms = [letter(letters[j], idx[j]) for j in range(p)]
                    if arctic:
                        val = sum(ms, Fraction(0))
                    else:
                        val = Fraction(1)
                        for m in ms:
                            val *= m
                    if best is None or val > best or (val == best and idx[::-1] < arg[::-1]):
                        best, arg = val, idx
                for j in range(p):
                    for d, e in enumerate(letters[j]):
                        if e == 0:
                            continue
                        if arctic:
                            dx[d][arg[j]] += g * e
                            continue
                        rest = Fraction(1)
                        for i in range(p):
                            if i != j:
                                rest *= letter(letters[i], arg[i])
                        dm = e * x[d][arg[j]] ** (e - 1) * letter(letters[j], arg[j], skip=d)
                        dx[d][arg[j]] += g * dm * rest
        for d in range(D):
            for t in range(T):
                out[n, d, t] = dx[d][t]
    return out


# ------------------------------------------------------------------ the float64 forward pass
def _nodes_of(rows):
    """The prefix trie of the output rows: a node is a prefix; parents in front of their children."""
    return sorted({r[:j] for r in rows for j in range(1, len(r) + 1)}, key=lambda r: (len(r), r))


def forward_f64(X, nodes, semiring):
    """({v: z_v}, {v: S_v}) in float64 and in the reference's operation order
    (oracle.ref_numpy.arctic_iterated_sum_fast / bayesian_iterated_sum_fast: per letter
    ``tmp = tmp + el * Z[d]`` resp. repeated ``tmp = tmp * Z[d]`` / ``tmp / Z[d]`` ON the parent's
    running maximum, then the running maximum; no shift).  Every S_v is asserted to be the
    oracle's own row, bit for bit."""
    X = np.asarray(X, dtype=np.float64)
    N, D, T = X.shape
    z, S = {}, {}
    for v in nodes:
        el = list(v[-1]) + [0] * (D - len(v[-1]))
        if semiring == "Arctic":
            tmp = np.zeros((N, T)) if len(v) == 1 else S[v[:-1]]
            for d, e in enumerate(el):
                if e != 0:
                    tmp = tmp + e * X[:, d, :]
        else:
            tmp = orc._letters(np.ones((N, T)) if len(v) == 1 else S[v[:-1]], X, el)
        z[v] = tmp
        S[v] = np.maximum.accumulate(tmp, axis=1)
        word = [list(l) + [0] * (D - len(l)) for l in v]
        want = orc.iterated_sums(X, word, extended=1, semiring=semiring)[:, 0]
        assert np.array_equal(S[v], want), ("forward_f64 is not the oracle's arithmetic", v)
    return z, S


def _heads(S):
    """(N, T) bool: t == 0 or S[t] > S[t-1] - strictly, the first of equal maxima wins."""
    h = np.ones(S.shape, dtype=bool)
    h[:, 1:] = S[:, 1:] > S[:, :-1]
    return h


def smallest_gap(X, word_strings, mode="SINGLE", semiring="Arctic"):
    """The smallest ``|z_v[s] - S_v[s-1]|`` over all nodes v of the trie, series and times s >= 1
    (inf without any): how far the case is from a tie - from an input where a head appears or
    disappears under a perturbation.  0.0: an exact tie."""
    nodes = _nodes_of(gr.output_prefixes(word_strings, mode))
    z, S = forward_f64(X, nodes, semiring)
    gap = np.inf
    for v in nodes:
        if z[v].shape[1] > 1:
            gap = min(gap, float(np.abs(z[v][:, 1:] - S[v][:, :-1]).min()))
    return gap


# ------------------------------------------------------------------ the adjoint recursion
def _segment_sums(B, head):
    """A[s] = sum of B over [s, next head) at a head s, 0 elsewhere; added from the right."""
    A = np.zeros_like(B)
    run = np.zeros(B.shape[0], dtype=B.dtype)
    for t in range(B.shape[1] - 1, -1, -1):
        run = run + B[:, t]
        A[:, t] = np.where(head[:, t], run, 0)
        run = np.where(head[:, t], 0, run)
    return A


def _at_heads(zv, head):
    """S[t] = z[the last head <= t]: the running maximum GIVEN the heads (any dtype)."""
    T = zv.shape[1]
    last = np.maximum.accumulate(np.where(head, np.arange(T)[None, :], 0), axis=1)
    return np.take_along_axis(zv, last, axis=1)


def iss_grad_max(X, G, word_strings, mode="SINGLE", semiring="Arctic", magnitude=False, dtype=HP):
    """d/dX of ``sum G * Y`` for the max semirings by the adjoint recursion, sequential sums, in
    ``dtype``.  Over the nodes v of the prefix trie of the rows (parent p, letter m_v):

        z_v = m_v (x) S_p  (depth 1: m_v),  S_v = running maximum of z_v          (no shift)
        head_v[s]: s == 0 or S_v[s] > S_v[s-1]; a head opens the segment [s, next head)
        B_v[t] = G_v[t] + sum over children c of w_c[t] A_c[t]    (w = 1 Arctic, m_c Bayesian)
        A_v[s] = sum of B_v over the segment of s at a head s, 0 elsewhere
        Arctic:   dX_d[s] += e_vd A_v[s]
        Bayesian: dX_d[s] += A_v[s] S_p[s] e_vd x_d^(e_vd - 1) prod over d' != d of x_d'^e_vd'

    The forward pass that decides the heads ALWAYS runs in float64 in the reference's operation
    order (``forward_f64``): the heads are the ones the device sees.  Only what follows - the
    letter values, S_p given the heads, the sums and products of the adjoint - runs in ``dtype``.
    ``magnitude=True``: G, the coefficients e and the values replaced by their magnitudes, with
    the heads of the SIGNED run - the sum of the magnitudes of the terms."""
    assert semiring in SEMIRINGS
    if np.dtype(dtype).type is not np.float64:
        orc.require_extended_precision()
    X64 = np.asarray(X, dtype=np.float64)
    Xd = X64.astype(dtype)
    Gd = np.asarray(G, dtype=np.float64).astype(dtype)
    if magnitude:
        Xd, Gd = np.abs(Xd), np.abs(Gd)
    N, D, T = X64.shape
    rows = gr.output_prefixes(word_strings, mode)
    assert Gd.shape == (N, len(rows), T)
    nodes = _nodes_of(rows)
    kids = {v: [c for c in nodes if len(c) == len(v) + 1 and c[:-1] == v] for v in nodes}
    _, S64 = forward_f64(X64, nodes, semiring)
    head = {v: _heads(S64[v]) for v in nodes}
    arctic = semiring == "Arctic"
    S = {}
    if not arctic:
        # S_p in `dtype`, the value at the heads the float64 run chose
        for v in nodes:
            m = gr._letter(Xd, v[-1])
            S[v] = _at_heads(m if len(v) == 1 else m * S[v[:-1]], head[v])
    A = {}
    dX = np.zeros((N, D, T), dtype=dtype)
    for v in reversed(nodes):
        B = np.zeros((N, T), dtype=dtype)
        for k, r in enumerate(rows):
            if r == v:
                B = B + Gd[:, k]
        for c in kids[v]:
            B = B + (A[c] if arctic else gr._letter(Xd, c[-1]) * A[c])
        A[v] = _segment_sums(B, head[v])
        for d, e in enumerate(v[-1]):
            if e == 0:
                continue
            coef = dtype(abs(e) if magnitude else e)
            if arctic:
                dX[:, d] = dX[:, d] + coef * A[v]
                continue
            dm = A[v] if len(v) == 1 else A[v] * S[v[:-1]]
            dpow = (coef * gr._ipow(Xd[:, d], e - 1) if e > 0
                    else coef * (1 / gr._ipow(Xd[:, d], 1 - e)))
            dX[:, d] = dX[:, d] + dm * (dpow * gr._letter(Xd, v[-1], skip=d))
    return dX


# ------------------------------------------------------------------ the rounding count
def n_ops_grad_max(word_strings, T, mode="SINGLE", semiring="Arctic"):
    """Roundings on the longest path of one term of ``dX[n, d, s]`` as fr_iss_backward_max computes
    it (csrc/kernels_grad.hip), in the manner of ``iss_grad_ref.n_ops_grad``: with it,
    ``|device - R| <= 2 n_ops_grad_max 2^-53 A`` elementwise, R = ``iss_grad_max`` and A =
    ``iss_grad_max(magnitude=True)``.  Both sides take the heads from the same float64 forward
    pass, so the heads carry no error: given them, the gradient is a sum of products.

    A term belongs to an output row - the prefix u of l_u letters -, to a time t of it and to a
    node v on the path from the root to u whose back-tracked position is s.

    Arctic: the term is ``e_vd G[n, u, t]``.
    * A_v: the segment sums of the nodes from u up to v, l_u - l_v + 1 of them.  A segment's sum
      joins the B of that segment alone (the lane's steps, the wave scan, the wave totals and the
      carry between chunks only ever add disjoint runs of ONE segment, and adding the exact zero
      of an empty run rounds nothing): at most T-1 additions each:             L (T-1)
    * B_v = the E rows of G that v is, then the A of its C children, added one after another
      onto an exact zero: E + C - 1 additions per node of the path:            L (E + C - 1)
    * the sum over the nodes whose letter holds dimension d, onto an exact zero: V - 1
    * the product ``e * A_v``:                                                   1

        n_ops_grad_max(Arctic) = L (T-1) + L (E + C - 1) + V - 1 + 1

    Bayesian: the term is a product of G, of the letter values at the back-tracked positions and
    of the derivative of v's letter; the device forms it as ``A_v[s] * S_p[s] * (dpow * others)``
    with ``m_c * A_c`` per step up the path.  To the sums above (without ``e * A_v``; it is kept
    in the count, which only loosens the bound) come, exactly as ``n_ops_grad`` counts them:
    * the letter values - of p in S_p (the forward walk: one multiplication or division per
      elementary letter, the running maximum rounds nothing), of the nodes below v in B, at v
      ``others`` and ``dpow``: at most one per elementary letter of u and two more:  W + 2
    * the products that join the pieces: ``m_c * A_c`` (l_u - l_v <= L - 1), ``A_v * S_p``,
      ``dpow * others`` and the product of the two:                            L + 2

        n_ops_grad_max(Bayesian) = n_ops_grad_max(Arctic) + W + 2 + L + 2

    with L, W, E, C, V as in ``n_ops_grad``.  One number for the whole call, taken at the full
    length T.  No measured error enters."""
    assert semiring in SEMIRINGS
    rows = gr.output_prefixes(word_strings, mode)
    nodes = {r[:j] for r in rows for j in range(1, len(r) + 1)}
    L = max(len(r) for r in rows)
    W = max(sum(abs(e) for el in r for e in el) for r in rows)
    E = max(sum(1 for r in rows if r == v) for v in nodes)
    C = max(sum(1 for c in nodes if len(c) == len(v) + 1 and c[:-1] == v) for v in nodes)
    V = len(nodes)
    n = L * max(T - 1, 0) + L * (E + C - 1) + V - 1 + 1
    if semiring == "Bayesian":
        n += W + 2 + L + 2
    return n
