"""References for the backward pass of the Reals iterated sums weighted with the path length of
the input itself (fruits_amd.nn.pathlen_iss, fr_plan_set_grad_pathlen).  Builds
on iss_grad_ref.py and iss_grad_weighted_ref.py.

Not a conftest: the modules that need it import it by name.

The scalar that is differentiated is ``sum over n, k, t of G[n, k, t] * Y[n, k, t]`` with ``Y`` the
weighted iterated sums ``oracle.ref_numpy.iss_transform(X, word_strings, mode, alphas, g(X), total)``
and ``g = scale * r / r[T-1]``, ``r = cumsum(|dx_0|)`` (L1) or ``cumsum(dx_0^2)`` (L2).  The gradient
with respect to ``X`` is the sum of the INPUT part - ``iss_grad_weighted``, g held constant - and
the LOOKUP part: ``dg = dL/dg`` gathered over the trie, then carried through the normalised
cumulative sum into dimension 0.

* ``iss_grad_lookup``: dg (N, T) by the recursion of DESIGN.md 4.14.8, sequential, ``np.longdouble``.
* ``pathlen_grad``: dg -> what it adds to ``dX[:, 0, :]``.
* ``iss_grad_pathlen``: input part + lookup part.
* ``n_ops_grad_pathlen``: the roundings on the longest path of one term.
"""
import numpy as np

import iss_grad_ref as gr
import iss_grad_weighted_ref as gw
from iss_grad_ref import HP, orc


def iss_grad_lookup(X, G, word_strings, alphas, lookup, total, mode="SINGLE", magnitude=False, dtype=HP):
    """dL/dg (N, T), the exp factors ``exp(+-g alpha)`` being the only way g reaches L.  In the
    notation of ``iss_grad_weighted`` (alpha_v the float32 alpha of v's last letter, alpha_p its
    parent's, 0 at depth 1; dm_v what the input gather forms; m_v the letter's value):

        total:      dg = sum_v (alpha_v - alpha_p) dm_v m_v  -  sum over rows v of alpha_v G_v S_v,
                    S_v = C_v E-_v
        non-total:  dg = sum over v with children of alpha_v R_v y_v  -  sum over v of depth >= 2
                    of alpha_p dm_v m_v,        R_v = suffix(Q_v) = dL/dy_v,   y_v = z_v E+_v

    (total: every y_v carries E-_p E+_v and dL/dy_v y_v = dm_v m_v, every emitted row E-_v; non-total:
    z_v carries E-_p and dL/dz_v z_v = dm_v m_v, and y_v = z_v E+_v is read by the children alone.)
    ``magnitude=True``: X and G replaced by their magnitudes and every term added with its absolute
    value."""
    if np.dtype(dtype).type is not np.float64:
        orc.require_extended_precision()
    X = np.asarray(X, dtype=np.float64).astype(dtype)
    G = np.asarray(G, dtype=np.float64).astype(dtype)
    if magnitude:
        X, G = np.abs(X), np.abs(G)
    N, D, T = X.shape
    rows = gw.output_nodes(word_strings, alphas, mode)
    assert G.shape == (N, len(rows), T)
    nodes = gw.trie_nodes(rows)
    kids = {v: [c for c in nodes if len(c) == len(v) + 1 and c[:-1] == v] for v in nodes}
    g = np.broadcast_to(np.asarray(lookup, dtype=np.float64), (N, T)).astype(dtype)
    keys = {v[-1][1] for v in nodes}
    Ep = {a: np.exp(g * dtype(np.float32(a))) for a in keys}
    Em = {a: np.exp(-g * dtype(np.float32(a))) for a in keys}
    sign = dtype(1 if magnitude else -1)
    C, Y = {}, {}
    for v in nodes:
        y = gr._letter(X, v[-1][0]) * Ep[v[-1][1]]
        if len(v) > 1:
            y = y * Em[v[-2][1]] * gr._shift(C[v[:-1]])
        Y[v] = y
        C[v] = np.cumsum(y, axis=1)
    A = {}
    dg = np.zeros((N, T), dtype=dtype)
    for v in reversed(nodes):
        a_v = dtype(np.float32(v[-1][1]))
        a_p = dtype(np.float32(v[-2][1])) if len(v) > 1 else dtype(0)
        Gv = np.zeros((N, T), dtype=dtype)
        for k, r in enumerate(rows):
            if r == v:
                Gv = Gv + G[:, k]
        Q = np.zeros((N, T), dtype=dtype)
        for c in kids[v]:
            term = gr._letter(X, c[-1][0]) * Em[v[-1][1]] * A[c]
            if total:
                term = term * Ep[c[-1][1]]
            Q[:, :-1] = Q[:, :-1] + term[:, 1:]
        if total:
            A[v] = gr._suffix(Gv * Em[v[-1][1]] + Q)
            dm = A[v] * Ep[v[-1][1]]
        else:
            R = gr._suffix(Q)
            A[v] = gr._suffix(Gv) + Ep[v[-1][1]] * R
            dm = A[v]
        if len(v) > 1:
            dm = dm * Em[v[-2][1]] * gr._shift(C[v[:-1]])
        dmm = dm * gr._letter(X, v[-1][0])
        if total:
            diff = a_v - a_p
            dg = dg + (abs(diff) if magnitude else diff) * dmm
            if any(r == v for r in rows):
                dg = dg + sign * a_v * (Gv * (C[v] * Em[v[-1][1]]))
        else:
            if kids[v]:
                dg = dg + a_v * (R * Y[v])
            if len(v) > 1:
                dg = dg + sign * a_p * dmm
    return dg


def pathlen_grad(X, dg, g, norm, scale, magnitude=False, dtype=HP):
    """What dg (N, T) adds to ``dX[:, 0, :]`` through ``g = scale r / r_L``, ``r = cumsum(f(dx_0))``,
    ``f = |.|`` (norm 1) or ``.^2`` (norm 2), ``r[0] = 0``, ``r_L = r[T-1]``:

        dr[t] = scale dg[t] / r_L,      dr[T-1] -= sum_s dg[s] g[s] / r_L
        D[t]  = sum over s >= t of dr[s]
        dX0[t] = w_t D[t] - w_(t+1) D[t+1],     w_t = sign(dx_t) | 2 dx_t,   w_0 = w_T = 0

    ``sign(0) = 0``.  A series with ``r_L = 0`` (a constant dimension 0; T = 1) gets exact zeros.
    ``g``: the lookup the device used, an input.  ``magnitude=True``: every term with its absolute
    value.  Returns (N, T)."""
    x0 = np.asarray(X, dtype=np.float64)[:, 0, :].astype(dtype)
    dg = np.asarray(dg).astype(dtype)
    g = np.broadcast_to(np.asarray(g, dtype=np.float64), dg.shape).astype(dtype)
    N, T = dg.shape
    out = np.zeros((N, T), dtype=dtype)
    if T < 2:
        return out
    delta = np.zeros((N, T + 1), dtype=dtype)          # delta[:, t] = x[t] - x[t-1], 0 at t = 0 and t = T
    delta[:, 1:T] = x0[:, 1:] - x0[:, :-1]
    f = np.abs(delta) if norm == 1 else delta * delta
    rL = f.sum(axis=1)
    w = np.sign(delta) if norm == 1 else 2 * delta
    if magnitude:
        dg, g, w = np.abs(dg), np.abs(g), np.abs(w)
    for n in range(N):
        if rL[n] == 0:
            continue
        dr = dtype(scale) * dg[n] / rL[n]
        P = (dg[n] * g[n]).sum() / rL[n]
        dr[T - 1] = dr[T - 1] + P if magnitude else dr[T - 1] - P
        Dn = np.zeros(T + 1, dtype=dtype)
        Dn[:T] = np.cumsum(dr[::-1])[::-1]
        a, b = w[n, :T] * Dn[:T], w[n, 1:] * Dn[1:]
        out[n] = a + b if magnitude else a - b
    return out


def iss_grad_pathlen(X, G, word_strings, alphas, lookup, total, norm, scale, mode="SINGLE",
                     magnitude=False, dtype=HP, parts=False):
    """The full gradient (N, D, T): ``iss_grad_weighted`` on the lookup plus ``pathlen_grad`` of
    ``iss_grad_lookup`` in dimension 0.  ``parts=True``: (input part, lookup part (N, T))."""
    inp = gw.iss_grad_weighted(X, G, word_strings, alphas, lookup, total, mode, magnitude=magnitude, dtype=dtype)
    dg = iss_grad_lookup(X, G, word_strings, alphas, lookup, total, mode, magnitude=magnitude, dtype=dtype)
    look = pathlen_grad(X, dg, lookup, norm, scale, magnitude=magnitude, dtype=dtype)
    if parts:
        return inp, look
    out = inp.copy()
    out[:, 0] = out[:, 0] + look
    return out


def n_ops_grad_lookup(word_strings, alphas, lookup, T, mode="SINGLE"):
    """Roundings on the longest path of one term of ``dg[n, t]`` as grad_lookup_kernel forms it.
    A term is ``alpha * (dm_v * m_v)``, ``alpha_v * (G_v * (C_v * E-_v))`` or ``alpha_v * (R_v * y_v)``:

    * dm_v, C_v, R_v and G_v lie on the paths ``n_ops_grad_weighted`` counts (R_v is a suffix scan
      of the adjoint, C_v a carried sum, G_v the rows of one node): at most  n_ops_grad_weighted
    * the letter m_v again (``letter_value``: at most W), or y_v = m_v E-_p C_p E+_v (W + 3), or
      C_v E-_v (1), each exp factor with its own error counted in the 4 L (...) of the weighted
      count; then the two products of the term and the difference alpha_v - alpha_p     W + 3 + 3
    * the terms added one after another onto an exact zero, at most two per node        2 V
    """
    rows = gw.output_nodes(word_strings, alphas, mode)
    V = len(gw.trie_nodes(rows))
    W = max(sum(abs(e) for el, _ in r for e in el) for r in rows)
    return gw.n_ops_grad_weighted(word_strings, alphas, lookup, T, mode) + W + 6 + 2 * V


def n_ops_grad_pathlen(word_strings, alphas, lookup, T, mode="SINGLE"):
    """Roundings on the longest path of one term of ``dX[n, 0, t]`` as the armed
    fr_iss_backward_weighted computes it: with it ``|device - R| <= 2 n 2^-53 A`` elementwise, R =
    ``iss_grad_pathlen`` and A = ``iss_grad_pathlen(magnitude=True)``, both on the DEVICE'S OWN
    lookup (the forward lookup's rounding stays outside the bound).

    The input part is ``n_ops_grad_weighted``; a term of the lookup part passes

    * one term of dg (``n_ops_grad_lookup``):         n_ops_grad_weighted + W + 6 + 2 V
    * ``sum dg g``: a product and at most T - 1 additions (a block reduction has fewer)       T
    * r_L, the divisor of everything: per step a difference and an absolute value or a square,
      at most T - 1 additions; its relative error is that of every quotient                 T + 1
    * ``scale * dg / r_L``, ``P / r_L`` and the subtraction at T - 1                           4
    * the suffix scan D: at most T - 1 additions                                           T - 1
    * ``w_t D[t]`` (the difference dx_t is one rounding, the factor 2 none), the difference of the
      two products, the addition onto the input part                                           4

        n_ops_grad_pathlen = n_ops_grad_weighted + W + 2 V + 3 T + 14

    One number for the whole call; no measured error enters."""
    return n_ops_grad_lookup(word_strings, alphas, lookup, T, mode) + 3 * T + 8
