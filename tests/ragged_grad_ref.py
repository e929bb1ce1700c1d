"""Per-series lengths in the backward pass: the existing oracles of the five
adjoints, run series by series on the truncated series ``X[n, :, :L_n]`` with the truncated
upstream ``G[n, :, :L_n]``.  No torch.  Nothing here knows about padding: the expected gradient of
a ragged batch IS the dense oracle on each truncated series, and +0.0 behind it.

Kinds: ``reals`` (iss_grad_ref), ``arctic`` / ``bayesian`` (iss_grad_max_ref), ``nontotal`` /
``total`` (iss_grad_weighted_ref; ``row(L)`` gives the weighting's row of a series of L steps)."""
import numpy as np

import iss_grad_max_ref as gm
import iss_grad_ref as gr
import iss_grad_weighted_ref as gw

KINDS = ("reals", "nontotal", "total", "arctic", "bayesian")
CHUNK = 1024       # time steps the scan kernels take at once (csrc/kernels.h, kGradChunk)
# the lengths at which the kernels change path: a lane's four steps, a wave, a chunk and their edges
CLASSES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1,
           2 * CHUNK, 2 * CHUNK + 3)


def deal(classes, copies, seed):
    """Every class ``copies`` times, dealt over the batch by a seeded permutation."""
    L = np.repeat(np.asarray(classes, dtype=np.int64), copies)
    return L[np.random.default_rng(seed).permutation(L.shape[0])]


def series_grad(kind, Xn, Gn, strings, mode, alphas=None, lookup=None, magnitude=False, dtype=gr.HP):
    """The dense oracle of ``kind`` on one (truncated) series ``(1, D, L)``."""
    if kind == "reals":
        return gr.iss_grad(Xn, Gn, strings, mode, magnitude=magnitude, dtype=dtype)
    if kind in ("arctic", "bayesian"):
        return gm.iss_grad_max(Xn, Gn, strings, mode, kind.capitalize(), magnitude=magnitude, dtype=dtype)
    return gw.iss_grad_weighted(Xn, Gn, strings, alphas, lookup, kind == "total", mode, magnitude=magnitude,
                                dtype=dtype)


def n_ops(kind, strings, L, mode, alphas=None, lookup=None):
    """The operation count of the derived bound of ``kind`` for a series of L steps."""
    if kind == "reals":
        return gr.n_ops_grad(strings, L, mode)
    if kind in ("arctic", "bayesian"):
        return gm.n_ops_grad_max(strings, L, mode, kind.capitalize())
    return gw.n_ops_grad_weighted(strings, alphas, lookup, L, mode)


def truncated(a, n, L):
    """Series n of ``a`` (N, rows, T) up to its length, as a batch of one."""
    return np.ascontiguousarray(a[n:n + 1, :, :L])


def grad(kind, X, G, lengths, strings, mode, alphas=None, row=None, magnitude=False, dtype=gr.HP):
    """``(N, D, T)``: per series the oracle on the truncated series, zeros behind it.  ``G`` is
    never read at ``t >= L_n`` - it may hold anything there."""
    out = np.zeros(X.shape, dtype=dtype)
    for n, L in enumerate(int(v) for v in lengths):
        lookup = None if row is None else np.asarray(row(L), dtype=np.float64)[np.newaxis, :]
        out[n, :, :L] = series_grad(kind, truncated(X, n, L), truncated(G, n, L), strings, mode, alphas,
                                    lookup, magnitude, dtype)[0]
    return out
