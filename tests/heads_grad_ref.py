"""The heads of ``fruits_amd.nn.iss_band_features`` in numpy - MPI and CUR beside the selecting
sieves END / MAX / MIN - and the dense gradient of the rows that their feature gradients are: the
reference of ``fr_sieve_heads`` and ``fr_sieve_heads_adjoint``.  No torch.

A sieve is a tuple - ``("MPI", cuts, thresholds, inc)``, ``("CUR", cuts, thresholds)``, or one of
``features_grad_ref`` - or a sieve object of ``fruits_amd.sieving`` (``spec_of`` reads it; AVG and
STD are CUR).  Everything is float64 and performed in the order the contract states:

    E a[t] = a[t] - a[t-1] (t >= 1), E a[0] = 0;  D = E^r Y, r = inc (MPI) or 2 (CUR)
    MPI: phi = (sum of in-band D[t]) / c, 0 for c = 0; weight on D[t]: g / (double)c
    CUR: phi = sum of in-band D[t]^2;                  weight on D[t]: (2.0 * g) * D[t]
    per sieve u = +0.0, plus the weights in column order; contribution (E^T)^r u with
    (E^T u)[s] = (s >= 1 ? u[s] : 0.0) - (s + 1 < L ? u[s+1] : 0.0)
    G = +0.0 plus the sieves' contributions in head order (a selecting sieve: its pairs in turn)
"""
import numpy as np

import features_grad_ref as fg

SELECTING = ("END", "MAX", "MIN")


def spec_of(sieve):
    if isinstance(sieve, tuple):
        return sieve
    name = type(sieve).__name__
    if name in SELECTING:
        return fg.spec_of(sieve)
    base = fg.spec_of(sieve)
    if name == "MPI":
        return ("MPI", base[1], base[2], int(sieve._inc))
    if name in ("CUR", "AVG", "STD"):
        return ("CUR", base[1], base[2])
    raise ValueError(f"{name} is no head")


def order_of(spec):
    return spec[3] if spec[0] == "MPI" else (2 if spec[0] == "CUR" else 0)


def nfeatures(sieves):
    return sum(len(s[1]) * (1 if s[0] == "END" else len(s[2]) - 1) for s in map(spec_of, sieves))


def increments(Y, r):
    """``E^r Y`` along the last axis."""
    D = np.array(Y, dtype=np.float64)
    for _ in range(r):
        E = np.zeros_like(D)
        E[..., 1:] = D[..., 1:] - D[..., :-1]
        D = E
    return D


def transposed_increments(u, r):
    """``(E^T)^r u`` along the last axis (extent: the axis)."""
    u = np.array(u, dtype=np.float64)
    for _ in range(r):
        a = u.copy()
        a[..., 0] = 0.0
        b = np.zeros_like(u)
        b[..., :-1] = u[..., 1:]
        u = a - b
    return u


def masks(D, spec):
    """Per feature of a band sieve, in column order: the (N, K, T) mask of the elements it holds."""
    T = D.shape[-1]
    row = fg.cut_row(spec[1], T)
    t = np.arange(T)
    for j in range(len(row) - 1):
        lo, hi = max(row[j], 0), min(row[j + 1], T)
        for b in range(len(spec[2]) - 1):
            yield (t >= lo) & (t < hi) & (spec[2][b] < D) & (D <= spec[2][b + 1])


def _per_series(fn, Y, lengths, *more):
    """``fn`` on every truncated series ``Y[n:n+1, :, :lengths[n]]``, as a list."""
    return [fn(Y[n:n + 1, :, :int(L)], *(m[n:n + 1] for m in more)) for n, L in enumerate(lengths)]


def heads(Y, sieves, lengths=None):
    """``(features, companion)``, both ``(N, K, F)``, of the rows ``Y`` ``(N, K, T)``: the companion
    is the position of a selecting feature and the in-band count of an MPI / CUR one.  With
    ``lengths``, series n is ``Y[n, :, :lengths[n]]``."""
    Y = np.asarray(Y, dtype=np.float64)
    if lengths is not None:
        outs = _per_series(lambda y: heads(y, sieves), Y, lengths)
        return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])
    feats, comp = [], []
    for s in map(spec_of, sieves):
        if s[0] in SELECTING:
            f, p = fg.pick(Y, [s])
            feats.append(f)
            comp.append(p)
            continue
        D = increments(Y, order_of(s))
        for mask in masks(D, s):
            c = mask.sum(axis=-1)
            total = np.where(mask, D * D if s[0] == "CUR" else D, 0.0).sum(axis=-1)
            feats.append((total if s[0] == "CUR" else np.where(c > 0, total / np.maximum(c, 1), 0.0))[..., None])
            comp.append(c.astype(np.int32)[..., None])
    return np.concatenate(feats, axis=-1), np.concatenate(comp, axis=-1)


def band_upstream(Y, sieves, companion, g, lengths=None):
    """The ``(N, K, T)`` gradient of the rows that the feature gradients ``g`` (``(N, K, F)`` or
    ``(N, K * F)``) are; ``companion`` as ``heads`` returns it.  With ``lengths`` the gradient of
    series n is that of the truncated series, and +0.0 behind it."""
    Y = np.asarray(Y, dtype=np.float64)
    N, K, T = Y.shape
    companion = np.asarray(companion)
    g = np.asarray(g, dtype=np.float64).reshape(companion.shape)
    if lengths is not None:
        G = np.zeros((N, K, T))
        outs = _per_series(lambda y, c, w: band_upstream(y, sieves, c, w), Y, lengths, companion, g)
        for n, L in enumerate(lengths):
            G[n, :, :int(L)] = outs[n][0]
        return G
    G = np.zeros((N, K, T))
    n_at, k_at = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    f = 0
    for s in map(spec_of, sieves):
        if s[0] in SELECTING:
            for _ in range(len(s[1]) * (1 if s[0] == "END" else len(s[2]) - 1)):
                p = companion[:, :, f]
                ok = p >= 0
                G[n_at[ok], k_at[ok], p[ok]] += g[:, :, f][ok]
                f += 1
            continue
        r = order_of(s)
        D = increments(Y, r)
        u = np.zeros((N, K, T))
        for mask in masks(D, s):
            gf = g[:, :, f]
            if s[0] == "MPI":
                c = companion[:, :, f].astype(np.float64)
                w = np.divide(gf, c, out=np.zeros_like(gf), where=c > 0)[..., None]
                u = np.where(mask, u + w, u)
            else:
                u = np.where(mask, u + (2.0 * gf)[..., None] * D, u)
            f += 1
        G = G + transposed_increments(u, r)
    return G


def threshold_distance(Y, sieves, lead=None):
    """The smallest distance of any ``D[t]`` of any band sieve to one of its finite thresholds
    (inf: none).  Left out are the elements that are 0 whatever the input holds: ``D[0]`` of an
    order >= 1, and the first ``lead[k]`` steps of row k (``(K,)`` ints: an iterated sum of p
    letters is 0 on its first p - 1 steps, and so is every difference of it)."""
    Y = np.asarray(Y, dtype=np.float64)
    lead = np.zeros(Y.shape[1], dtype=np.int64) if lead is None else np.asarray(lead)
    t = np.arange(Y.shape[-1])
    dist = np.inf
    for s in map(spec_of, sieves):
        if s[0] in SELECTING:
            continue
        D = increments(Y, order_of(s))
        free = t[None, :] >= np.maximum(lead, 1 if order_of(s) >= 1 else 0)[:, None]          # (K, T)
        for q in s[2]:
            if np.isfinite(q) and free.any():
                dist = min(dist, float(np.abs(D - q)[:, free].min()))
    return dist
