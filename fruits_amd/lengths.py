"""Variable-length series: what ``lengths=`` of ``Fruit`` / ``FruitSlice`` means (DESIGN.md,
"Per-series lengths").

``lengths`` is an integer array ``(N,)`` with ``1 <= lengths[n] <= T``; series ``n`` is
``X[n, :, :lengths[n]]``.  What lies behind a series' length (its *tail*) has to be finite and
influences no result: row ``n`` of ``fruit.transform(X, lengths=lengths)`` is what
``fruit.transform(X[n:n+1, :, :lengths[n]])[0]`` returns for the same fitted state.

The iterated sums are causal and need nothing.  This module holds the host side of the rest: the
validation, the gate (one ``_supports_lengths`` hook per seed class), and the two pure functions
that turn lengths into tables - a sieve's cuts resolved per series, and the row of a
series-independent weighting per distinct length.
"""
from __future__ import annotations

from typing import Optional

import numpy as np


def check_lengths(lengths, N: int, T: int) -> Optional[np.ndarray]:
    """``lengths`` as an int64 array (None stays None).

    Raises:
        TypeError: for a dtype that is not an integer.
        ValueError: for a shape other than ``(N,)`` or values outside ``1..T``.
    """
    if lengths is None:
        return None
    arr = np.asarray(lengths)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise TypeError(f"lengths has to be an array of integers, not {arr.dtype}")
    if arr.shape != (N,):
        raise ValueError(f"lengths has to be of shape ({N},), one entry per series, not {arr.shape}")
    if N and (arr.min() < 1 or arr.max() > T):
        raise ValueError(f"lengths has to be in 1..{T} (the padded series length)")
    return arr.astype(np.int64)


def require_support(seeds) -> None:
    """Raises NotImplementedError, naming the seed, for the first of ``seeds`` that does not take
    per-series lengths - before anything is launched."""
    for seed in seeds:
        if not seed._supports_lengths():
            raise NotImplementedError(
                f"{type(seed).__name__} ({seed}) does not support per-series lengths")


def with_lengths(method, *args, **lengths):
    """``method(*args)`` for a dense batch, ``method(*args, lengths=...)`` for a ragged one
    (``lengths``: the one keyword the method takes them by, None for a dense batch).

    The rule: lengths are handed only to seeds that said yes (``require_support``).  A dense call
    never names the parameter, so a user's subclass written without it keeps working."""
    for value in lengths.values():
        if value is None:
            return method(*args)
    return method(*args, **lengths)


def resolve_cuts(cut, lengths) -> np.ndarray:
    """``(N, len(cut) + 1)`` int64 segment boundaries of integer cuts, resolved per series as the
    reference resolves them for a series of that length (SegmentSieve._get_transformed_cuts,
    fruits/sieving/segment.py:51-64): ``c >= 0 -> c``, ``c < 0 -> L_n + c + 1``, every row sorted
    behind its leading 0 - then clipped to ``[0, L_n]``, the extent a slice ``X[lo:hi]`` of a
    series of that length has."""
    L = np.asarray(lengths, dtype=np.int64)
    c = np.asarray(cut, dtype=np.int64)[np.newaxis, :]
    rows = np.zeros((L.shape[0], c.shape[1] + 1), dtype=np.int64)
    rows[:, 1:] = np.where(c >= 0, c, L[:, np.newaxis] + c + 1)
    rows.sort(axis=1)
    return np.clip(rows, 0, L[:, np.newaxis])


def resolve_end_cuts(cut, lengths) -> np.ndarray:
    """END's table: ``rows[n, j + 1] - 1`` is the index END reads of series ``n`` for its
    ``j``-th (sorted) cut, with the wrap of a negative index (``X[:, c - 1]``, numpy's ``-1``)
    made HERE for the series' own length - the kernels wrap by the padded one.

    Raises:
        IndexError: as the reference's np.take_along_axis does for a series whose index
            ``c - 1`` lies outside ``[-L_n, L_n - 1]`` (fruits/sieving/segment.py:213-218).
    """
    L = np.asarray(lengths, dtype=np.int64)
    c = np.asarray(cut, dtype=np.int64)[np.newaxis, :]
    rows = np.zeros((L.shape[0], c.shape[1] + 1), dtype=np.int64)
    rows[:, 1:] = np.where(c >= 0, c, L[:, np.newaxis] + c + 1)
    rows.sort(axis=1)
    idx = rows[:, 1:] - 1
    bad = (idx < -L[:, np.newaxis]) | (idx > L[:, np.newaxis] - 1)
    if bad.any():
        n, j = np.argwhere(bad)[0]
        raise IndexError(f"index {int(idx[n, j])} is out of bounds for axis 1 with size "
                         f"{int(L[n])} (END cut {tuple(cut)}, series {int(n)})")
    rows[:, 1:] = np.where(idx < 0, idx + L[:, np.newaxis], idx) + 1
    rows[:, 0] = 0      # (never read: END takes the upper end of every segment)
    return rows


def lookup_rows(row_of_length, lengths, T: int) -> np.ndarray:
    """``(N, T)`` lookup of a weighting whose row is a function of the series length alone
    (Indices, Plateaus): ``row_of_length(L)`` once per distinct length, zeros behind it."""
    L = np.asarray(lengths, dtype=np.int64)
    table = np.zeros((L.shape[0], T))
    for length in np.unique(L):
        table[L == length, :length] = np.asarray(row_of_length(int(length)), dtype=np.float64)
    return table
