"""The filters: preparateurs that set parts of every series to zero (mirrors DIL, WIN, DOT and
PDD of fruits/preparation/filter.py).  All four run as ONE HIP kernel, ``fr_prep_mask``: DIL, DOT
and PDD hand it a bit mask over the time steps, built on the host from the fitted state and
uploaded once per fit, WIN the per-series coquantile counts of the shared seed cache, which are
computed on the device and stay there.

The fits draw from numpy's GLOBAL generator with the reference's calls in the reference's order
and read ``X.shape`` alone."""
from __future__ import annotations

from typing import Any, Optional, Union

import numpy as np

from .. import _native as nat
from ..cache import CacheType
from .abstract import Preparateur
from .transform import _seed_cache, _ShapeFitted, _TimeMasked

__all__ = ["DIL", "WIN", "DOT", "PDD"]


class DIL(_TimeMasked, _ShapeFitted):
    """Dilation: random strips of every series are set to zero
    (fruits/preparation/filter.py:11-68).

    Args:
        clusters: a float in [0, 1] makes ``clusters * T`` strips; None a random number of them
            between 1 and ``floor(T / 10) - 1``.
    """

    def __init__(self, clusters: Optional[float] = None) -> None:
        self._clusters = clusters

    def _fit(self, X: np.ndarray) -> None:
        T = X.shape[2]
        # the reference's draws in its order (filter.py:34-54): the number of strips, where they
        # start, then one length per strip - a strip ends in front of the next one
        if self._clusters is not None:
            count = int(self._clusters * T)
        elif int(np.floor(T / 10.0)) <= 1:
            count = 1
        else:
            count = np.random.randint(1, int(np.floor(T / 10.0)))
        if count >= T:
            self._indices = np.arange(T)
        else:
            self._indices = np.sort(np.random.choice(T, size=count, replace=False))
        ends = list(self._indices[1:count]) + [T]
        self._lengths = [np.random.randint(1, ends[i] - self._indices[i] + 1)
                         for i in range(count)]

    def _check_fitted(self) -> None:
        if not hasattr(self, "_indices") or not hasattr(self, "_lengths"):
            raise RuntimeError("Missing call of self.fit()")

    def _time_mask(self, T: int) -> np.ndarray:
        keep = np.ones(T, dtype=bool)
        for start, length in zip(self._indices, self._lengths):
            keep[start:start + length] = False
        return keep

    def _mask_state(self) -> tuple:
        return (np.asarray(self._indices).tobytes(), tuple(int(n) for n in self._lengths))

    def _transform_device(self, Xd):
        self._check_fitted()
        return self._masked_device(Xd)

    def _copy(self) -> "DIL":
        return DIL(self._clusters)

    def __str__(self) -> str:
        return f"DIL(clusters={self._clusters})"


class WIN(Preparateur):
    """Window: outside of a window every series is zero.  The window of a series lies between
    two quantiles of its quadratic variation - the coquantiles of the cumulative L2 path length
    of the fruit's input (fruits/preparation/filter.py:71-120).  Row ``i`` of a batch takes the
    window of row ``i`` of the cache's input.

    Args:
        start: quantile at which the window starts, in [0, 1].
        end: quantile at which it ends.
    """

    def __init__(self, start: float, end: float) -> None:
        self._start = start
        self._end = end

    @property
    def requires_fitting(self) -> bool:
        return False

    def _transform_device(self, Xd):
        cache = _seed_cache(self, Xd)
        first = cache.get_device(CacheType.COQUANTILE, f"{self._start}:L2").contiguous()
        last = cache.get_device(CacheType.COQUANTILE, f"{self._end}:L2").contiguous()
        if int(Xd.shape[0]) > int(first.shape[0]):
            raise IndexError(f"index {int(first.shape[0])} is out of bounds: the cache holds the "
                             f"windows of {int(first.shape[0])} series, the batch has "
                             f"{int(Xd.shape[0])}")
        return nat.prep_mask(Xd, None, first, last)

    def _copy(self) -> "WIN":
        return WIN(self._start, self._end)

    def __eq__(self, other: Any) -> bool:
        if not isinstance(other, WIN):
            raise TypeError(f"Cannot compare WIN with type {type(other)}")
        return self._start == other._start and self._end == other._end

    def __str__(self) -> str:
        return f"WIN(start={self._start}, end={self._end})"


def _int_or_fraction(value, name: str, kinds: str) -> None:
    """An integer, or a float strictly between 0 and 1 (a fraction of the series length)."""
    if isinstance(value, float):
        if not 0 < value < 1:
            raise ValueError(f"If {name} is a float, it has to satisfy 0 < {name} < 1")
    elif not isinstance(value, int):
        raise TypeError(f"{name} has to be either {kinds}")


class DOT(_TimeMasked, _ShapeFitted):
    """Dotting: every ``n``-th point of a series is kept, the rest set to zero
    (fruits/preparation/filter.py:123-206).

    Args:
        n: the distance of the kept points; a float in (0, 1) is a fraction of the length.
        first: the first kept index (same rules); ``n - 1`` if None.
    """

    def __init__(self, n: Union[int, float] = 2,
                 first: Optional[Union[int, float]] = None) -> None:
        _int_or_fraction(n, "n", "a float or integer")
        if first is not None:
            _int_or_fraction(first, "first", "a float, integer or None")
        self._n_given = n
        self._first_given = first

    def _fit(self, X: np.ndarray) -> None:
        T = X.shape[2]
        if isinstance(self._n_given, float):
            self._n = max(int(self._n_given * T), 1)
        else:
            self._n = min(self._n_given, T)
        if self._first_given is None:
            self._first = self._n - 1
        elif isinstance(self._first_given, float):
            self._first = min(max(int(self._first_given * T), 1), T - 1)
        else:
            self._first = min(self._first_given, T - 1)

    def _check_fitted(self) -> None:
        if not hasattr(self, "_n") or not hasattr(self, "_first"):
            raise RuntimeError("Missing call of self.fit()")

    def _time_mask(self, T: int) -> np.ndarray:
        keep = np.zeros(T, dtype=bool)
        keep[self._first::self._n] = True
        return keep

    def _mask_state(self) -> tuple:
        return (int(self._first), int(self._n))

    def _transform_device(self, Xd):
        self._check_fitted()
        return self._masked_device(Xd)

    def _copy(self) -> "DOT":
        return DOT(self._n_given, self._first_given)

    def __eq__(self, other: Any) -> bool:
        if not isinstance(other, DOT):
            raise TypeError(f"Cannot compare DOT with type {type(other)}")
        return self._n_given == other._n_given and self._first_given == other._first_given

    def __str__(self) -> str:
        return f"DOT(n={self._n_given}, first={self._first_given})"


class PDD(_TimeMasked, _ShapeFitted):
    """Proportion-density-drop: evenly spread strips of every series are set to zero
    (fruits/preparation/filter.py:209-270).

    Args:
        density: a float in (0, 1]; the lower, the further apart the strips.
        proportion: the share of every series to drop, a float in (0, 1).
    """

    def __init__(self, density: float = 0.1, proportion: float = 0.5) -> None:
        if not isinstance(density, float) or not 0.0 < density <= 1.0:
            raise ValueError("density has to be a float 0 < density <= 1")
        if not isinstance(proportion, float) or not 0.0 < proportion < 1.0:
            raise ValueError("proportion has to be a float 0 < proportion < 1")
        self._d_given = density
        self._p_given = proportion

    def _fit(self, X: np.ndarray) -> None:
        T = X.shape[2]
        dropped = max(int(self._p_given * T), 1)
        strips = max(int((1.0 - self._d_given) * T), 1)
        self._width = int(dropped / strips)      # (0 for many strips: the identity)
        if strips == T - self._width:
            strips -= 1
        self._indices = np.linspace(0, T - self._width, strips, dtype="int")

    def _check_fitted(self) -> None:
        if not hasattr(self, "_width") or not hasattr(self, "_indices"):
            raise RuntimeError("Missing call of self.fit()")

    def _time_mask(self, T: int) -> np.ndarray:
        keep = np.ones(T, dtype=bool)
        for start in self._indices:
            keep[start:start + self._width] = False
        return keep

    def _mask_state(self) -> tuple:
        return (np.asarray(self._indices).tobytes(), int(self._width))

    def _transform_device(self, Xd):
        self._check_fitted()
        return self._masked_device(Xd)

    def _copy(self) -> "PDD":
        return PDD(self._d_given, self._p_given)

    def __eq__(self, other: Any) -> bool:
        if not isinstance(other, PDD):
            raise TypeError(f"Cannot compare PDD with type {type(other)}")
        return self._d_given == other._d_given and self._p_given == other._p_given

    def __str__(self) -> str:
        return f"PDD(density={self._d_given}, proportion={self._p_given})"
