"""Sieve wrappers (mirrors INC / INT of fruits/sieving/wrapper.py): the wrapped sieve is fitted
and evaluated on the increments, or on the cumulative sums, of the iterated sum.  The rows are
formed on the device and handed to the inner sieve's ``transform_device``; a wrapper that only
raises or lowers the differencing order of a band sieve is that sieve at the other order
(``_reduced``) and takes part in the fused launch.

``fruits_amd.preparation.INC`` is another class: a preparateur."""
from __future__ import annotations

import numpy as np

from .. import _native as nat
from ..cache import SharedSeedCache
from .abstract import FeatureSieve
from .increment import _cumsum_plan

__all__ = ["INC", "INT"]


class _SieveWrapper(FeatureSieve):
    _sieve: FeatureSieve

    @property
    def requires_fitting(self) -> bool:
        return self._sieve.requires_fitting

    def _nfeatures(self) -> int:
        return self._sieve.nfeatures()

    def _pre_transform_device(self, Ad):
        raise NotImplementedError

    def _inner_on(self, Yd, fn):
        """Runs ``fn`` with the inner sieve attached to a cache over the rows ``Yd`` it sees: the
        reference's fruit hands its cache to the wrapper only, so a float cut of the inner sieve
        is a coquantile of the rows the wrapper made (fruits/seed.py:41-51)."""
        inner = self._sieve
        own = not hasattr(inner, "_cache")
        if own:
            inner._cache = SharedSeedCache()
            inner._cache.adopt_device_input(Yd.unsqueeze(1).contiguous())
        try:
            return fn()
        finally:
            if own:
                del inner._cache

    def _supports_lengths(self) -> bool:
        # (where the wrapper is its inner sieve at another differencing order - INC(NPI),
        # INC(MAX, depth=0), INT(NPI(inc=-1)), INT(MAX) run fused and materialising, over every
        # preparateur, semiring and weighting of the gate's list, in tests/test_lengths_batch_gpu.py.
        # The rows it forms otherwise - a shift > 1, sums of increments - are causal too, but no
        # test runs them with lengths, so they stay outside.)
        return self._reduced() is not None and self._sieve._supports_lengths()

    def transform_device(self, Ad, out, col: int, lengths=None):
        """Writes the inner sieve's features of the pre-transformed (N, T) device array ``Ad``
        into columns [col, col + nfeatures) of the (N, F) device tensor ``out``."""
        Yd = self._pre_transform_device(Ad)
        if lengths is None:
            self._inner_on(Yd, lambda: self._sieve.transform_device(Yd, out, col))
        else:
            self._inner_on(Yd, lambda: self._sieve.transform_device(Yd, out, col, lengths=lengths))

    def _checked(self, X: np.ndarray):
        if not isinstance(X, np.ndarray) or X.dtype != np.float64 or X.ndim != 2:
            raise TypeError("input has to be a float64 array of shape (N, T)")
        return nat.to_device(X)

    def _fit(self, X: np.ndarray) -> None:
        Yd = self._pre_transform_device(self._checked(X))
        if self._sieve.requires_fitting:
            self._inner_on(Yd, lambda: self._sieve.fit(nat.to_host(Yd)))

    def _fit_valid(self, X: np.ndarray, lengths) -> None:
        Yd = self._pre_transform_device(self._checked(X))
        if self._sieve.requires_fitting:
            self._sieve._fit_valid(nat.to_host(Yd), lengths)

    def _transform(self, X: np.ndarray) -> np.ndarray:
        t = nat.torch()
        Ad = self._checked(X)
        out = t.zeros((X.shape[0], self.nfeatures()), dtype=t.float64, device=Ad.device)
        self.transform_device(Ad, out, 0)
        return nat.to_host(out)

    def _summary(self) -> str:
        return f"{self.__class__.__name__}>{self._sieve.summary()}"

    def _label(self, index: int) -> str:
        return f"{self.__class__.__name__} of {self._sieve._label(index)}"

    def _shifted(self, step: int):
        """The inner sieve's reduced form ``step`` differencing orders further on, None when the
        wrapped rows are not exactly the rows of that order."""
        inner = self._sieve._reduced() if hasattr(self._sieve, "_reduced") else None
        if inner is None:
            return None
        leaf, kind, order, fit_order = inner
        # END reads values, LPI is not fused; the inner sieve's float cuts are coquantiles of the
        # wrapped rows, which no fused launch forms
        # (no wrappers around PPV / CPV either: such a slice materialises)
        if kind in (nat.FR_SIEVE_END, nat.FR_SIEVE_LPI, nat.FR_SIEVE_PPV, nat.FR_SIEVE_CPV) \
                or leaf._has_float_cuts():
            return None
        # increments of increments and sums of sums compose exactly; cumulating increments (or
        # the other way round) is not the identity in floating point
        if step * order < 0 or step * fit_order < 0:
            return None
        if not -8 <= order + step <= 8:
            return None
        return leaf, kind, order + step, fit_order + step


class INC(_SieveWrapper):
    """Evaluates ``sieve`` on the increments ``X[t] - X[t - shift]`` (zero-padded) of its input
    (fruits/sieving/wrapper.py:9-64).  Like the reference, which restarts from the input in
    every round of its loop, any ``depth >= 1`` is one application; ``depth = 0`` hands the
    input itself to the sieve."""

    def __init__(self, sieve: FeatureSieve, depth: int = 1, shift: int = 1) -> None:
        self._sieve = sieve
        self._shift = shift
        self._depth = depth

    def _pre_transform_device(self, Ad):
        if self._depth < 1:
            return Ad
        if not isinstance(self._shift, (int, np.integer)) or self._shift < 1:
            raise ValueError("shift has to be a positive integer")
        if self._shift == 1:
            return nat.pre_transform(Ad, 1)
        return nat.increments(Ad.contiguous().unsqueeze(1), int(self._shift))[:, 0, :]

    def _reduced(self):
        if self._depth < 1:
            return self._shifted(0)
        return self._shifted(1) if self._shift == 1 else None

    def _copy(self) -> "INC":
        return INC(self._sieve.copy(), depth=self._depth, shift=self._shift)

    def __str__(self) -> str:
        return f"INC({self._sieve}, {self._depth}, {self._shift})"


class INT(_SieveWrapper):
    """Evaluates ``sieve`` on the cumulative sums (np.cumsum along time) of its input
    (fruits/sieving/wrapper.py:67-104)."""

    def __init__(self, sieve: FeatureSieve) -> None:
        self._sieve = sieve

    def _pre_transform_device(self, Ad):
        return _cumsum_plan().run(Ad.unsqueeze(1).contiguous(), None, layout="KNT")[0]

    def _reduced(self):
        return self._shifted(-1)

    def _copy(self) -> "INT":
        return INT(self._sieve.copy())

    def __str__(self) -> str:
        return f"INT({self._sieve})"
