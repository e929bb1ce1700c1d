"""Implicit sieves (mirrors PPV / CPV of fruits/sieving/implicit.py): the share of the values of
an iterated sum at or above a threshold - or inside ``q_{j-1} <= x < q_j`` with ``segments`` -
and the number of connected components of that indicator.  The thresholds are given values or
quantiles that ``fit`` takes of a random subset of the fit sample's rows.  The counting is the
HIP kernel ``fr_sieve_implicit``: one pass over a row for all thresholds of the sieve.

The tests are closed BELOW (every band of the other sieves is ``q_lo < x <= q_hi``), and the
fitted thresholds stay in the order of the constructor's pairs: with ``segments`` a band whose
lower threshold came out above its upper one is empty, as in the reference.
"""
from __future__ import annotations

from typing import Union

import numpy as np

from .. import _native as nat
from .abstract import FeatureSieve

__all__ = ["PPV", "CPV"]


class PPV(FeatureSieve):
    """Proportion of the values ``>= q_j`` (``segments``: inside ``q_{j-1} <= x < q_j``) of every
    series (fruits/sieving/implicit.py:11-153).

    ``quantile``: value(s) or probabilities; ``constant`` (one boolean, or one per entry) says
    which.  ``segments=True`` pairs ``list(set(quantile))`` with ``constant`` BY POSITION and then
    sorts the pairs by quantile (implicit.py:79-81) - the same expression here, so that both give
    the same pairs on the same interpreter.
    """
    _kind = nat.FR_SIEVE_PPV

    def __init__(
        self,
        quantile: Union[list[float], float] = 0.5,
        constant: Union[list[bool], bool] = False,
        sample_size: float = 1.0,
        segments: bool = False,
    ) -> None:
        if isinstance(quantile, list):
            if not isinstance(constant, list):
                constant = [constant for _ in range(len(quantile))]
            elif len(quantile) != len(constant):
                raise ValueError("If 'quantile' is a list, then 'constant' "
                                 + "also has to be a list of same length or "
                                 + "a single boolean.")
            for q, c in zip(quantile, constant):
                if not c and not 0 <= q <= 1:
                    raise ValueError("If 'constant' is set to False, "
                                     + "'quantile' has to be a value in [0,1]")
        else:
            quantile = [quantile]
            if isinstance(constant, list):
                if len(constant) > 1:
                    raise ValueError("'constant' has to be a single boolean"
                                     + "if 'quantile' is a single float")
            else:
                constant = [constant]
        if segments:
            self._q_c_input = list(zip(list(set(quantile)), constant))
            self._q_c_input = sorted(self._q_c_input, key=lambda x: x[0])
        else:
            self._q_c_input = list(zip(quantile, constant))
        self._q: list[float]
        if not 0 < sample_size <= 1:
            raise ValueError("'sample_size' has to be a float in (0, 1]")
        self._sample_size = sample_size
        if segments and len(quantile) == 1:
            raise ValueError("If 'segments' is set to `True` then 'quantile'"
                             + "has to be a list of length >= 2.")
        self._segments = segments

    def _nfeatures(self) -> int:
        if self._segments:
            return len(self._q_c_input) - 1
        return len(self._q_c_input)

    def _fit(self, X: np.ndarray) -> None:
        # implicit.py:99-112: one draw from numpy's global generator per non-constant
        # threshold, in order; np.quantile of the chosen rows, flattened
        self._q = [x[0] for x in self._q_c_input]
        for i, q in enumerate(self._q):
            if not self._q_c_input[i][1]:
                sample_size = max(int(self._sample_size * len(X)), 1)
                selection = np.random.choice(
                    np.arange(len(X)),
                    size=sample_size,
                    replace=False,
                )
                self._q[i] = np.quantile(X[selection].flatten(), q)

    # ---- what the fused pipeline and the device-side fit are told (fruit.py) ----------------
    # (``_q`` holds the fitted THRESHOLDS here, as in the reference, where a segment sieve's
    # ``_q`` holds probabilities and ``_quantiles`` the thresholds: ``_quantiles`` is this sieve's
    # ``_q`` under the name fruit.py reads and sets on the fitted copies)
    def _reduced(self):
        """(this sieve, its FR_SIEVE_* kind, differencing order 0 of the transform, of the fit)."""
        return self, self._kind, 0, 0

    @property
    def _quantiles(self) -> np.ndarray:
        if not hasattr(self, "_q"):
            raise AttributeError("_quantiles")
        return np.asarray(self._q, dtype=np.float64)

    @_quantiles.setter
    def _quantiles(self, values) -> None:
        self._q = [float(v) for v in values]
        self.__dict__.pop("_q_dev", None)

    def _n_thresholds(self) -> int:
        return len(self._q_c_input)

    def _quantile_requests(self, n: int):
        """[(index of the threshold, lower rank, upper rank, gamma)] for the thresholds ``fit``
        takes of the data, as np.quantile(method="linear") places them among ``n`` values
        (SegmentSieve._quantile_requests; here 0 and 1 are plain probabilities)."""
        reqs = []
        for i, (q, constant) in enumerate(self._q_c_input):
            if constant:
                continue
            pos = (n - 1) * q
            lo = int(np.floor(pos))
            gamma = pos - lo
            if pos >= n - 1:
                lo = hi = n - 1
            else:
                hi = lo + 1
            reqs.append((i, lo, hi, gamma))
        return reqs

    def _thresholds_from_stats(self, reqs, lo_vals: np.ndarray, hi_vals: np.ndarray) -> np.ndarray:
        """(rows, thresholds) table of the fitted thresholds of many copies at once from the
        (rows, len(reqs)) order statistics np.quantile interpolates between - in the order of
        the constructor's pairs, NOT sorted (implicit.py:99-112)."""
        qs = np.empty((lo_vals.shape[0], len(self._q_c_input)))
        qs[:] = [float(x[0]) for x in self._q_c_input]
        for j, (i, _, _, gamma) in enumerate(reqs):
            # numpy's _lerp: a + (b-a)*t, from the other end when t >= 0.5
            a, b = lo_vals[:, j], hi_vals[:, j]
            d = b - a
            qs[:, i] = a + d * gamma if gamma < 0.5 else b - d * (1 - gamma)
        return qs

    def _fit_draws(self, n_series: int) -> None:
        """The draws ``_fit`` makes from numpy's global generator on ``n_series`` rows, without
        the fit (the device-side fit selects the order statistics itself)."""
        for _, constant in self._q_c_input:
            if not constant:
                np.random.choice(np.arange(n_series),
                                 size=max(int(self._sample_size * n_series), 1), replace=False)

    def thresholds_device(self):
        """The fitted thresholds on the device: uploaded once per fit of this copy (the
        materialising path transforms with one copy per iterated sum, call after call)."""
        if not hasattr(self, "_q"):
            raise RuntimeError(f"Missing call of {self.__class__.__name__}.fit()")
        held = self.__dict__.get("_q_dev")
        if held is None or held[0] != self._q:
            held = (list(self._q), nat.to_device(np.asarray(self._q, dtype=np.float64)))
            self._q_dev = held
        return held[1]

    def __getstate__(self):
        # (the device tensor is the process's, like the cache: Seed._TRANSIENT)
        return {k: v for k, v in super().__getstate__().items() if k != "_q_dev"}

    def _supports_lengths(self) -> bool:
        return True

    def transform_device(self, Ad, out, col: int, lengths=None):
        """Writes this sieve's features of the (N, T) device array ``Ad`` into columns
        [col, col + nfeatures) of the (N, F) device tensor ``out``.  ``lengths``: host array
        (N,), series n is its first ``lengths[n]`` elements (fr_sieve_implicit_lengths)."""
        lengths_d = None if lengths is None else nat.to_device(
            np.ascontiguousarray(lengths, dtype=np.int32), dtype=np.int32)
        nat.sieve_implicit(self._kind, Ad, self.thresholds_device(), self._segments, out, col,
                           lengths_d=lengths_d)

    def _transform(self, X: np.ndarray) -> np.ndarray:
        if not hasattr(self, "_q"):
            raise RuntimeError(f"Missing call of {self.__class__.__name__}.fit()")
        if not isinstance(X, np.ndarray) or X.dtype != np.float64 or X.ndim != 2:
            raise TypeError("input has to be a float64 array of shape (N, T)")
        t = nat.torch()
        Ad = nat.to_device(X)
        out = t.zeros((X.shape[0], self.nfeatures()), dtype=t.float64, device=Ad.device)
        self.transform_device(Ad, out, 0)
        return nat.to_host(out)

    def _copy(self):
        return self.__class__(
            quantile=[x[0] for x in self._q_c_input],
            constant=[x[1] for x in self._q_c_input],
            sample_size=self._sample_size,
            segments=self._segments,
        )

    def _summary(self) -> str:
        string = f"{self.__class__.__name__} [sampling={self._sample_size}"
        if self._segments:
            string += ", segments"
        string += f"] -> {self.nfeatures()}:"
        for x in self._q_c_input:
            string += f"\n   > {x[0]} | {x[1]}"
        return string

    def __str__(self) -> str:
        return (f"{self.__class__.__name__}("
                f"quantile={[x[0] for x in self._q_c_input]}, "
                f"constant={[x[1] for x in self._q_c_input]}, "
                f"sample_size={self._sample_size}, "
                f"segments={self._segments})")


class CPV(PPV):
    """Connected components of the values ``>= q_j`` (``segments``: inside the band) of every
    series: twice the number of rising edges of the indicator at ``t >= 1`` over the series
    length rounded up to even (fruits/sieving/implicit.py:156-213).  A component that starts at
    ``t = 0`` is not counted - the reference's first difference is zero-padded there."""
    _kind = nat.FR_SIEVE_CPV
