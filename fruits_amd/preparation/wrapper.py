"""Wrapping preparateurs (mirrors DIM and NEW of fruits/preparation/wrapper.py:11-103)."""
from __future__ import annotations

from collections.abc import Sequence
from typing import Optional, Union

import numpy as np

from .. import _native as nat
from ..lengths import with_lengths
from .abstract import Preparateur

__all__ = ["DIM", "NEW"]


class DIM(Preparateur):
    """Runs another preparateur on the given dimension(s) only; its results are appended behind
    the remaining dimensions, so the dimensions may get reordered
    (fruits/preparation/wrapper.py:11-50)."""

    def __init__(self, preparateur: Preparateur, dim: Union[int, Sequence[int]]) -> None:
        self._preparateur = preparateur
        self._dim = np.array([dim]) if isinstance(dim, int) else np.array(dim)

    @property
    def requires_fitting(self) -> bool:
        return self._preparateur.requires_fitting

    def _fit_needs_data(self) -> bool:
        return self._preparateur._fit_needs_data()

    def _fit_needs_shape(self) -> bool:
        return self._preparateur._fit_needs_shape()

    def _fit(self, X: np.ndarray) -> None:
        if self._preparateur._fit_needs_data():
            sub = X[:, self._dim, :]
        else:     # (a fit that reads the shape alone: no gather of a stand-in's zeros)
            k = int(np.arange(X.shape[1])[self._dim].size)
            sub = np.broadcast_to(0.0, (X.shape[0], k, X.shape[2]))
        self._preparateur.fit(sub)

    def _check_fitted(self) -> None:
        self._preparateur._check_fitted()

    def _supports_lengths(self) -> bool:
        return self._preparateur._supports_lengths()

    def _transform_device(self, Xd, lengths_d=None):
        t = nat.torch()
        D = int(Xd.shape[1])
        dim = np.arange(D)[self._dim]      # (numpy's index rules: negative entries, range errors)
        idx = nat.to_device(np.ascontiguousarray(dim, dtype=np.int64), dtype=np.int64)
        sub = t.index_select(Xd, 1, idx).contiguous()
        transformed = with_lengths(self._preparateur._transform_device, sub, lengths_d=lengths_d)
        rest = np.delete(np.arange(D), self._dim)
        if rest.size == 0:
            return transformed
        keep = nat.to_device(np.ascontiguousarray(rest, dtype=np.int64), dtype=np.int64)
        return t.cat((t.index_select(Xd, 1, keep), transformed), dim=1).contiguous()

    def _copy(self) -> "DIM":
        return DIM(self._preparateur.copy(), tuple(self._dim))

    def __str__(self) -> str:
        # tuple() of a numpy array: numpy scalars, whose repr depends on the numpy version
        # ((np.int64(0),) under numpy 2) - the reference prints the same (wrapper.py:50)
        return f"DIM({str(self._preparateur)}, {tuple(self._dim)})"


class NEW(Preparateur):
    """Appends the output of another preparateur as new dimensions; with no
    preparateur given the input dimensions are duplicated."""

    def __init__(self, preparateur: Optional[Preparateur] = None) -> None:
        self._preparateur = preparateur

    @property
    def requires_fitting(self) -> bool:
        return False if self._preparateur is None else self._preparateur.requires_fitting

    def _fit_needs_data(self) -> bool:
        return self._preparateur is not None and self._preparateur._fit_needs_data()

    def _fit_needs_shape(self) -> bool:
        return self._preparateur is not None and self._preparateur._fit_needs_shape()

    def _fit(self, X: np.ndarray) -> None:
        if self._preparateur is not None:
            self._preparateur.fit(X)

    def _check_fitted(self) -> None:
        if self._preparateur is not None:
            self._preparateur._check_fitted()

    def _supports_lengths(self) -> bool:
        return self._preparateur is None or self._preparateur._supports_lengths()

    def _transform_device(self, Xd, lengths_d=None):
        t = nat.torch()
        extra = Xd if self._preparateur is None else with_lengths(
            self._preparateur._transform_device, Xd, lengths_d=lengths_d)
        return t.cat((Xd, extra), dim=1).contiguous()

    def _copy(self) -> "NEW":
        return NEW() if self._preparateur is None else NEW(self._preparateur.copy())

    def __str__(self) -> str:
        return f"NEW({str(self._preparateur)})"
