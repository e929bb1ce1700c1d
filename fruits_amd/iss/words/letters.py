"""Letters and extended letters of generic words (the API of fruits/iss/words/letters.py).

A letter is a function ``(X, i) -> (T,)`` of one series ``X (D, T)`` and a dimension index,
registered under a name with the :func:`letter` decorator.  The predefined ``DIM`` and ``ABS``
are formed on the device (``fr_letter_rows``); every other name is a Python callable whose
VALUES are computed on the host and uploaded as extra input rows - the callable itself never
crosses the C ABI (fruits_amd/iss/lowering.py).

One registry maps a name to a :class:`_Registered` letter; an :class:`ExtendedLetter` is a list
of ``(registered letter, dimension)`` pairs, which is also what the lowering reads.
"""
from __future__ import annotations

import functools
import re
from typing import Callable, Iterator, Optional

import numpy as np

__all__ = ["ExtendedLetter", "get_available", "letter"]

_PIECE = re.compile(r"([^()]+)\((-?\d+)\)")     # "ABS(1)": a name and a 1-based dimension


class _Registered:
    """A named letter ``fn(X, i)``.  Calling it with a dimension binds that dimension - the
    decorated name is used like the reference's: ``ReLU(0)(X)``."""

    def __init__(self, name: str, fn: Callable) -> None:
        self.name = name
        self.fn = fn
        functools.update_wrapper(self, fn)

    def __call__(self, dim: int) -> Callable[[np.ndarray], np.ndarray]:
        return functools.partial(self._evaluate, dim)

    def _evaluate(self, dim: int, X: np.ndarray) -> np.ndarray:
        return self.fn(X, dim)


_REGISTRY: dict[str, _Registered] = {}


def _register(name: str, fn: Callable) -> _Registered:
    if name in _REGISTRY:
        raise RuntimeError(f"Letter with name '{name}' already exists")
    entry = _REGISTRY[name] = _Registered(name, fn)
    return entry


def _registered(name: str) -> _Registered:
    try:
        return _REGISTRY[name]
    except KeyError:
        raise RuntimeError(f"Letter with name '{name}' does not exist") from None


_register("DIM", lambda X, i: X[i, :])
_register("ABS", lambda X, i: np.abs(X[i, :]))


def get_available() -> list[str]:
    """Names usable in an :class:`ExtendedLetter`, in the order they were registered."""
    return list(_REGISTRY)


def letter(*args, name: Optional[str] = None):
    """Decorator that registers ``func(X, i) -> (T,)`` as a letter, under the function's name
    (``@letter``) or a given one (``@letter(name="ReLU")``); names are unique."""
    if len(args) > 1:
        raise RuntimeError("Too many arguments")
    if name is not None:
        return functools.partial(_register, name)
    if args and callable(args[0]):
        return _register(args[0].__name__, args[0])
    raise ValueError("Please either specify the 'name' argument or use this "
                     "decorator without calling it.")


class ExtendedLetter:
    """``ExtendedLetter("ABS(1)DIM(2)")``: a product of named letters, each with a dimension -
    1-based in the string form, 0-based in ``append``.  Iterating or indexing yields the bound
    letter functions ``X (D, T) -> (T,)``."""

    def __init__(self, letter_string: str = "") -> None:
        self._pairs: list[tuple[_Registered, int]] = []
        for name, dim in _PIECE.findall(letter_string):
            self.append(name, int(dim) - 1)

    def append(self, letter: str, dim: int = 0) -> None:
        self._pairs.append((_registered(letter), dim))

    def copy(self) -> "ExtendedLetter":
        dup = ExtendedLetter()
        dup._pairs = list(self._pairs)
        return dup

    def named(self) -> list[tuple[str, int]]:
        """``(name, dim)`` of every letter."""
        return [(entry.name, dim) for entry, dim in self._pairs]

    def registered(self, i: int) -> _Registered:
        """The registered (unbound) letter at position ``i``."""
        return self._pairs[i][0]

    def __len__(self) -> int:
        return len(self._pairs)

    def __getitem__(self, i: int) -> Callable[[np.ndarray], np.ndarray]:
        entry, dim = self._pairs[i]
        return entry(dim)

    def __iter__(self) -> Iterator[Callable[[np.ndarray], np.ndarray]]:
        return iter([entry(dim) for entry, dim in self._pairs])

    def __str__(self) -> str:
        return "[" + "".join(f"{entry.name}({dim + 1})" for entry, dim in self._pairs) + "]"
