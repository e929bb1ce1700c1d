"""Lowering of generic words to exponent tables over virtual input rows.

The reference sends every word that is not a ``SimpleWord`` down its slow path
(fruits/iss/semiring.py:54-75): per extended letter it multiplies the values of the letter
functions, shifts the running result by one step and accumulates.  Only the VALUES of the letter
functions enter, so a generic word is an ordinary word over other input rows:

    one virtual row per distinct (letter, dimension[, shift]) = (kind, source, shift)
      DIM  X[n, source, t + shift]            ABS  |X[n, source, t + shift]|
      EXT  ext[n, source, t + shift], the values a Python letter gave on the host
      ONE  the semiring's one (an extended letter without letters)

and one ``(L, Dv) int32`` exponent table per word over those rows.  ``fr_letter_rows`` forms the
rows, the plan compiler and the walks run unchanged on them.

Strict and non-strict sums.  The generic slow path shifts between extended letters, so the
max-times sums of Bayesian run over ``i1 < i2 < ...`` there; the device kernel of Bayesian,
like the reference's fast one, does not shift (``i1 <= i2 <= ...``).  With letter ``m`` of a
word reading its rows shifted left by ``m`` steps, ``Z'_m[j] = Z[j + m]``, the non-strict sum
``R'`` over the shifted rows is the strict one moved: ``R[t] = R'[t - (p - 1)]`` for the prefix
of length ``p`` and ``t >= p - 1``, and ``R[t] = 0`` in front (the reference leaves those
positions at exactly 0.0).  ``fr_rows_unshift`` moves the rows back.  Only ``R'[0 .. T - p]`` is
read, which never touches the padding past a row's end.  Reals needs neither: its device
recursion is strict already.  Nor does Arctic: it overrides the slow path
(fruits/iss/semiring.py:428-446) with a loop that does not shift - the non-strict recursion of
its fast kernel, which is the device's.

The weighting is ignored for generic words, as in the reference (``_iterated_sum`` never sees
it); lowered plans are unweighted.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

from .._native import FR_ROW_ABS as ROW_ABS
from .._native import FR_ROW_DIM as ROW_DIM
from .._native import FR_ROW_EXT as ROW_EXT
from .._native import FR_ROW_ONE as ROW_ONE
from .semiring import Arctic, Bayesian
from .words.word import SimpleWord

_KIND_OF = {"DIM": ROW_DIM, "ABS": ROW_ABS}


def is_generic(word) -> bool:
    return not isinstance(word, SimpleWord)


@dataclass
class Lowering:
    tables: list                  # per word: (L, Dv) int32 over the virtual rows
    rows: list                    # (kind, source, shift), deduplicated; Dv = len(rows)
    ext: list                     # EXT sources: (name, dim, registered letter), source = position
    out_shifts: np.ndarray        # int32 per emitted row
    one_is_zero: bool = False     # the semiring's one is 0.0 (max-plus)
    spec: np.ndarray = field(init=False)

    def __post_init__(self) -> None:
        self.spec = np.asarray(self.rows, dtype=np.int32).reshape(len(self.rows), 3)
        self._device: dict = {}   # device copies of spec and out_shifts, per device

    def device_tables(self, device):
        """(spec, out_shifts) as int32 tensors on ``device``: uploaded once per lowering."""
        key = str(device)
        if key not in self._device:
            from .. import _native as nat
            t = nat.torch()
            self._device[key] = (t.from_numpy(self.spec).to(device),
                                 t.from_numpy(self.out_shifts).to(device))
        return self._device[key]

    @property
    def shifted(self) -> bool:
        return bool(np.any(self.out_shifts))


def lower(words: Sequence, semiring, D: int, depths: Sequence[int] = None):
    """Lowers ``words`` (generic and simple mixed) for an input of ``D`` dimensions.
    ``depths[i]``: how many trailing prefixes of word ``i`` are emitted (1 each when omitted).
    Returns None for a list without a generic word: such a list is not lowered."""
    if not any(is_generic(w) for w in words):
        return None
    strict_by_shift = isinstance(semiring, Bayesian)
    depths = [1] * len(words) if depths is None else list(depths)
    index: dict = {}
    rows: list = []
    ext_index: dict = {}
    ext: list = []

    def column(kind: int, source: int, shift: int) -> int:
        key = (kind, source, shift)
        if key not in index:
            index[key] = len(rows)
            rows.append(key)
        return index[key]

    def dimension(dim: int) -> int:
        src = dim + D if dim < 0 else dim     # (a letter indexes X[i, :]: numpy's negative indices)
        if not 0 <= src < D:
            raise IndexError(
                f"a word references dimension {dim + 1} but the input has only {D}")
        return src

    sparse, out_shifts = [], []
    for word, depth in zip(words, depths):
        L = len(word)
        entries = []        # per extended letter: [(column, exponent)]
        if is_generic(word):
            for m, el in enumerate(word._extended_letters):
                shift = m if strict_by_shift else 0
                cols: dict = {}
                for pos, (name, dim) in enumerate(el.named()):
                    if name in _KIND_OF:
                        c = column(_KIND_OF[name], dimension(dim), shift)
                    else:
                        if (name, dim) not in ext_index:
                            ext_index[(name, dim)] = len(ext)
                            ext.append((name, dim, el.registered(pos)))
                        c = column(ROW_EXT, ext_index[(name, dim)], shift)
                    cols[c] = cols.get(c, 0) + 1
                if not cols:
                    cols[column(ROW_ONE, 0, shift)] = 1
                entries.append(sorted(cols.items()))
            out_shifts += [p - 1 if strict_by_shift else 0 for p in range(L - depth + 1, L + 1)]
        else:
            for row in word.table():
                cols = []
                for d, e in enumerate(row):
                    if e != 0:
                        cols.append((column(ROW_DIM, dimension(d), 0), int(e)))
                entries.append(cols)
            out_shifts += [0] * depth
        sparse.append(entries)

    Dv = len(rows)
    tables = []
    for entries in sparse:
        tab = np.zeros((len(entries), Dv), dtype=np.int32)
        for k, cols in enumerate(entries):
            for c, e in cols:
                tab[k, c] += e
        tables.append(tab)
    return Lowering(tables, rows, ext, np.asarray(out_shifts, dtype=np.int32),
                    one_is_zero=isinstance(semiring, Arctic))


def letter_values(low: Lowering, Z: np.ndarray) -> np.ndarray:
    """``(N, H, T)`` values of the lowering's Python letters on the host batch ``Z (N, D, T)``:
    ``letter(Z[i])`` per series and distinct (letter, dimension), exactly as the reference calls
    it (fruits/iss/semiring.py:61-66).  Every call has to give ``(T,)`` numbers."""
    N, _, T = Z.shape
    out = np.empty((N, len(low.ext), T), dtype=np.float64)
    for h, (name, dim, registered) in enumerate(low.ext):
        bound = registered(dim)
        for i in range(N):
            try:
                vals = np.asarray(bound(Z[i]), dtype=np.float64)
            except (TypeError, ValueError) as err:
                raise TypeError(f"letter {name!r} did not return numbers: {err}") from err
            if vals.shape != (T,):
                raise ValueError(f"letter {name!r} returned an array of shape {vals.shape}; "
                                 f"a letter has to return one value per time step, ({T},)")
            out[i, h] = vals
    return out
