"""The ISS stage (mirrors fruits/iss/iss.py).

``ISS(words, mode=..., semiring=..., weighting=...)`` computes the iterated sums
``(K, N, T)`` of a batch ``(N, D, T)``.  Where the reference loops over the words
in Python and calls one numba kernel per word (fruits/iss/iss.py:49-65), this
stage compiles the whole word list into ONE device program (a prefix trie in DFS
order, csrc/plan.cpp) and walks it in one HIP launch; the result has the
reference's row order and layout (iss.py:46).

Generic words - ``Word``s of named letter functions, which the reference sends down its slow
path (fruits/iss/semiring.py:54-75) - run through the same program: ``lowering.py`` rewrites
them as exponent tables over virtual input rows, ``fr_letter_rows`` forms those rows.  ``DIM``
and ``ABS`` letters are formed on the device; any other letter is a Python callable, so its
values are computed on the host - the batch is downloaded once, ``letter(Z[i])`` is evaluated
per series and distinct (letter, dimension), the values are uploaded: the same round trip as
the ``FUN`` preparateur.  The weighting is ignored for generic words, as in the reference.
"""
from __future__ import annotations

import os
from enum import Enum, auto
from typing import Generator, Optional, Sequence

import numpy as np

from .. import _native as nat
from ..cache import SharedSeedCache
from ..lengths import lookup_rows
from ..seed import Seed
from . import lowering
from .cache import CachePlan
from .semiring import Arctic, Bayesian, Reals, Semiring

_AUTO_PREPARE_BYTES = 64 << 20   # materialised output from which a plan is prepared unasked
from .weighting import Weighting
from .words.word import Word


class ISSMode(Enum):
    """SINGLE: one iterated sum per word.  EXTENDED: additionally every prefix
    of every word that no earlier word already produced."""

    SINGLE = auto()
    EXTENDED = auto()


def _device_budget_bytes() -> int:
    return int(float(os.environ.get("FRUITS_AMD_ISS_GIB", "8")) * (1 << 30))


class ISS(Seed):
    def __init__(self, words: Sequence[Word], /, *, mode: ISSMode = ISSMode.SINGLE,
                 semiring: Optional[Semiring] = None,
                 weighting: Optional[Weighting] = None) -> None:
        self.words = words
        self.mode = mode
        self.semiring = semiring if semiring is not None else Reals()
        self._cache_plan = CachePlan(self.words if mode == ISSMode.EXTENDED else [])
        self.weighting = weighting
        self._generic: Optional[bool] = None
        self._fresh_transients()

    def _fresh_transients(self) -> None:
        self._plans: dict = {}      # device programs by (words, mode, weighting)

    @property
    def requires_fitting(self) -> bool:
        return False

    def _fit(self, X: np.ndarray) -> None:
        pass

    # ------------------------------------------------------------------ plans
    @property
    def _argmax(self) -> bool:
        return isinstance(self.semiring, Arctic) and self.semiring._argmax

    def _depth(self, i: int) -> int:
        """Rows word i contributes (EXTENDED: CachePlan's depth; Arctic argmax: every prefix
        with the positions of its maxima, L + L(L+1)/2 rows - fruits/iss/iss.py:37-47)."""
        if self._argmax:
            L = len(self.words[i])
            return L + L * (L + 1) // 2
        return self._cache_plan.unique_el_depth(i) if self.mode == ISSMode.EXTENDED else 1

    def _rows_of(self, start: int, stop: int) -> int:
        return sum(self._depth(i) for i in range(start, stop))

    def _check_supported(self) -> None:
        if self._argmax and self.mode == ISSMode.SINGLE:
            raise NotImplementedError(
                "Arctic argmax is not implemented when using ISSMode.SINGLE")
        if isinstance(self.semiring, Arctic):
            pass
        elif not isinstance(self.semiring, (Reals, Bayesian)):
            raise NotImplementedError(
                f"semiring {type(self.semiring).__name__} is not on the MI355X hot path")
        for w in self.words:
            if not isinstance(w, Word):
                raise TypeError(f"an ISS takes words, not {type(w).__name__}")
        if self._argmax and self._has_generic:
            # the reference's slow path returns one row per prefix, which its argmax layout of
            # L + L(L+1)/2 rows per word cannot take (fruits/iss/iss.py:37-65): it fails there too
            raise NotImplementedError(
                "Arctic(argmax=True) is defined for SimpleWord only: the reference's slow path "
                "for generic words returns no positions of the maxima")

    @property
    def _has_generic(self) -> bool:
        # (decided once, like the cache plan: a word list of simple words pays nothing per call)
        if getattr(self, "_generic", None) is None:
            self._generic = any(lowering.is_generic(w) for w in self.words)
        return self._generic

    def _generic_in(self, indices) -> bool:
        return any(lowering.is_generic(self.words[i]) for i in indices)

    def _plan(self, start: int, stop: int) -> nat.Plan:
        return self._plan_indices(tuple(range(start, stop)))

    def _lowered(self, indices, D: int):
        """(lowering, device program) of a subset that holds generic words, for inputs of ``D``
        dimensions: the words as exponent tables over virtual rows (lowering.py), compiled like
        any other plan.  Lowered plans are unweighted - the reference ignores the weighting for
        generic words (fruits/iss/semiring.py:40) - so a weighted ISS lowers subsets of generic
        words only (``_class_runs``)."""
        indices = tuple(indices)
        arctic = isinstance(self.semiring, Arctic)
        bayesian = isinstance(self.semiring, Bayesian)
        # The lowering and its plan are kept together, found by what the row specification is a
        # function of: the words (their strings name every letter and dimension), the semiring
        # and D.  The entry itself holds the row specification (and its device copy).
        key = ("lowered", indices, self.mode, arctic, bayesian, int(D),
               tuple(str(self.words[i]) for i in indices))
        entry = self._plans.get(key)
        if entry is None:
            depths = [self._depth(i) for i in indices]
            low = lowering.lower([self.words[i] for i in indices], self.semiring, int(D), depths)
            plan = nat.Plan(low.tables, depths, None, nat.FR_W_NONE, arctic=arctic,
                            bayesian=bayesian)
            entry = self._plans[key] = (low, plan)
        return entry

    def _class_runs(self, indices):
        """``indices`` cut into maximal runs of words of one class (generic / simple).  A
        weighted ISS runs them as separate plans into slices of one output: the simple words
        weighted on the input itself, exactly as without generic neighbours, the generic ones
        unweighted on their virtual rows.  (The alternative, one plan with ``alpha = 0`` for
        the generic words, stages the exp tables of the simple words next to the virtual rows
        of the generic ones: two smaller plans fit a workgroup's LDS more often.)"""
        runs = []
        for i in indices:
            g = lowering.is_generic(self.words[i])
            if runs and runs[-1][0] == g:
                runs[-1][1].append(i)
            else:
                runs.append((g, [i]))
        return [tuple(r) for _, r in runs]

    def needs_unshift(self) -> bool:
        """Whether rows of this ISS come out of the walk time-shifted (generic words under
        Bayesian): such an ISS materialises, it cannot feed fused sieves."""
        return self._has_generic and isinstance(self.semiring, Bayesian)

    def virtual_rows(self, Xd, low, host=None):
        """The ``(N, Dv, T)`` input of a lowered plan (fr_letter_rows).  Letters other than DIM
        and ABS are Python callables: the batch is downloaded ONCE (``host``: a list that keeps
        the copy for the other plans of the same call), ``letter(Z[i])`` is evaluated per series
        and distinct (letter, dimension) on the host, and the values are uploaded - the same
        documented round trip as FUN."""
        ext_d = None
        if low.ext:
            host = [] if host is None else host
            if not host:
                host.append(nat.to_host(Xd))
            ext_d = nat.to_device(lowering.letter_values(low, host[0]))
        return nat.letter_rows(Xd, low.spec, ext_d, one_is_zero=low.one_is_zero,
                               spec_d=low.device_tables(Xd.device)[0])

    def _transform_lowered(self, Xd, indices, lookup_d, out, groups: int, host=None):
        t = nat.torch()
        N, D, T = (int(v) for v in Xd.shape)
        K = sum(self._depth(i) for i in indices)
        if out is None:
            out = t.empty((K, N, T), dtype=t.float64, device=Xd.device)
        runs = self._class_runs(indices)
        if self.weighting is not None and len(runs) > 1:
            host = [] if host is None else host
            k0 = 0
            for run in runs:
                k1 = k0 + sum(self._depth(i) for i in run)
                if self._generic_in(run):
                    self._transform_lowered(Xd, run, lookup_d, out[k0:k1], groups, host)
                else:
                    self.transform_device(Xd, lookup_d=lookup_d, out=out[k0:k1], groups=groups,
                                          indices=run)
                k0 = k1
            return out
        low, plan = self._lowered(indices, D)
        if not plan.fits(T):
            if len(indices) == 1:
                raise NotImplementedError(
                    f"word {self.words[indices[0]]} alone needs {plan.staged_rows} staged rows: "
                    "more than the LDS of a workgroup holds")
            host = [] if host is None else host
            half = len(indices) // 2
            k0 = sum(self._depth(i) for i in indices[:half])
            for part, dst in ((indices[:half], out[:k0]), (indices[half:], out[k0:])):
                if self._generic_in(part):
                    self._transform_lowered(Xd, part, lookup_d, dst, groups, host)
                else:
                    self.transform_device(Xd, lookup_d=lookup_d, out=dst, groups=groups,
                                          indices=part)
            return out
        V = self.virtual_rows(Xd, low, host)
        if not low.shifted:
            return plan.run(V, None, out=out, layout="KNT", groups=groups)
        return nat.rows_unshift(plan.run(V, None, layout="KNT", groups=groups), low.out_shifts,
                                out=out, shifts_d=low.device_tables(Xd.device)[1])

    def _plan_indices(self, indices, D: Optional[int] = None) -> nat.Plan:
        """Device program of an arbitrary subset of the words (in the given
        order).  Output depths come from the cache plan of the FULL word list, so
        shards of a word list (fruits_amd.parallel) emit exactly their share of
        the rows.  A subset that holds generic words is lowered for inputs of ``D``
        dimensions (``_lowered``)."""
        indices = tuple(indices)
        if self._has_generic and self._generic_in(indices):
            if D is None:
                raise ValueError("the plan of generic words depends on the input's dimensions")
            return self._lowered(indices, D)[1]
        if self.weighting is None:
            wmode, alphas = nat.FR_W_NONE, None
        else:
            # (the argmax body weights like the non-total one whatever `total` says,
            # fruits/iss/semiring.py:262-263,271-272)
            wmode = (nat.FR_W_TOTAL if self.weighting.total and not self._argmax
                     else nat.FR_W_NONTOTAL)
            alphas = [np.asarray(self.words[i].alpha, dtype=np.float32) for i in indices]
        arctic = isinstance(self.semiring, Arctic)
        bayesian = isinstance(self.semiring, Bayesian)
        key = (indices, self.mode, wmode, arctic, bayesian,
               None if alphas is None else tuple(a.tobytes() for a in alphas))
        plan = self._plans.get(key)
        if plan is None:
            # argmax: the running maxima of ALL prefixes of every word (depth = its length)
            depths = ([len(self.words[i]) for i in indices] if self._argmax
                      else [self._depth(i) for i in indices])
            plan = nat.Plan([self.words[i].table() for i in indices], depths, alphas, wmode,
                            arctic=arctic, bayesian=bayesian, letter_sum=self._argmax)
            self._plans[key] = plan
        return plan

    # ------------------------------------------------------------------ device path
    def _attach_cache(self, X) -> None:
        if self.weighting is None:
            return
        if hasattr(self, "_cache"):
            self.weighting._cache = self._cache
        else:
            self.weighting._cache = SharedSeedCache(X)

    def _supports_lengths(self) -> bool:
        """Per-series lengths: simple words over Reals, Arctic (without argmax) or Bayesian,
        unweighted or with a weighting whose row is a function of the series length (Indices,
        Plateaus - one row per distinct length, lengths.lookup_rows).  A subclass says for
        itself."""
        if type(self) is not ISS or self._argmax or self._has_generic:
            return False
        if not isinstance(self.semiring, (Reals, Arctic, Bayesian)):
            return False
        return self.weighting is None or self.weighting._supports_lengths()

    def lookup_device(self, Xd, lengths=None):
        """(rows, T) device lookup of the weighting, rows in {1, N}; when the
        cache holds more series than Xd (fit on a sub-sample) the leading rows
        are used - the reference indexes ``lookup[j]`` by position
        (fruits/iss/semiring.py:185-199).  ``lengths`` (host array): the (N, T) lookup whose
        row n is the weighting's row for a series of ``lengths[n]`` elements."""
        if self.weighting is None:
            return None
        if lengths is not None:
            return nat.to_device(lookup_rows(self.weighting._row, lengths, int(Xd.shape[2])))
        # (max-plus results meet fitted quantiles in exact ties: bit-exact lookup there)
        lk = self.weighting.lookup_device(Xd, exact=not isinstance(self.semiring, Reals))
        n = int(Xd.shape[0])
        if lk.shape[0] != 1:
            if lk.shape[0] < n:
                raise IndexError("weighting lookup has fewer rows than the input")
            lk = lk[:n]
        return lk.contiguous()

    def word_batches(self, N: int, T: int, batch_size: Optional[int] = None):
        """[start, stop) word ranges: ``batch_size`` words each, or as many as
        fit the device budget."""
        W = len(self.words)
        if batch_size is not None:
            return [(s, min(s + batch_size, W)) for s in range(0, W, batch_size)]
        budget = max(_device_budget_bytes() // max(8 * N * T, 1), 1)
        out, s = [], 0
        while s < W:
            e, rows = s, 0
            while e < W and (e == s or rows + self._depth(e) <= budget):
                rows += self._depth(e)
                e += 1
            out.append((s, e))
            s = e
        return out

    def transform_device(self, Xd, start: int = 0, stop: Optional[int] = None,
                         lookup_d="auto", out=None, groups: int = 0, indices=None):
        """Iterated sums of words [start, stop) (or of ``indices``) as a
        (K, N, T) device tensor."""
        self._check_supported()
        stop = len(self.words) if stop is None else stop
        if self._argmax:
            # values of every prefix, then positions + back-tracking (fr_arctic_argmax)
            idx = tuple(range(start, stop)) if indices is None else tuple(indices)
            plan = self._plan_indices(idx)
            if plan.max_dim > Xd.shape[1]:
                raise IndexError(
                    f"a word references dimension {plan.max_dim} but the input has "
                    f"only {Xd.shape[1]}")
            if isinstance(lookup_d, str):
                lookup_d = self.lookup_device(Xd)
            V = plan.run(Xd, lookup_d, layout="KNT", groups=groups)
            res = nat.arctic_argmax(V, [len(self.words[i]) for i in idx])
            if out is not None:
                out.copy_(res)
                return out
            return res
        if self._has_generic:
            idx = tuple(range(start, stop)) if indices is None else tuple(indices)
            if self._generic_in(idx):
                if isinstance(lookup_d, str):
                    lookup_d = self.lookup_device(Xd) if len(self._class_runs(idx)) > 1 else None
                if out is not None and not out.is_contiguous():
                    raise TypeError("out must be contiguous")
                return self._transform_lowered(Xd, idx, lookup_d, out, groups)
        plan = self._plan(start, stop) if indices is None else self._plan_indices(indices)
        if plan.max_dim > Xd.shape[1]:
            raise IndexError(
                f"a word references dimension {plan.max_dim} but the input has "
                f"only {Xd.shape[1]}")
        if isinstance(lookup_d, str):
            lookup_d = self.lookup_device(Xd)
        T = int(Xd.shape[2])
        if not plan.fits(T):
            # many distinct alphas -> more exp tables than a workgroup can stage: halves
            if indices is None:
                indices = tuple(range(start, stop))
            if len(indices) == 1:
                raise NotImplementedError(
                    f"word {self.words[indices[0]]} alone needs {plan.staged_rows} staged rows "
                    "(input dimensions + exp tables of its distinct alphas): more than the "
                    "LDS of a workgroup holds")
            if out is None:
                out = nat.torch().empty((plan.rows, int(Xd.shape[0]), T),
                                        dtype=nat.torch().float64, device=Xd.device)
            half = len(indices) // 2
            k0 = sum(self._depth(i) for i in indices[:half])
            self.transform_device(Xd, lookup_d=lookup_d, out=out[:k0], groups=groups,
                                  indices=indices[:half])
            self.transform_device(Xd, lookup_d=lookup_d, out=out[k0:], groups=groups,
                                  indices=indices[half:])
            return out
        # A big materialising launch of a small plan: prepare it once (fr_plan_prepare compiles
        # the plan's static program with hipRTC when no pre-compiled one matches - about a
        # second the first time a word list is seen, milliseconds from the disk cache after).
        # FRUITS_AMD_AUTO_PREPARE=0 leaves that to explicit Plan.prepare calls.
        N, T = int(Xd.shape[0]), int(Xd.shape[2])
        if (8 * plan.rows * N * T >= _AUTO_PREPARE_BYTES and not getattr(plan, "_prepared", False)
                and os.environ.get("FRUITS_AMD_AUTO_PREPARE", "1") != "0"
                and not nat.torch().cuda.is_current_stream_capturing()):
            plan.prepare(N, T, groups)
            plan._prepared = True
        return plan.run(Xd, lookup_d, out=out, layout="KNT", groups=groups)

    # ------------------------------------------------------------------ reference API
    @staticmethod
    def _validate(X) -> np.ndarray:
        if not isinstance(X, np.ndarray) or X.dtype != np.float64 or X.ndim != 3:
            raise TypeError("input has to be a float64 array of shape (N, D, T)")
        return X

    def _transform(self, X: np.ndarray) -> np.ndarray:
        X = self._validate(X)
        self._attach_cache(X)
        Xd = nat.to_device(X)
        return nat.to_host(self.transform_device(Xd))

    def n_iterated_sums(self) -> int:
        """Number of iterated sums ``transform`` returns."""
        if self.mode == ISSMode.EXTENDED:
            if self._argmax:
                return sum(len(w) + len(w) * (len(w) + 1) // 2 for w in self.words)
            return self._cache_plan.n_iterated_sums()
        if self._argmax:
            raise NotImplementedError(
                "Arctic argmax is not implemented when using ISSMode.SINGLE")
        return len(self.words)

    def batch_transform(self, X: np.ndarray,
                        batch_size: int = 1) -> Generator[np.ndarray, None, None]:
        """Yields ``(k, N, T)`` arrays, the iterated sums of ``batch_size`` words
        at a time (fruits/iss/iss.py:152-185)."""
        if batch_size > len(self.words):
            raise ValueError("batch_size too large, has to be < len(words)")
        X = self._validate(X)
        self._attach_cache(X)
        Xd = nat.to_device(X)
        lookup_d = self.lookup_device(Xd)
        for s, e in self.word_batches(X.shape[0], X.shape[2], batch_size):
            yield nat.to_host(self.transform_device(Xd, s, e, lookup_d))

    def _copy(self) -> "ISS":
        return ISS(self.words, mode=self.mode, semiring=self.semiring,
                   weighting=self.weighting)

    def _label(self, index: int) -> str:
        if self.mode == ISSMode.EXTENDED:
            text = self._cache_plan.get_word_string(index)
        else:
            text = str(self.words[index])
        if not isinstance(self.semiring, Reals):
            text += " : " + self.semiring.__class__.__name__
        if self.weighting is not None:
            text += " : " + self.weighting.__class__.__name__
        return text
