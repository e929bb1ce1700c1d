"""Pipeline orchestration: ``Fruit`` and ``FruitSlice`` (mirrors fruits/fruit.py).

The public behaviour is the reference's - slices of preparateurs -> ISS ->
sieves, per-iterated-sum fitted sieve copies, feature column order (slice, then
iterated sum, then sieve, then the sieve's own (segment, band) order) and the
final ``nan_to_num``.  The execution is not: the batch is uploaded to HBM once,
every stage runs as HIP kernels on device tensors, iterated sums are produced
by one launch per word batch instead of one numba call per word, sieves write
straight into the ``(N, F)`` feature tensor, and only that tensor travels back.
"""
from __future__ import annotations

import inspect
import os
from typing import Callable, Generator, Literal, Optional, Union

import numpy as np

from . import _native as nat
from . import preparation as _prep
from .cache import SharedSeedCache
from .callback import AbstractCallback
from .iss.iss import ISS
from .iss.weighting import _PathLength, _SeriesIndependent
from .lengths import check_lengths, require_support, with_lengths
from .preparation.abstract import Preparateur
from .seed import Seed
from .sieving.abstract import FeatureSieve


def _check_batch(X) -> np.ndarray:
    if not isinstance(X, np.ndarray) or X.ndim != 3:
        raise TypeError("input has to be an array of shape (N, D, T)")
    if X.dtype != np.float64:
        raise TypeError("input has to be float64 (the reference's numba kernels "
                        "accept nothing else)")
    return X


_SELECTIONS_IN_FLIGHT = 6     # of the 8 the library allows per device (fr_select_ranks_begin)


class _FittedRows:
    """The fitted sieve copies of a slice, one list per iterated sum - what fruits/fruit.py:462-476
    builds as it fits - held as ARRAYS: per sieve the thresholds of all rows, computed from the
    device's order statistics with numpy (np.quantile's interpolation over the rows at once).  The
    copy objects are made when somebody asks for a row; the fused pipeline reads the arrays.
    (fruit_reduced: 633 rows x 7 sieves - as eager Python objects, each fitted by a call of its
    own, they were 20 of the 36 ms of Fruit.fit, all on the thread that also feeds the device.)"""

    def __init__(self, sieves, cache) -> None:
        self._sieves = list(sieves)
        self._cache = cache
        self._segments: list = []     # [first row, rows, per sieve (rows, len(q)) array or None]
        self._n = 0
        self._made: dict = {}

    def __getstate__(self):
        # (copies somebody changed are part of the state; the cache is the process's)
        return {"_sieves": self._sieves, "_cache": None, "_n": self._n, "_made": {},
                "_segments": [[r0, n, [None if q is None else q.copy() for q in qs]]
                              for r0, n, qs in self._with_made()]}

    def _with_made(self):
        for r0, n, qs in self._segments:
            qs = [None if q is None else q.copy() for q in qs]
            for k, fitted in self._made.items():
                if r0 <= k < r0 + n:
                    for i, sv in enumerate(fitted):
                        if qs[i] is not None:
                            qs[i][k - r0] = _leaf(sv)._quantiles
            yield r0, n, qs

    def add_rows(self, n: int) -> list:
        """A run of ``n`` more rows; returns its (still empty) list of threshold arrays."""
        seg = [self._n, n, [None] * len(self._sieves)]
        self._segments.append(seg)
        self._n += n
        return seg[2]

    def __len__(self) -> int:
        return self._n

    def __bool__(self) -> bool:
        return self._n > 0

    def __iter__(self):
        return (self[k] for k in range(self._n))

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(self._n))]
        if k < 0:
            k += self._n
        if not 0 <= k < self._n:
            raise IndexError(k)
        fitted = self._made.get(k)
        if fitted is None:
            r0, _, qs = next(seg for seg in self._segments if seg[0] <= k < seg[0] + seg[1])
            fitted = [sv.copy() for sv in self._sieves]
            for sv, q in zip(fitted, qs):
                sv._cache = self._cache
                if q is not None:
                    _leaf(sv)._quantiles = q[k - r0].copy()
            self._made[k] = fitted
        return fitted

    def thresholds(self, i: int, rows) -> Optional[np.ndarray]:
        """(len(rows), len(q)) thresholds of sieve ``i`` (None: it is not fitted on data)."""
        if not self._segments or self._segments[0][2][i] is None:
            return None
        if len(self._segments) == 1 and not self._made:
            table = self._segments[0][2][i]
        else:
            table = np.concatenate([qs[i] for _, _, qs in self._with_made()])
        return table[np.asarray(rows, dtype=np.int64)]


def _reduced(sv):
    """(sieve that holds the cuts and thresholds, FR_SIEVE_* kind, differencing order of the
    transform, of the fit) of a sieve the fused pipeline or the device-side fit can express
    (SegmentSieve._reduced; a wrapper of sieving/wrapper.py answers for its inner sieve), else
    None."""
    return sv._reduced() if hasattr(sv, "_reduced") else None


def _leaf(sv):
    """The sieve that holds ``sv``'s thresholds: the inner sieve of a reducible wrapper."""
    form = _reduced(sv)
    return sv if form is None else form[0]


def _n_thresholds(sv) -> int:
    """Entries of a sieve's row of the pipeline's threshold table: a band sieve's len(q); PPV /
    CPV say (their ``_q`` holds the fitted thresholds, sieving/implicit.py)."""
    return sv._n_thresholds() if hasattr(sv, "_n_thresholds") else len(sv._q)


def _interpolated_quantiles(sieve, reqs, lo_vals: np.ndarray, hi_vals: np.ndarray) -> np.ndarray:
    """SegmentSieve._set_quantiles_from_stats for all rows at once: (rows, len(q)) thresholds
    from the (rows, len(reqs)) order statistics np.quantile interpolates between."""
    if hasattr(sieve, "_thresholds_from_stats"):      # PPV / CPV: their own order, not sorted
        return sieve._thresholds_from_stats(reqs, lo_vals, hi_vals)
    qs = np.empty((lo_vals.shape[0], len(sieve._q)))
    qs[:] = [np.inf if q == 1.0 else (-np.inf if q == -1.0 else 0.0) for q in sieve._q]
    for j, (i, _, _, gamma) in enumerate(reqs):
        # numpy's _lerp (lib/_function_base_impl.py): a + (b-a)*t, from the other end
        # when t >= 0.5
        a, b = lo_vals[:, j], hi_vals[:, j]
        d = b - a
        qs[:, i] = a + d * gamma if gamma < 0.5 else b - d * (1 - gamma)
    return np.sort(qs, axis=1)


class Fruit:
    """Feature extractor made of one or more :class:`FruitSlice` objects whose
    features are concatenated.

    .. code-block:: python

        fruit = fruits_amd.Fruit("My Fruit")
        fruit.add(fruits_amd.preparation.INC)
        fruit.add(fruits_amd.ISS(fruits_amd.words.of_weight(2, dim=3),
                                 mode=fruits_amd.ISSMode.EXTENDED))
        fruit.add(fruits_amd.sieving.NPI(q=(0.5, 1.0)), fruits_amd.sieving.END)
        fruit.fit(X)
        features = fruit.transform(X)
    """

    def __init__(self, name: str = "") -> None:
        self.name: str = name
        self._slices: list[FruitSlice] = []
        self._slc_index: int = 0
        self._fitted: bool = False
        self._cursor: int = -1

    # ---- structure ------------------------------------------------------------
    def cut(self, slice: Optional["FruitSlice"] = None) -> None:
        """Appends a (new, empty) slice and makes it the current one."""
        self._slices.append(FruitSlice() if slice is None else slice)
        self._slc_index = len(self._slices) - 1
        self._fitted = False

    def copycut(self) -> None:
        self.cut(self.get_slice().deepcopy())

    def get_slice(self, index: Optional[int] = None) -> "FruitSlice":
        return self._slices[self._slc_index if index is None else index]

    def switch_slice(self, index: int) -> None:
        if not (0 <= index < len(self._slices)):
            raise IndexError("Index has to be in [0, len(self)-1]")
        self._slc_index = index

    def add(self, *objects: Union[Seed, Callable[[], Seed]]) -> None:
        """Adds preparateurs, ISS or sieves to the current slice."""
        if not self._slices:
            self.cut()
        self._slices[self._slc_index].add(*objects)
        self._fitted = False

    def nfeatures(self) -> int:
        return sum(slc.nfeatures() for slc in self._slices)

    # ---- fit / transform ----------------------------------------------------
    def fit(self, X: np.ndarray, cache: Optional[SharedSeedCache] = None, lengths=None) -> None:
        """``lengths``: integer array (N,), series n is ``X[n, :, :lengths[n]]`` (DESIGN.md,
        "Per-series lengths"); None: every series is T long."""
        X = _check_batch(X)
        cache_ = SharedSeedCache(X) if cache is None else cache
        # the slices are started one after the other; the device-side selections of a slice's
        # thresholds are only queued (fr_select_ranks_begin) and waited for at the end
        deferred: list = []
        try:
            for slc in self._slices:
                slc.fit(X, cache=cache_, deferred=deferred, lengths=lengths)
        finally:
            for finish in deferred:
                finish()
        # (the selection scratch of the device-side fit - a blob of device and page-locked memory
        # per slice in flight, some 50 MB each - lives outside torch's allocator and is kept for
        # the next fit: allocating it is a millisecond per blob on the fit's critical path.
        # fruits_amd.release_scratch() hands it back.)
        self._fitted = True

    def transform(self, X: np.ndarray,
                  callbacks: Optional[list[AbstractCallback]] = None,
                  cache: Optional[SharedSeedCache] = None, lengths=None) -> np.ndarray:
        """``(N, nfeatures)`` features of all slices.  ``lengths``: integer array (N,) - row n
        is then what ``transform(X[n:n+1, :, :lengths[n]])[0]`` returns; the values behind a
        series' length must be finite and influence nothing.

        Raises:
            RuntimeError: if :meth:`fit` was not called.
            NotImplementedError: with ``lengths``, for a seed that does not take them.
        """
        callbacks = callbacks or []
        if not self._fitted:
            raise RuntimeError("Missing call of self.fit")
        X = _check_batch(X)
        cache_ = SharedSeedCache(X) if cache is None else cache
        t = nat.torch()
        blocks = []
        for slc in self._slices:
            for cb in callbacks:
                cb.on_next_slice()
            blocks.append(slc.transform_device(X, callbacks, cache_, lengths=lengths))
        # assembled on the device: one download instead of a strided host copy per slice
        result = blocks[0] if len(blocks) == 1 else t.cat(blocks, dim=1)
        return nat.to_host(nat.nan_to_num(result.contiguous()))

    def fit_transform(self, X: np.ndarray,
                      callbacks: Optional[list[AbstractCallback]] = None,
                      lengths=None) -> np.ndarray:
        self.fit(X, lengths=lengths)
        return self.transform(X, callbacks=callbacks, lengths=lengths)

    # ---- the fitted state, to be handed to other processes (fruits_amd.parallel) ----
    def fit_state(self) -> bytes:
        """Everything ``fit`` derived from the data, pickled: the fitted seeds of every slice."""
        if not self._fitted:
            raise RuntimeError("Missing call of self.fit")
        import pickle
        return pickle.dumps([slc._fit_state() for slc in self._slices])

    def load_fit_state(self, state: bytes) -> None:
        """Makes this fruit (same configuration) the fitted fruit ``state`` was taken from."""
        import pickle
        states = pickle.loads(state)
        if len(states) != len(self._slices):
            raise ValueError("the state belongs to a fruit with another number of slices")
        for slc, st in zip(self._slices, states):
            slc._load_fit_state(st)
        self._fitted = True

    # ---- introspection ------------------------------------------------------
    def summary(self) -> str:
        bar = 80 * "="
        ident = "Fruit" + (f" {self.name!r}" if self.name != "" else "")
        ident += f" -> Features: {self.nfeatures()}"
        text = bar + "\n<" + f"{ident: ^78}" + ">\n" + bar + "\n"
        rule = "|" + 38 * "-"
        pairs = len(self._slices) - len(self._slices) % 2
        for i in range(0, pairs, 2):
            left = self._slices[i].summary().split("\n")
            right = self._slices[i + 1].summary().split("\n")
            height = max(len(left), len(right))
            left += [38 * " "] * (height - len(left))
            right += [38 * " "] * (height - len(right))
            text += rule + "|" + rule + "|\n"
            text += "\n".join(f"|{a}||{b}|" for a, b in zip(left, right))
            text += "\n" + rule + "|" + rule + "|\n"
        if len(self._slices) % 2:
            text += rule + "|\n|"
            text += self._slices[-1].summary().replace("\n", "|\n|")
            text += "|\n" + rule + "|\n"
        return text + bar

    def copy(self) -> "Fruit":
        dup = Fruit(self.name + " (Copy)")
        for slc in self._slices:
            dup.cut(slc.copy())
        return dup

    def deepcopy(self) -> "Fruit":
        dup = Fruit(self.name + " (Deepcopy)")
        for slc in self._slices:
            dup.cut(slc.deepcopy())
        return dup

    def label(self, index: int,
              level: Literal["prepared", "iterated sums", "features"] = "features",
              verbose: Literal[1, 2] = 1) -> str:
        """Label of one feature (or prepared input / iterated sum, by ``level``)."""
        for slc in self._slices:
            if level == "prepared":
                total = len(slc.get_preparateurs())
            elif level == "iterated sums":
                total = slc.niteratedsums()
            else:
                total = slc.nfeatures()
            if index < total:
                return slc.label(index, level, verbose)
            index -= total
        raise RuntimeError("Label index out of range")

    def __len__(self) -> int:
        return len(self._slices)

    def __iter__(self) -> "Fruit":
        self._cursor = -1
        return self

    def __next__(self) -> "FruitSlice":
        if self._cursor + 1 < len(self._slices):
            self._cursor += 1
            return self._slices[self._cursor]
        raise StopIteration()

    def __getitem__(self, index: int) -> "FruitSlice":
        return self.get_slice(index)


# The three stages of a slice, in pipeline order: (name of the stage's list, what may be added to
# it, the suffix of its add_ / get_ / clear_ verbs; fruits/fruit.py:280-429 is the contract - the
# verbs, what they accept and raise).  Everything a slice derives from its configuration (the
# fitted sieve copies, fused pipelines) is dropped whenever a stage changes.
_STAGES = (
    ("preparateurs", Preparateur, "preparateur", "preparateurs"),
    ("iss", ISS, "iss", "iss"),
    ("sieves", FeatureSieve, "sieve", "sieves"),
)


class FruitSlice:
    """One slice: preparateurs -> (chained) ISS -> sieves."""

    def __init__(self) -> None:
        self._stage: dict[str, list[Seed]] = {name: [] for name, *_ in _STAGES}
        self.fit_sample_size: Union[float, int] = 1
        self._invalidate()

    def _invalidate(self) -> None:
        # one list of fitted sieve copies per iterated sum
        self._sieves_extended: list[list[FeatureSieve]] = []
        self._fused_cache: dict = {}
        self._fitted: bool = False

    # the stage lists under the names the rest of the slice reads them by
    _preparateurs = property(lambda self: self._stage["preparateurs"])
    _iss = property(lambda self: self._stage["iss"])
    _sieves = property(lambda self: self._stage["sieves"])

    # ---- configuration ------------------------------------------------------
    def _put(self, stage: str, accepts: type, seed: Seed) -> None:
        if not isinstance(seed, accepts):
            raise TypeError
        self._stage[stage].append(seed)
        self._invalidate()

    def _wipe(self, stage: str) -> None:
        self._stage[stage] = []
        self._invalidate()

    def add(self, *objects: Union[Seed, Callable[[], Seed]]) -> None:
        """Appends seeds (instances, or classes to be instantiated without arguments) to the
        stage each belongs to."""
        for obj in objects:
            seed = obj() if inspect.isclass(obj) else obj
            for stage, accepts, _, _ in _STAGES:
                if isinstance(seed, accepts):
                    self._put(stage, accepts, seed)
                    break
            else:
                raise TypeError(f"Cannot add variable of type {type(seed)}")

    def clear(self) -> None:
        for stage, *_ in _STAGES:
            self._wipe(stage)
        self.fit_sample_size = 1

    def _fit_state(self) -> dict:
        return {"stage": self._stage, "extended": self._sieves_extended,
                "fit_sample_size": self.fit_sample_size}

    def _load_fit_state(self, state: dict) -> None:
        if [len(v) for v in state["stage"].values()] != [len(v) for v in self._stage.values()]:
            raise ValueError("the state belongs to a slice of another configuration")
        self._stage = state["stage"]
        self.fit_sample_size = state["fit_sample_size"]
        self._invalidate()
        self._sieves_extended = state["extended"]
        self._fitted = True

    def niteratedsums(self) -> int:
        return int(np.prod([iss.n_iterated_sums() for iss in self._iss]))

    def nfeatures(self) -> int:
        return self.niteratedsums() * sum(sieve.nfeatures() for sieve in self._sieves)

    def _compile(self) -> None:
        for stage, what in (("iss", "ISS"), ("sieves", "feature sieves")):
            if not self._stage[stage]:
                raise RuntimeError(f"No {what} given")

    def _select_fit_indices(self, X: np.ndarray) -> np.ndarray:
        # same draws from numpy's global generator as the reference
        # (fruits/fruit.py:430-438) so a seeded run picks the same series
        if isinstance(self.fit_sample_size, int) and self.fit_sample_size == 1:
            ind = np.random.randint(0, X.shape[0])
            return np.arange(ind, ind + 1)
        s = max(int(self.fit_sample_size * X.shape[0]), 1)
        return np.random.choice(X.shape[0], size=s, replace=False)

    def _select_fit_sample(self, X: np.ndarray) -> np.ndarray:
        return X[self._select_fit_indices(X), :, :]

    # ---- device pipeline --------------------------------------------------------
    def _prepare_device(self, Xd, cache, callbacks=(), fit_on=None, lengths_d=None):
        for prep in self._preparateurs:
            prep._cache = cache
            if fit_on is not None:
                if prep._fit_needs_data():
                    prep.fit(nat.to_host(Xd))
                elif prep._fit_needs_shape():
                    prep.fit(np.broadcast_to(0.0, tuple(int(v) for v in Xd.shape)))
                else:
                    prep.fit(fit_on)
            Xd = with_lengths(prep._transform_device, Xd, lengths_d=lengths_d)
            for cb in callbacks:
                cb.on_preparateur(nat.to_host(Xd))
        return Xd

    def _iterate_iss_device(self, Xd, iss_index: int = 0, upto: Optional[int] = None,
                            lengths=None, indices=None) -> Generator:
        """Yields every iterated sum as an (N, T) device tensor, in the order of
        fruits/fruit.py:440-454 (chained ISS feed each row to the next ISS).  ``upto``: stop in
        front of that ISS of the chain and yield its (N, 1, T) INPUTS instead.  ``indices``
        (single ISS): the iterated sums of these words only, formed by ONE launch."""
        if upto is not None and iss_index == upto:
            yield Xd
            return
        if iss_index == len(self._iss):
            yield Xd[:, 0, :]
            return
        iss = self._iss[iss_index]
        if indices is not None:
            yield from iss.transform_device(Xd, indices=indices)
            return
        # (``lengths``: a single ISS - the gate of a ragged batch has seen to that)
        lookup = with_lengths(iss.lookup_device, Xd, lengths=lengths)
        for s, e in iss.word_batches(int(Xd.shape[0]), int(Xd.shape[2])):
            block = iss.transform_device(Xd, s, e, lookup)
            for k in range(block.shape[0]):
                if iss_index + 1 == len(self._iss):
                    yield block[k]
                else:
                    yield from self._iterate_iss_device(block[k].unsqueeze(1).contiguous(),
                                                        iss_index + 1, upto)

    # ---- device-side fit ------------------------------------------------------------
    def _fit_on_device(self, Sd, cache, deferred: Optional[list] = None) -> bool:
        """Fits the per-iterated-sum sieve copies without moving the fit sample's
        iterated sums to the host: the order statistics np.quantile interpolates
        between are selected on the device (fr_select_ranks).  Returns False when a
        sieve or the ISS layout needs the host path - among them a PPV / CPV with
        ``sample_size < 1``: every copy of it takes its quantiles of a random subset of its own.
        With ``sample_size == 1`` the subset is the whole sample, whose order statistics do not
        depend on the order of the rows; the draws from numpy's global generator the reference
        makes for it (fruits/sieving/implicit.py:104-108: iterated sum by iterated sum, sieve by
        sieve, threshold by threshold) are made HERE, when the slice is fitted, never in the
        deferred closures - the preparateurs of the next slice draw from the same generator.
        ``deferred``: the selections are only
        QUEUED (fr_select_ranks_begin); a closure per word batch that waits for its selection and
        forms the thresholds is appended - Fruit.fit runs them when every slice has been queued,
        so that the device goes from one slice's selection to the next slice's iterated sums
        without waiting for the host."""
        if os.environ.get("FRUITS_AMD_DEVICE_FIT", "1") == "0" or len(self._iss) != 1:
            return False
        # (a sieve wrapper that is its inner sieve at another differencing order is fitted as
        # that: the thresholds belong to the inner sieve - _reduced, sieving/wrapper.py)
        forms = [_reduced(sv) for sv in self._sieves]
        for sv, form in zip(self._sieves, forms):
            if sv.requires_fitting and not (form is not None and 0 <= form[3] <= 8):
                return False
            if form is not None and getattr(form[0], "_sample_size", 1.0) != 1.0:
                return False
        drawing = [form[0] for form in forms if form is not None and hasattr(form[0], "_fit_draws")]
        # what asks for order statistics, and the differencing order it asks them of
        leaves = [None if form is None else form[0] for form in forms]
        fit_inc = [None if form is None else form[3] for form in forms]
        iss = self._iss[0]
        Ns, T = int(Sd.shape[0]), int(Sd.shape[2])
        n = Ns * T
        lookup = iss.lookup_device(Sd)
        self._sieves_extended = _FittedRows(self._sieves, cache)
        for s, e in iss.word_batches(Ns, T):
            block = iss.transform_device(Sd, s, e, lookup)
            for _ in range(int(block.shape[0]) if drawing else 0):
                for sv in drawing:
                    sv._fit_draws(Ns)
            # (what a sieve asks for depends on its q and the sample size only: once per sieve,
            # not once per copy)
            asks = [leaf._quantile_requests(n) if sv.requires_fitting else None
                    for sv, leaf in zip(self._sieves, leaves)]
            # Every iterated sum is asked for the same order statistics: the jobs of ONE row -
            # (differencing order, rank) pairs, those that several sieves share (NPI / MPI with the
            # same band) once - are laid out as a template and repeated for the rows with numpy
            # (19 000 jobs per fit of fruit_reduced: as Python loops their construction left the
            # device idle for 2-4 ms per slice between the iterated sums and their selection)
            t_index: dict = {}
            t_inc, t_rank, t_pairs = [], [], []
            for inc, reqs in zip(fit_inc, asks):
                if reqs is None:
                    continue
                idx = []
                for (_, lo, hi, _) in reqs:
                    for r in (lo, hi):
                        if (inc, r) not in t_index:
                            t_index[(inc, r)] = len(t_inc)
                            t_inc.append(inc)
                            t_rank.append(r)
                    idx.append((t_index[(inc, lo)], t_index[(inc, hi)]))
                t_pairs.append((np.asarray([a for a, _ in idx], dtype=np.int64),
                                np.asarray([b for _, b in idx], dtype=np.int64)))
            K_rows, J = int(block.shape[0]), len(t_inc)
            rows = np.repeat(np.arange(K_rows, dtype=np.int32), J)
            incs = np.tile(np.asarray(t_inc, dtype=np.int32), K_rows)
            ranks = np.tile(np.asarray(t_rank, dtype=np.int64), K_rows)
            # the selection is QUEUED (fr_select_ranks_begin: no pass waits for the host) and this
            # thread goes on to the next slice; the thresholds of the rows are formed as arrays
            # when somebody waits for it (_FittedRows)
            pending = nat.Selection(block, rows, incs, ranks) if len(rows) else None
            tables = self._sieves_extended.add_rows(K_rows)

            def finish(pending=pending, block=block, t_pairs=t_pairs, tables=tables, asks=asks,
                       K_rows=K_rows, J=J):
                # (`block` lives until its selection is done)
                vals = (pending.result() if pending is not None else np.zeros(0)).reshape(K_rows, J)
                which = 0
                for i, (sieve, reqs) in enumerate(zip(leaves, asks)):
                    if reqs is not None:
                        lo_idx, hi_idx = t_pairs[which]
                        tables[i] = _interpolated_quantiles(sieve, reqs, vals[:, lo_idx], vals[:, hi_idx])
                        which += 1
            if deferred is None:
                finish()
            else:
                deferred.append(finish)
                # (a selection in flight owns one of 8 scratch blobs - and its (K, N, T) block:
                # a fruit of many slices, or a slice of many word batches, ends the oldest)
                while len(deferred) > _SELECTIONS_IN_FLIGHT:
                    deferred.pop(0)()
        return True

    # ---- fused ISS + sieves (one launch, no (K, N, T) tensor) --------------------
    def _fusable(self) -> bool:
        from .sieving.implicit import CPV, PPV
        from .sieving.increment import MPI, NPI, XPI
        from .sieving.segment import AVG, CUR, END, MAX, MIN, STD
        from .sieving.wrapper import INC, INT
        # (a chain of ISS: the LAST one fuses with the sieves, once per row of the chain in front
        # of it - fruits/fruit.py:440-454 feeds every row of an ISS to the next one)
        if os.environ.get("FRUITS_AMD_FUSED", "1") == "0" or not self._iss:
            return False
        last = self._iss[-1]
        if getattr(last, "_argmax", False):
            # Arctic argmax: the running maxima are materialised, every argmax row is formed in
            # LDS for the sieves that look at it (fr_pipeline_set_argmax) - differencing orders
            # 0 to 2, single ISS; anything else keeps fr_arctic_argmax + one launch per sieve
            if len(self._iss) != 1 or os.environ.get("FRUITS_AMD_FUSED_ARGMAX", "1") == "0":
                return False
            for sv in self._sieves:
                if type(sv) not in (NPI, MPI, END):
                    return False     # (the argmax kernel forms NPI / MPI / END only)
                if type(sv) in (NPI, MPI) and not 0 <= sv._inc <= 2:
                    return False
        if type(last) is not ISS:
            from .iss.cos import CosWISS
            # the factorised CosWISS kernels fuse; the term-by-term path reduces first
            if type(last) is not CosWISS or not last._native():
                return False
            if last._ffn_size is not None and len(self._iss) != 1:
                return False     # (every (word, frequency) reads its own transformed input:
                                 # fused word by word, _transform_ffn_fused - single ISS only)
        for sv in self._sieves:
            # a wrapper (INC / INT) takes part as its inner sieve at another differencing order
            # where that is exact (_reduced, sieving/wrapper.py); else the slice materialises
            form, inner = _reduced(sv), sv
            while type(inner) in (INC, INT):
                inner = inner._sieve
            if form is None or form[0] is not inner:
                return False
            # (LPI is not fused: a run crosses lanes, waves and time chunks - DESIGN 4.3)
            if type(inner) not in (NPI, MPI, XPI, MAX, MIN, END, CUR, AVG, STD, PPV, CPV):
                return False
            if type(inner) is not END and not -8 <= form[2] <= 8:
                return False     # (cumulated rows: series of one time chunk; the pipeline says if not)
        return True

    def _fused(self, T: int, indices=None, chain_row: int = 0, D: Optional[int] = None,
               ragged: bool = False):
        """The fused pipeline for series length T (thresholds of the fitted sieve
        copies already resolved), or None when a sieve or the weighting is outside
        the fused set; cached until the next fit.  ``indices``: only these words
        (a rank's share of a word-sharded slice, fruits_amd.parallel); the pipeline
        then produces the feature columns of their iterated sums, in that order.
        ``chain_row`` (chained ISS): the pipeline of the LAST ISS for the ``chain_row``-th row of
        the chain in front of it - the same program, that row's thresholds.
        ``ragged``: the pipeline for a batch with per-series lengths - every sieve's cuts are
        slots of the per-series table (_arm_lengths); an entry of its own, never the dense one."""
        key = T if indices is None else (T, tuple(indices))
        if chain_row:
            key = (key, chain_row)
        if ragged:
            key = (key, "ragged")
        # Generic words (iss/lowering.py): the plan runs on virtual rows formed from the prepared
        # (N, D, T) input, so the pipeline belongs to that D.  Fused are a single ISS over Reals
        # or Arctic (no output unshift) whose weighting, if any, meets generic words only;
        # everything else - Bayesian, whose rows come out time-shifted, chains that end in
        # generic words, generic next to weighted simple words - materialises through
        # ISS.transform_device.
        iss = self._iss[-1] if self._iss else None
        generic = getattr(iss, "_has_generic", False)
        if generic:
            used = range(len(iss.words)) if indices is None else indices
            if (D is None or len(self._iss) != 1 or iss.needs_unshift() or getattr(iss, "_argmax", False)
                    or (iss.weighting is not None and len(iss._class_runs(used)) > 1)):
                return None
            key = (key, "D", int(D))
        if key not in self._fused_cache:
            self._fused_cache[key] = self._build_fused(T, indices, chain_row, D if generic else None, ragged)
        return self._fused_cache[key]

    def _build_fused(self, T: int, indices, chain_row: int, D: Optional[int], ragged: bool):
        """``_fused`` behind its cache: the pipeline of the iterated sums of the words ``indices``
        (None: all) of the last ISS, or None.  ``D``: the dimensions a plan of generic words is
        lowered for."""
        if not self._fusable():
            return None
        iss = self._iss[-1]
        iss._check_supported()
        words = tuple(range(len(iss.words)) if indices is None else indices)
        # (argmax: the pipeline's rows are the argmax rows, not the plan's)
        argmax = [len(iss.words[i]) for i in words] if getattr(iss, "_argmax", False) else None
        plan = iss._plan_indices(words) if D is None else iss._plan_indices(words, D=D)
        if hasattr(iss, "_arm_plan"):     # CosWISS dropout: the plan carries the mask
            iss._arm_plan(plan, words, T)
        rows = [chain_row * iss.n_iterated_sums() + r for r in self._rows_of_words(iss, words)]
        acting = self._sieves_extended[rows[0]] if self._sieves_extended and rows else self._sieves
        specs, cut_columns, n_slots = self._pipeline_specs(acting, T, ragged)
        if not rows or not plan.fits(T):
            return None
        try:
            pipe = nat.Pipeline(plan, specs, T, argmax_lengths=argmax)
        except ValueError:
            return None
        assert pipe.rows == len(rows)
        pipe.set_quantiles(self._threshold_table(rows, pipe.q_stride))
        pipe._cut_columns = [(slot0, sv) for slot0, sv in cut_columns.values()]
        pipe._cut_slots = n_slots
        return pipe

    @staticmethod
    def _rows_of_words(iss, words) -> list:
        """The iterated sums (rows of the whole word list, reference order) of ``words``."""
        first = [0, *np.cumsum([iss._depth(i) for i in range(len(iss.words))]).tolist()]
        return [r for i in words for r in range(first[i], first[i + 1])]

    def _threshold_table(self, rows, q_stride: int) -> np.ndarray:
        """The pipeline's ``(len(rows), q_stride)`` thresholds: per iterated sum in ``rows`` those
        of its fitted sieve copies, in sieve order (END has none) - read from the arrays of
        ``_FittedRows`` or from the copy objects, whichever ``_sieves_extended`` holds."""
        fitted = self._sieves_extended
        quant = np.zeros((len(rows), q_stride))
        off = 0
        for i, sv in enumerate(self._sieves):
            leaf, kind, _, _ = _reduced(sv)
            if kind == nat.FR_SIEVE_END:
                continue
            n = _n_thresholds(leaf)
            if isinstance(fitted, _FittedRows):     # (the thresholds of all rows are arrays already)
                th = fitted.thresholds(i, rows)
                if th is None:
                    leaf._get_unfitted_quantiles()
                    th = leaf._quantiles
            else:
                th = []
                for row in rows:
                    copy = _reduced(fitted[row][i])[0] if fitted else leaf
                    if not copy.requires_fitting:
                        copy._get_unfitted_quantiles()
                    th.append(copy._quantiles)
            quant[:, off:off + n] = th
            off += n
        return quant

    @staticmethod
    def _pipeline_specs(acting, T: int, ragged: bool = False):
        """What fr_pipeline_create is told about the sieves ``acting`` for series of length T:
        (specs, cut columns, slots of the per-series cut table).  ``ragged``: integer cuts name
        slots too - they resolve per series length (lengths.resolve_cuts; END's own table,
        lengths.resolve_end_cuts) - and PPV / CPV the slot pair {0, length} (cut column None)."""
        # float ("coquantile") cuts differ from series to series: such a sieve names
        # columns of a per-series table instead of indices; sieves with the same cuts
        # share their columns (so NPI / MPI pairs still merge)
        # (the sieves that transform are the fitted COPIES, which forget coquantile_norm -
        # fruits/sieving/segment.py:90-91 - so the copies decide the norm here too)
        specs, cut_columns, n_slots = [], {}, 0
        for sv in acting:
            # (a wrapper: its inner sieve at the reduced order - cuts, thresholds and the column
            # order are the inner sieve's, which are the wrapper's)
            sv, kind, inc, _ = _reduced(sv)
            if kind == nat.FR_SIEVE_END:
                inc = 0
            if kind in (nat.FR_SIEVE_PPV, nat.FR_SIEVE_CPV):
                # (the whole row itself; the thresholds in the sieve's own order)
                segments = nat.FR_SIEVE_SEGMENTS if sv._segments else 0
                if ragged:
                    if "length" not in cut_columns:
                        cut_columns["length"] = (n_slots, None)
                        n_slots += 2
                    slot0 = cut_columns["length"][0]
                    specs.append((kind | segments | nat.FR_SIEVE_SERIES_CUTS, 0,
                                  np.array([slot0, slot0 + 1], dtype=np.int64), _n_thresholds(sv)))
                    continue
                specs.append((kind | segments, 0,
                              np.array([0, T], dtype=np.int64), _n_thresholds(sv)))
                continue
            if sv._has_float_cuts() or ragged:
                cuts_key = (tuple(sv._cut), sv._coquantile_norm)
                if ragged:
                    cuts_key = ("int", tuple(sv._cut), kind == nat.FR_SIEVE_END)
                if cuts_key not in cut_columns:
                    cut_columns[cuts_key] = (n_slots, sv)
                    n_slots += len(sv._cut) + 1
                slot0 = cut_columns[cuts_key][0]
                specs.append((kind | nat.FR_SIEVE_SERIES_CUTS, inc,
                              np.arange(slot0, slot0 + len(sv._cut) + 1), len(sv._q)))
            else:
                specs.append((kind, inc, sv._int_cut_row(T), len(sv._q)))
        return specs, cut_columns, n_slots

    @staticmethod
    def _auto_prepare(pipe, N: int, T: int) -> None:
        """A fused launch asks for its pipeline's own kernels - the fused walk compiled at run time
        (hipRTC) with the sieves and the plan as immediates, 1.3 to 2 times as fast as the generic
        instance - WITHOUT ever waiting for the compiler: what an earlier process on this machine
        compiled comes from the disk cache right away (milliseconds; launches from 16 MiB of
        iterated sums on); a compilation (seconds the first time) runs on a helper thread for
        launches from 256 MiB on - this launch and any other before it is done take the generic
        kernel, later ones the compiled one (same results).  FRUITS_AMD_AUTO_PREPARE=0: never,
        =cached: what the disk cache and the kernels shipped with the build hold, no compiler,
        =all: every fused launch, and waited for; ``pipeline.prepare(N)`` is the explicit,
        synchronous way."""
        mode = os.environ.get("FRUITS_AMD_AUTO_PREPARE", "1")
        if mode == "0" or getattr(pipe, "_prepared_for", None) == N:
            return
        size = 8 * N * pipe.plan.rows * T
        if mode == "all":
            pipe.prepare(N)
        elif size >= (16 << 20):
            # (a stream capture must not see the uploads, module loads and the helper thread's
            # work: a captured launch takes what is there - fr_pipeline_prepare before the capture
            # is the documented way)
            if nat.torch().cuda.is_current_stream_capturing():
                return
            # the uploads (plan tables, the tables of a plan in pieces) and whatever the disk cache
            # or the kernels shipped with the build hold: here, on the caller's thread ...
            pipe.prepare_cached(N)
            # ... the helper thread only compiles and loads what is still missing
            if size >= (256 << 20) and mode != "cached" and not pipe.fully_compiled():
                pipe.prepare_in_background(N)
        else:
            return
        pipe._prepared_for = N

    def _arm_series_cuts(self, pipe, N: int, T: int, cache) -> None:
        """Uploads the per-series boundaries of the float-cut sieves of a fused pipeline
        (SegmentSieve._get_transformed_cuts on this batch's cache) for a run on N series."""
        if not getattr(pipe, "_cut_slots", 0):
            return
        table = np.zeros((N, pipe._cut_slots), dtype=np.int32)
        shape = np.empty((N, T))
        for first, sv in pipe._cut_columns:
            sv._cache = cache
            rows = sv._get_transformed_cuts(shape)      # sorted, leading 0; END checks its range
            table[:, first:first + rows.shape[1]] = np.clip(rows, 0, T)
        pipe.set_series_cuts(nat.to_device(table, dtype=np.int32))

    @staticmethod
    def _arm_lengths(pipe, lengths: np.ndarray, lengths_d) -> None:
        """Uploads the per-series boundaries of a ragged pipeline - every sieve's integer cuts
        resolved for each series' length - and hands it the lengths (STD's statistics, the
        divisions of PPV / CPV).  END's IndexError for a series too short is raised here."""
        table = np.zeros((len(lengths), pipe._cut_slots), dtype=np.int32)
        for first, sv in pipe._cut_columns:
            if sv is None:
                table[:, first + 1] = lengths
            else:
                rows = sv._series_cut_rows(lengths)
                table[:, first:first + rows.shape[1]] = rows
        pipe.set_series_cuts(nat.to_device(table, dtype=np.int32))
        pipe.set_lengths(lengths_d)

    def _fusable_preparation(self, T: int):
        """(inc_lag, as_new, standardize, eps) when the preparateur chain is one the fused
        launch forms while staging the raw input - [INC | NEW(INC)] [STD], the chains of the
        experiment fruits - else None (the prepared input is then materialised)."""
        INC, STD = _prep.INC, _prep.STD     # (the preparateurs, not the sieves of the same names)
        level = os.environ.get("FRUITS_AMD_FUSED_PREP", "1")
        if level == "0":
            return None
        # (CosWISS: the kernel CAN form the prepared rows where a letter reads them - but it reads
        # them once per (word, frequency, letter), so the differences and divisions are redone 165
        # times per series for fruit_reduced's slices: 3.08 ms against 2.53 ms with the small
        # prepared tensor materialised once.  Only on request: FRUITS_AMD_FUSED_PREP=2.)
        if level != "2" and any(type(iss) is not ISS for iss in self._iss):
            return None
        preps = list(self._preparateurs)
        lag, as_new, std, eps = 0, False, 0, 0.0

        def plain_inc(p):
            return (type(p) is INC and p._depth == 1 and p._zero_padding
                    and isinstance(p._lag(T), int) and 1 <= p._lag(T) < T)
        if preps and plain_inc(preps[0]):
            lag = preps.pop(0)._lag(T)
        elif preps and type(preps[0]) is _prep.NEW and preps[0]._preparateur is not None \
                and plain_inc(preps[0]._preparateur):
            lag, as_new = preps.pop(0)._preparateur._lag(T), True
        if preps and type(preps[0]) is STD and preps[0]._separately:
            p = preps.pop(0)
            std, eps = (2 if p._div_std else 1), float(p._eps)
        if preps or (lag == 0 and std == 0):
            return None
        # The lookup of a weighting is computed from what the ISS is handed
        # (fruits/iss/weighting.py:65-66) - the PREPARED input, which a fused preparation never
        # writes.  Safe are only weightings that do not look at the data (Indices, Plateaus) and
        # path lengths of the cache's RAW input; a Custom function, or any user subclass, gets
        # the materialised preparation.
        for iss in self._iss:
            w = getattr(iss, "weighting", None)
            if w is None or isinstance(w, _SeriesIndependent):
                continue
            if isinstance(w, _PathLength) and not w._on_prepared:
                continue
            return None
        return lag, as_new, std, eps

    def _attach(self, cache) -> None:
        for iss in self._iss:
            iss._cache = cache
            iss._attach_cache(None)

    # ---- fit / transform ----------------------------------------------------
    def _ragged_lengths(self, X: np.ndarray, lengths) -> Optional[np.ndarray]:
        """The validated ``lengths`` of a call, None when there are none; the gate: every seed
        of the slice is asked (``_supports_lengths``) before anything is launched."""
        lengths = check_lengths(lengths, X.shape[0], X.shape[2])
        if lengths is None:
            return None
        if len(self._iss) > 1:
            raise NotImplementedError("chained ISS do not support per-series lengths")
        require_support((*self._preparateurs, *self._iss, *self._sieves))
        return lengths

    def fit(self, X: np.ndarray, cache: Optional[SharedSeedCache] = None,
            deferred: Optional[list] = None, lengths=None) -> None:
        self._compile()
        self._fused_cache = {}
        X = _check_batch(X)
        lengths = self._ragged_lengths(X, lengths)
        if cache is None:
            cache = SharedSeedCache(X)
        # the fit sample: rows of the input, gathered ON THE DEVICE from the cache's one upload of
        # X when the cache holds this batch (every slice of a fruit draws its own sample: a host
        # gather + upload per slice otherwise); the host copy only for a preparateur whose fit
        # looks at the data
        indices = self._select_fit_indices(X)
        if lengths is not None and not (lengths == X.shape[2]).all():
            # The sample is drawn as ever.  Series of ONE length (the default sample of one
            # series among them) are truncated to it and fitted as the ordinary batch they are;
            # a sample of unequal lengths is fitted on the host, every threshold from the valid
            # parts of its rows (_fit_valid).
            sample_lengths = lengths[indices]
            if (sample_lengths == sample_lengths[0]).all():
                X = np.ascontiguousarray(X[indices, :, :int(sample_lengths[0])])
                indices, sample_lengths = np.arange(X.shape[0]), None
                cache = SharedSeedCache(X)
            else:
                self._fit_unequal(X[indices, :, :], sample_lengths, cache)
                return
        needs_host = any(prep._fit_needs_data() for prep in self._preparateurs)
        whole = cache._input_dev is not None or 2 * len(indices) >= X.shape[0]   # (else: upload the sample alone)
        if cache._input is X and not needs_host and whole:
            sample = X[indices[:1], :, :]            # (what a data-blind Seed.fit is handed)
            Sd0 = cache.input_device(X)[nat.to_device(indices, dtype=np.int64)]
        else:
            sample = X[indices, :, :]
            Sd0 = nat.to_device(sample)
        Sd = self._prepare_device(Sd0, cache, fit_on=sample)
        self._attach(cache)
        for iss in self._iss:
            if iss.requires_fitting:
                iss.fit(nat.to_host(Sd))
        if not any(sieve.requires_fitting for sieve in self._sieves):
            self._fitted = True
            return
        self._sieves_extended = []
        if self._fit_on_device(Sd, cache, deferred):
            self._fitted = True
            return
        for itsum in self._iterate_iss_device(Sd):
            host = None
            fitted = [sieve.copy() for sieve in self._sieves]
            for sieve in fitted:
                sieve._cache = cache
                if sieve.requires_fitting:
                    if host is None:
                        host = nat.to_host(itsum)
                    sieve.fit(host)
            self._sieves_extended.append(fitted)
        self._fitted = True

    def _fit_unequal(self, sample: np.ndarray, lengths: np.ndarray, cache) -> None:
        """Fits the sieves on a sample whose series differ in length, on the host: the sample is
        prepared and its iterated sums are formed with the tails in place (both are causal), and
        every sieve copy takes its quantiles over the concatenated VALID parts of its
        pre-transformed rows (``_fit_valid``; PPV / CPV raise NotImplementedError there)."""
        for sieve in self._sieves:
            if sieve.requires_fitting and not hasattr(sieve, "_fit_valid"):
                raise NotImplementedError(
                    f"{type(sieve).__name__} ({sieve}) cannot be fitted on a sample of unequal lengths")
        lengths_d = nat.to_device(lengths.astype(np.int32), dtype=np.int32)
        Sd = self._prepare_device(nat.to_device(sample), cache, fit_on=sample, lengths_d=lengths_d)
        self._attach(cache)
        self._sieves_extended = []
        if any(sieve.requires_fitting for sieve in self._sieves):
            for itsum in self._iterate_iss_device(Sd, lengths=lengths):
                host = nat.to_host(itsum)
                fitted = [sieve.copy() for sieve in self._sieves]
                for sieve in fitted:
                    sieve._cache = cache
                    if sieve.requires_fitting:
                        sieve._fit_valid(host, lengths)
                self._sieves_extended.append(fitted)
        self._fitted = True

    def transform(self, X: np.ndarray,
                  callbacks: Optional[list[AbstractCallback]] = None,
                  cache: Optional[SharedSeedCache] = None, lengths=None) -> np.ndarray:
        return nat.to_host(self.transform_device(X, callbacks, cache, lengths=lengths))

    def transform_device(self, X: np.ndarray,
                         callbacks: Optional[list[AbstractCallback]] = None,
                         cache: Optional[SharedSeedCache] = None, lengths=None):
        """``transform`` with the ``(N, nfeatures)`` result left on the device."""
        callbacks = callbacks or []
        if not self._fitted:
            raise RuntimeError("Missing call of self.fit")
        X = _check_batch(X)
        lengths = self._ragged_lengths(X, lengths)
        if cache is None:
            cache = SharedSeedCache(X)
        if lengths is not None and (lengths == X.shape[2]).all():
            lengths = None      # (lengths that all equal T: the dense call itself, bit for bit)
        if lengths is not None and callbacks:
            raise NotImplementedError("callbacks do not support per-series lengths")
        Xd = cache.input_device(X) if cache._input is X else nat.to_device(X)
        feats = self._run(Xd, cache, lengths=lengths, callbacks=callbacks)
        if callbacks:
            out = nat.to_host(feats)
            for cb in callbacks:
                cb.on_sieving_end(out)
        return feats

    def _run(self, Xd, cache, *, indices=None, lengths=None, callbacks=()):
        """The route ladder from the device batch ``Xd`` to the features of a fitted slice
         - of the whole slice, of a ragged batch (``lengths``: validated, not all
        T) or of the words ``indices`` alone (a rank's share, fruits_amd.parallel):

        1. one fused launch on the RAW batch when the preparateur chain fuses into the staging;
        2. else the prepared input is materialised, and then, the first that applies:
           a. a CosWISS with the randomised ffn runs word by word (``_transform_ffn_fused``);
           b. a chain of ISS runs one fused launch per row of the chain (``_transform_chain_fused``);
           c. one fused launch on the prepared input - on the virtual rows for generic words;
           d. every iterated sum is materialised and every sieve copy runs over it.

        Callbacks see every intermediate result, so they take 2d."""
        ffn = getattr(self._iss[-1], "_ffn_size", None) is not None
        # What cannot come with lengths or with a share of the words: the gate refuses chains, ffn
        # and generic words for a ragged batch (_ragged_lengths, ISS._supports_lengths) and
        # transform_device callbacks; slice_transform_sharded shards a single ISS only.
        assert lengths is None or not (len(self._iss) > 1 or ffn or self._iss[0]._has_generic
                                       or callbacks or indices is not None)
        assert indices is None or (len(self._iss) == 1 and not callbacks)
        iss = self._iss[0]
        ragged = None if lengths is None else (
            lengths, nat.to_device(lengths.astype(np.int32), dtype=np.int32))
        self._attach(cache)
        if not callbacks and len(self._iss) == 1 and not ffn:
            # INC / NEW(INC) / STD formed while the fused launch stages the RAW rows: no
            # prepared tensor is written (one launch [+ the STD statistics pre-pass])
            D, T = int(Xd.shape[1]), int(Xd.shape[2])
            chain = self._fusable_preparation(T)
            fused = (self._fused(T, indices=indices, ragged=ragged is not None)
                     if chain is not None else None)
            if fused is not None and fused.ensure_preparation(D, *chain):
                return self._launch(fused, Xd, with_lengths(iss.lookup_device, Xd, lengths=lengths),
                                    cache, ragged)
        Pd = self._prepare_device(Xd, cache, callbacks, lengths_d=None if ragged is None else ragged[1])
        for cb in callbacks:
            cb.on_preparation_end(nat.to_host(Pd))
        if ffn and not callbacks and self._fusable():
            return self._transform_ffn_fused(Pd, cache, words=indices)
        D, T = int(Pd.shape[1]), int(Pd.shape[2])
        # (a share of generic words materialises: the pipeline of generic words is asked for with
        # the D its virtual rows are formed for, and they are formed for the whole word list)
        fused = None if callbacks or ffn else self._fused(
            T, indices=indices, D=D if indices is None else None, ragged=ragged is not None)
        if fused is not None and len(self._iss) > 1:
            return self._transform_chain_fused(Pd, cache)
        if fused is not None:
            Vd = Pd
            if getattr(iss, "_has_generic", False):
                # generic words over Reals / Arctic: still ONE walk + sieve launch, on the virtual rows
                # formed from the prepared input (no in-launch preparation)
                low, _ = iss._lowered(range(len(iss.words)), D)
                Vd = iss.virtual_rows(Pd, low)
            fused.ensure_preparation(int(Vd.shape[1]))     # (prepared input: nothing to fuse)
            # (an unweighted plan - every lowered one - takes no lookup: none is computed)
            weighted = fused.plan.weighting != nat.FR_W_NONE
            lookup = with_lengths(iss.lookup_device, Pd, lengths=lengths) if weighted else None
            return self._launch(fused, Vd, lookup, cache, ragged)
        rows = (range(self.niteratedsums()) if indices is None
                else self._rows_of_words(iss, indices))
        t = nat.torch()
        per_sum = sum(sieve.nfeatures() for sieve in self._sieves)
        feats = t.zeros((int(Pd.shape[0]), len(rows) * per_sum), dtype=t.float64, device=Pd.device)
        col = 0
        for row, itsum in zip(rows, self._iterate_iss_device(Pd, lengths=lengths, indices=indices)):
            for cb in callbacks:
                cb.on_iterated_sum(nat.to_host(itsum))
            sieves = self._sieves_extended[row] if self._sieves_extended else self._sieves
            for sieve in sieves:
                sieve._cache = cache
                nf = sieve.nfeatures()
                with_lengths(sieve.transform_device, itsum, feats, col, lengths=lengths)
                for cb in callbacks:
                    cb.on_sieve(nat.to_host(feats[col:col + nf]))
                col += nf
        return feats

    def _launch(self, pipe, Xin, lookup, cache, ragged=None, auto_prepare: bool = True):
        """One fused launch of ``pipe`` on ``Xin`` - the raw batch, the prepared input, a row of a
        chain, the copies of an ffn word - behind its per-call set-up: the per-batch tables and
        the pipeline's own kernels.  ``ragged``: (lengths, their int32 device copy)."""
        N, T = int(Xin.shape[0]), int(Xin.shape[2])
        if ragged is not None:
            # (never _auto_prepare: a pipeline with per-series cuts has no compiled instance)
            self._arm_lengths(pipe, *ragged)
        else:
            self._arm_series_cuts(pipe, N, T, cache)
            if auto_prepare:
                self._auto_prepare(pipe, N, T)
        return pipe.run(Xin, lookup)

    def _transform_chain_fused(self, Pd, cache):
        """Chained ISS (fruits/fruit.py:440-454): the rows of the chain in front of the last ISS
        are materialised one word batch at a time, and every one of them goes through ONE fused
        launch of the last ISS + the sieves (that row's thresholds) - K_chain launches instead of
        K_chain x K_last x |sieves|, and no (K_chain x K_last, N, T) tensor."""
        t = nat.torch()
        N, T = int(Pd.shape[0]), int(Pd.shape[2])
        last = self._iss[-1]
        width = last.n_iterated_sums() * sum(sv.nfeatures() for sv in self._sieves)
        feats = t.empty((N, self.nfeatures()), dtype=t.float64, device=Pd.device)
        for r, Xin in enumerate(self._iterate_iss_device(Pd, 0, upto=len(self._iss) - 1)):
            pipe = self._fused(T, chain_row=r)
            pipe.ensure_preparation(1)
            feats[:, r * width:(r + 1) * width] = self._launch(
                pipe, Xin, last.lookup_device(Xin), cache, auto_prepare=False)
        return feats

    def _transform_ffn_fused(self, Pd, cache, words=None):
        """CosWISS with the randomised ffn (fruits/iss/cos.py:93-137): every (word, frequency)
        reads its own transformed copy of the input, so the slice runs word by word - the F copies
        of a word (coswiss_ffn) go through ONE fused launch of that word's units and the sieves
        (pipeline over the word alone, its rows' thresholds): W launches, and neither the
        (W x F, N, T) iterated sums nor a sieve pass over them.  ``words``: only these (a rank's
        share of a word-sharded slice), their column blocks in that order."""
        t = nat.torch()
        iss = self._iss[0]
        N, D, T = (int(v) for v in Pd.shape)
        F = len(iss._freqs)
        width = F * sum(sv.nfeatures() for sv in self._sieves)
        words = list(range(len(iss.words))) if words is None else list(words)
        feats = t.empty((N, len(words) * width), dtype=t.float64, device=Pd.device)
        Z = t.empty((F, N, D, T), dtype=t.float64, device=Pd.device)
        for slot, w in enumerate(words):
            pipe = self._fused(T, indices=(w,))
            if pipe.plan.max_dim > D:
                raise IndexError(f"a word references dimension {pipe.plan.max_dim} but "
                                 f"the input has only {D}")
            for f in range(F):
                nat.coswiss_ffn(Pd, iss._A[w, f], iss._b[w, f], iss._C[w, f], Z[f])
            nat.check(nat.lib().fr_coswiss_set_input_stride(pipe.plan._h, N * D * T))
            feats[:, slot * width:(slot + 1) * width] = self._launch(pipe, Z[0], None, cache,
                                                                     auto_prepare=False)
        return feats

    def fit_transform(self, X: np.ndarray, lengths=None) -> np.ndarray:
        self.fit(X, lengths=lengths)
        return self.transform(X, lengths=lengths)

    # ---- introspection ------------------------------------------------------
    def summary(self) -> str:
        def line(s: str) -> str:
            return f"{s: <38}"

        rows = [f"{f'FruitSlice -> {self.nfeatures()}': ^38}", 38 * "-",
                line(f"Preparateurs ({len(self._preparateurs)}):")]
        text = "\n".join(rows) + "\n"
        text += "\n".join(line(f"    + {p}") for p in self._preparateurs)
        if not self._preparateurs:
            text += 38 * " "
        text += "\n" + line(f"ISS Calculators ({len(self._iss)}):")
        if not self._iss:
            text += 38 * " "
        for iss in self._iss:
            text += "\n" + line(f"    + {iss} -> {iss.n_iterated_sums()}")
            text += "\n" + line(f"       | words: {len(iss.words)}")
            text += "\n" + line(f"       | semiring: {iss.semiring.__class__.__name__}")
            wname = "None" if iss.weighting is None else iss.weighting.__class__.__name__
            text += "\n" + line(f"       | weighting: {wname}")
        if not self._iss:
            text += "\n"
        text += "\n" + line(f"Sieves ({len(self._sieves)}):")
        if not self._sieves:
            text += "\n" + 38 * " "
        for sv in self._sieves:
            text += "\n" + line(f"    + {sv.__class__.__name__} -> {sv.nfeatures()}")
        return text

    def copy(self) -> "FruitSlice":
        dup = FruitSlice()
        dup.add(*self._preparateurs, *self._iss, *self._sieves)
        return dup

    def deepcopy(self) -> "FruitSlice":
        dup = FruitSlice()
        for seed in (*self._preparateurs, *self._iss, *self._sieves):
            dup.add(seed.copy())
        dup.fit_sample_size = self.fit_sample_size
        return dup

    def label(self, index: int,
              level: Literal["prepared", "iterated sums", "features"] = "features",
              verbose: Literal[1, 2] = 1) -> str:
        def short(label: str, sep: str) -> str:
            return label.split(sep)[0] if verbose == 1 else label

        if level == "prepared":
            parts = [short(p.label(), "(") for p in self._preparateurs[:index + 1]]
            return " -> ".join(parts) if parts else "input"
        text = " -> ".join(short(p.label(), "(") for p in self._preparateurs)
        if text:
            text += " | "
        findex = 0
        if level == "features":
            per_sum = int(np.sum([s.nfeatures() for s in self._sieves]))
            index, findex = map(int, divmod(index, per_sum))
        remaining = self.niteratedsums()
        words = []
        for iss in self._iss:
            k = iss.n_iterated_sums()
            words.append(short(iss.label(int((index % remaining) // (remaining / k))), " : "))
            remaining /= k
        text += " -> ".join(words)
        if level == "iterated sums":
            return text if text else "input"
        if text:
            text += " | "
        for sieve in self._sieves:
            if findex < sieve.nfeatures():
                return text + sieve.label(findex)
            findex -= sieve.nfeatures()
        raise RuntimeError("Feature index out of range")


def _stage_verbs(stage: str, accepts: type, one: str, many: str) -> None:
    """add_<one> / get_<many> / clear_<many> of one stage of a slice."""
    def add(self, seed) -> None:
        self._put(stage, accepts, seed)

    def get(self) -> list:
        return self._stage[stage]

    def clear(self) -> None:
        self._wipe(stage)

    for verb, fn in ((f"add_{one}", add), (f"get_{many}", get), (f"clear_{many}", clear)):
        fn.__name__ = fn.__qualname__ = verb
        setattr(FruitSlice, verb, fn)


for _row in _STAGES:
    _stage_verbs(*_row)

