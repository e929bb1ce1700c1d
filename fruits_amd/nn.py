"""Differentiable iterated sums: device tensor in, device tensor out (not in the reference).

``iss(X, words, mode)`` and ``ISSLayer(words, mode)`` compute the Reals iterated sums of
``SimpleWord``s, unweighted, of a ``torch.float64`` batch ``(N, D, T)`` that lives on the GPU,
and carry a gradient back to ``X``.  The forward pass is ``ISS(words, mode).transform_device``
itself - the same plan, the same launch - and returns its ``(K, N, T)`` buffer as an
``(N, K, T)`` view.  Only ``X`` is kept for the backward pass, which recomputes the iterated
sums of every prefix with one more walk and runs the adjoint recursion of DESIGN.md 4.14
(``fr_iss_backward``, csrc/kernels_grad.hip).  Nothing goes through the host.

``max_iss(X, words, mode, semiring=...)`` and ``MaxISSLayer(words, mode, semiring=...)`` are the
same for the two max semirings, ``Arctic()`` (max, +) and ``Bayesian()`` (max, x), unweighted:
the gradient flows through the arg-max of every running maximum, of equal maxima through the
FIRST (the tie rule of ``Arctic(argmax=True)``), and is a segmented suffix sum between the
positions where a running maximum rises (``fr_iss_backward_max``).

``weighted_iss(X, words, mode, weighting=...)`` and ``WeightedISSLayer(words, mode,
weighting=...)`` are the Reals iterated sums with an exponential time penalty, total or not, for
the weightings whose lookup does not depend on the input (``Indices``, ``Plateaus``).  Their
backward pass forms the sums the forward pass carries from letter to letter itself, with a prefix
scan per inner node of the trie, instead of a second walk (DESIGN.md 4.14.2,
``fr_iss_backward_weighted``).

``pathlen_iss(X, words, mode, weighting=...)`` and ``PathLengthISSLayer`` are the same for ``L1``
and ``L2``, whose lookup is the normalised cumulative path length of ``X`` itself: the backward
pass arms the weighted entry (``fr_plan_set_grad_pathlen``), which then gathers the derivative
with respect to the lookup over the trie and carries it through the path length into dimension 0
(DESIGN.md 4.14.8).  No ``lengths=``.

``iss_features(X, words, mode, sieves, semiring=..., weighting=...)`` and ``FeatureLayer`` return
what a classifier is fed instead of the rows: the ``END`` / ``MAX`` / ``MIN`` features of every
iterated sum, ``(N, K * F)`` in ``Fruit``'s column order, for any of the three configurations
above.  Each such feature is one element of one row, so the backward pass is handed the position
of that element and the feature's gradient - a sparse upstream (DESIGN.md 4.14.4,
``fr_sieve_pick``, ``fr_iss_backward_picked``) - and no ``(N, K, T)`` tensor outlives the call.

``iss_band_features(X, words, mode, sieves, semiring=..., weighting=...)`` and ``BandFeatureLayer``
are the same for the heads that are no selection: ``MPI`` (``inc`` 0 ... 8) and ``CUR`` / ``AVG`` /
``STD``, beside ``END`` / ``MAX`` / ``MIN``.  Their upstream with respect to a row is dense, but a
closed-form function of the row: one kernel forms every head (``fr_sieve_heads``), one expands
the feature gradients into the rows' gradient just before the dense adjoint reads it
(``fr_sieve_heads_adjoint``); only ``X`` and an int32 per feature are kept.

``cos_iss(X, words, freqs, exponent, total_weighting)`` and ``CosWISSLayer`` are the cosine
weighted sums of ``CosWISS``, ``(N, W * F, T)`` with the bits of ``CosWISS.transform_device``.
Their backward pass hands the CosWISS plan itself to ``fr_iss_backward`` (DESIGN.md 4.14.7,
csrc/kernels_grad_cos.hip): per (series, word, frequency) a workgroup recomputes the factorised
forward recursion and runs its adjoint, ``exponent + 1`` suffix scans per letter; a large batch
runs in blocks of series, which changes no bit.  No ``lengths=``: the angle is a function of ``T``.

PER-SERIES LENGTHS.  The three dense entries and the four layers' ``forward``
take ``lengths=``, an integer array or tensor ``(N,)`` with ``1 <= lengths[n] <= T``
(``fruits_amd.lengths.check_lengths``): series ``n`` is ``X[n, :, :lengths[n]]``, and the tail
behind it has to be finite and influences nothing.  ``Y[n, :, :L_n]`` and ``X.grad[n, :, :L_n]``
are those of the call on the truncated series, a weighted call with the ``Indices`` / ``Plateaus``
row of length ``L_n``; ``Y[n, :, L_n:]`` is unspecified finite data that carries no gradient - the
upstream gradient there is never read - and ``X.grad[n, :, L_n:]`` is ``+0.0``.  The features of
series ``n`` are those of the truncated series (``END`` wraps by ``L_n``, ``MAX`` / ``MIN``
segments end at ``L_n``); their functional form is ``iss_features_ragged`` (the band features':
``iss_band_features_ragged``), their layer takes the lengths in ``forward`` - lengths belong to
a batch, not to a module.  The lengths are
validated on the host: a device tensor costs one download (and a synchronisation) per call.
Lengths that all equal ``T`` take the dense path, ``lengths=None`` is untouched.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _native as nat
from .iss.cos import CosWISS
from .iss.iss import ISS, ISSMode, _device_budget_bytes
from .iss.semiring import Arctic, Bayesian, Reals
from .iss.words.word import SimpleWord
from .lengths import check_lengths
from .sieving import AVG, CUR, END, MAX, MIN, MPI, STD

__all__ = ["iss", "ISSLayer", "max_iss", "MaxISSLayer", "weighted_iss", "WeightedISSLayer",
           "pathlen_iss", "PathLengthISSLayer", "cos_iss", "CosWISSLayer",
           "iss_features", "iss_features_ragged", "FeatureLayer",
           "iss_band_features", "iss_band_features_ragged", "BandFeatureLayer",
           "backward_calls"]

_calls = {"backward": 0}
_OPS: dict = {}      # the functional form's ISS objects by (word strings, mode, device), oldest first
_OPS_KEPT = 8


def backward_calls() -> int:
    """Backward passes launched by this process so far (one ``fr_iss_backward``,
    ``fr_iss_backward_max``, ``fr_iss_backward_weighted`` or ``fr_iss_backward_picked`` each - the
    band features run one of the first three -; a ``cos_iss`` backward pass counts once however
    many series blocks it ran in)."""
    return _calls["backward"]


def _check_words(op: ISS) -> None:
    """The tail every configuration check shares."""
    op._check_supported()
    if op._has_generic:
        raise NotImplementedError(
            "generic words have no backward pass: only words of SimpleWord letters have")


def _check_config(op: ISS) -> None:
    """The refusals that depend on the configuration alone: raised before any launch."""
    if isinstance(op, CosWISS):
        raise NotImplementedError("CosWISS has no backward pass here: only the unweighted Reals ISS has "
                                  "(the cosine weighted sums are nn.cos_iss / nn.CosWISSLayer)")
    if op.weighting is not None:
        raise NotImplementedError(
            f"a weighting ({type(op.weighting).__name__}) has no backward pass here: the weighted "
            "Reals iterated sums are nn.weighted_iss / nn.WeightedISSLayer")
    if not isinstance(op.semiring, Reals):
        raise NotImplementedError(
            f"the semiring {type(op.semiring).__name__} has no backward pass: only Reals has")
    _check_words(op)


def _check_max_config(op: ISS) -> None:
    """``_check_config`` for ``max_iss``: raised before any launch."""
    if isinstance(op, CosWISS):
        raise NotImplementedError("CosWISS has no backward pass here: only the unweighted ISS has "
                                  "(the cosine weighted sums are nn.cos_iss / nn.CosWISSLayer)")
    if isinstance(op.semiring, Reals):
        raise NotImplementedError(
            "max_iss differentiates the max semirings Arctic and Bayesian: the Reals iterated "
            "sums are nn.iss / nn.ISSLayer")
    if not isinstance(op.semiring, (Arctic, Bayesian)):
        raise NotImplementedError(
            f"the semiring {type(op.semiring).__name__} has no backward pass: only Reals, Arctic "
            "and Bayesian have")
    if op._argmax:
        raise NotImplementedError(
            "Arctic(argmax=True) has no backward pass: its position rows are piecewise constant "
            "- differentiate Arctic() instead")
    if op.weighting is not None:
        raise NotImplementedError(
            f"a weighting ({type(op.weighting).__name__}) has no backward pass yet: only the "
            "unweighted ISS has")
    _check_words(op)


def _check_weighted_config(op: ISS) -> None:
    """``_check_config`` for ``weighted_iss``: raised before any launch."""
    if isinstance(op, CosWISS):
        raise NotImplementedError("CosWISS has no backward pass here: only the trie walk's ISS has "
                                  "(the cosine weighted sums are nn.cos_iss / nn.CosWISSLayer)")
    if op.weighting is None:
        raise NotImplementedError(
            "weighted_iss differentiates a weighted ISS: the unweighted iterated sums are "
            "nn.iss / nn.ISSLayer")
    if not op.weighting._supports_lengths():
        raise NotImplementedError(
            f"the lookup of the weighting {type(op.weighting).__name__} depends on the input, and "
            "the gradient would have to flow through it too: only weightings whose lookup is a "
            "function of the time step alone (Indices, Plateaus) have a backward pass")
    if not isinstance(op.semiring, Reals):
        raise NotImplementedError(
            f"the semiring {type(op.semiring).__name__} has no weighted backward pass: only "
            "Reals has")
    _check_words(op)


def _check_input(op: ISS, X) -> None:
    """The refusals that depend on the input: raised before any launch, the device last."""
    if not isinstance(X, torch.Tensor):
        raise TypeError(f"X has to be a torch.Tensor, not {type(X).__name__}")
    if X.dim() != 3:
        raise TypeError(f"X has to have the shape (N, D, T), not {X.dim()} dimensions")
    if X.dtype != torch.float64:
        raise TypeError(f"X has to be torch.float64, not {X.dtype}")
    if len(op.words) > 0:
        plan = op._plan(0, len(op.words))
        if plan.max_dim > X.shape[1]:
            raise IndexError(f"a word references dimension {plan.max_dim} but the input has "
                             f"only {X.shape[1]}")
    if not X.is_cuda:
        raise TypeError(f"X has to live on the GPU, not on {X.device}: nothing here goes "
                        "through the host")


def _ragged_lengths(lengths, N: int, T: int) -> Optional[np.ndarray]:
    """``lengths`` of a batch ``(N, D, T)`` validated on the host (``check_lengths``: its errors)
    as an int64 array - or None where the batch is dense: no lengths, or all equal to ``T``.  A
    torch tensor is brought to the host first: one download for a device tensor."""
    if lengths is None:
        return None
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().numpy()
    L = check_lengths(lengths, N, T)
    return None if N == 0 or bool((L == T).all()) else L


def _prefix_program(op: ISS):
    """(plan, row_prefix): the plan whose words are the distinct prefixes of the words, each with
    depth 1 (row j = the iterated sum of prefix j; the construction CosWISS._program uses for
    its terms), and per output row of ``op`` the prefix it is the iterated sum of.  Kept with
    the ISS's other device programs.

    A weighted ISS: the distinct (letters, alphas) prefixes, each with its slice of the alphas -
    two words with the same letters and other alphas are other nodes, as in the plan compiler's
    trie - and per output row the prefix with the alphas of the word that emits the row."""
    weighted = op.weighting is not None
    if weighted:
        wmode = nat.FR_W_TOTAL if op.weighting.total else nat.FR_W_NONTOTAL
        # (found by what the program is a function of besides the letters, as ISS._plan_indices does)
        key = ("grad_weighted", op.mode, wmode,
               tuple(np.asarray(w.alpha, dtype=np.float32).tobytes() for w in op.words))
    else:
        key = ("grad", op.mode)
    prog = op._plans.get(key)
    if prog is not None:
        return prog
    index, tables, alphas, row_prefix = {}, [], [], []
    for i, word in enumerate(op.words):
        depth = op._depth(i)
        if depth == 0:
            continue          # (every prefix was output by an earlier word: no rows, no work)
        tab = np.asarray(word.table(), dtype=np.int32)
        alpha = np.asarray(word.alpha, dtype=np.float32) if weighted else None
        L = tab.shape[0]
        ident = ()
        for k in range(L):
            # (a prefix is its letters - a letter its exponents without trailing zeros, as the
            # plan compiler compares them - and, weighted, the bits of their alphas)
            letter = tuple(np.trim_zeros(tab[k], "b").tolist())
            ident += ((letter, alpha[k].tobytes()) if weighted else letter,)
            if ident not in index:
                index[ident] = len(tables)
                tables.append(tab[:k + 1])
                if weighted:
                    alphas.append(alpha[:k + 1])
            if L - k <= depth:
                row_prefix.append(index[ident])
    if weighted:
        plan = nat.Plan(tables, [1] * len(tables), alphas, wmode)
    else:
        plan = nat.Plan(tables, [1] * len(tables), None, nat.FR_W_NONE,
                        arctic=isinstance(op.semiring, Arctic), bayesian=isinstance(op.semiring, Bayesian))
    if plan.nodes != len(tables):
        raise NotImplementedError("the prefix trie of these words is too deep for the walk's "
                                  "register frames: no backward pass")
    prog = op._plans[key] = (plan, np.asarray(row_prefix, dtype=np.int32))
    return prog


_weighted_prefix_program = _prefix_program      # (the name the weighted sums' callers know it by)


class _ISSFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, op, lengths=None):
        Xc = X.contiguous()
        if lengths is not None and op.weighting is not None:
            # (row n of the lookup: the weighting's row for a series of lengths[n] steps)
            Y = op.transform_device(Xc, lookup_d=op.lookup_device(Xc, lengths))
        else:
            # (the iterated sums are causal: the padded walk is the ragged one below each end)
            Y = op.transform_device(Xc)          # (K, N, T)
        ctx.op = op
        ctx.lengths = lengths                # (host; None: dense)
        # (a ragged batch keeps its (N,) int32 device lengths beside X; a dense one X alone)
        ctx.save_for_backward(Xc, *(() if lengths is None else (nat.to_device(lengths, dtype=np.int32),)))
        return Y.permute(1, 0, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        Xc, len_d = (*ctx.saved_tensors, None)[:2]
        op = ctx.op
        plan, row_prefix = _prefix_program(op)
        with torch.cuda.device(Xc.device):
            if op.weighting is not None:
                # (the lookup is a function of T - and the lengths - alone: formed again, not kept;
                # the prefix plan itself never runs - the entry forms the carried sums - so it need
                # not fit the LDS)
                lookup = op.lookup_device(Xc, ctx.lengths)
                _calls["backward"] += 1
                return nat.iss_backward_weighted(plan, Xc, lookup, G, row_prefix, lengths_d=len_d), None, None
            S = plan.run(Xc, None, layout="KNT")          # (prefixes, N, T), dies with this call
            _calls["backward"] += 1
            # (a max semiring: the rises of the recomputed running maxima are the segments' heads)
            entry = nat.iss_backward if isinstance(op.semiring, Reals) else nat.iss_backward_max
            return entry(plan, Xc, S, G, row_prefix, lengths_d=len_d), None, None


def _apply(op: ISS, X, lengths=None):
    _check_input(op, X)
    # (an unweighted backward pass runs the prefix plan: it has to fit a workgroup's LDS)
    if op.weighting is None and len(op.words) > 0 and not _prefix_program(op)[0].fits(int(X.shape[2])):
        raise NotImplementedError("the words name more input dimensions than a workgroup stages")
    lengths = _ragged_lengths(lengths, int(X.shape[0]), int(X.shape[2]))
    with torch.cuda.device(X.device):
        return _ISSFunction.apply(X, op, lengths)


def _cached_op(key, make) -> ISS:
    """The functional forms keep their device programs between calls (a training loop calls them
    every step): the ISS of the last few plain configurations, found by ``key`` (None: not kept)."""
    op = _OPS.get(key) if key is not None else None
    if op is None:
        op = make()
        if key is not None:
            if len(_OPS) >= _OPS_KEPT:
                _OPS.pop(next(iter(_OPS)))
            _OPS[key] = op
    return op


class _Layer(torch.nn.Module):
    """What the three layers share: a module without parameters around one ISS (``check``: its
    configuration check), which keeps its device programs between calls."""

    def __init__(self, op: ISS, check) -> None:
        super().__init__()
        self.op = op
        check(op)

    @property
    def words(self):
        return self.op.words

    @property
    def mode(self) -> ISSMode:
        return self.op.mode

    def forward(self, X, lengths=None):
        return _apply(self.op, X, lengths)

    def extra_repr(self) -> str:
        return f"{len(self.op.words)} words, {self.op.mode.name}"


# ----------------------------------------------------------------------- Reals, unweighted
def _reals_op(X, words, mode, semiring, weighting) -> ISS:
    """The ISS of an ``iss`` call: ``words`` itself if it is one, else kept between calls."""
    if isinstance(words, ISS):
        return words
    words = list(words)
    key = None
    if X is not None and semiring is None and weighting is None and all(isinstance(w, SimpleWord) for w in words):
        # (found by the words' strings; a plan's tables live on one device; no X: a layer's own)
        key = (tuple(str(w) for w in words), mode, str(getattr(X, "device", None)))
    return _cached_op(key, lambda: ISS(words, mode=mode, semiring=semiring, weighting=weighting))


def iss(X, words, mode: ISSMode = ISSMode.SINGLE, *, semiring=None, weighting=None, lengths=None):
    """Iterated sums ``(N, K, T)`` of the device tensor ``X`` ``(N, D, T)``, in the row order of
    ``ISS(words, mode).transform(X)`` and with its bits; differentiable with respect to ``X``.
    ``words`` may also be an ``ISS`` that carries the configuration.  ``lengths``: per-series
    lengths ``(N,)`` (the module's docstring): ``Y[n, :, :L_n]`` and ``X.grad[n, :, :L_n]`` are
    those of the truncated series, ``X.grad[n, :, L_n:]`` is ``+0.0``."""
    op = _reals_op(X, words, mode, semiring, weighting)
    _check_config(op)
    return _apply(op, X, lengths)


class ISSLayer(_Layer):
    """``iss`` as a module without parameters; keeps its device programs between calls."""

    def __init__(self, words: Sequence, mode: ISSMode = ISSMode.SINGLE, *, semiring=None,
                 weighting=None) -> None:
        super().__init__(words if isinstance(words, ISS) else
                         ISS(list(words), mode=mode, semiring=semiring, weighting=weighting), _check_config)


# ----------------------------------------------------------------------- the max semirings
def _max_op(words, mode, semiring) -> ISS:
    if isinstance(words, ISS):
        if semiring is not None and type(semiring) is not type(words.semiring):
            raise TypeError(f"the ISS carries {type(words.semiring).__name__}, not "
                            f"{type(semiring).__name__}")
        return words
    if semiring is None:
        raise TypeError("max_iss needs semiring=Arctic() or semiring=Bayesian()")
    return ISS(list(words), mode=mode, semiring=semiring)


def _cached_max_op(X, words, mode, semiring) -> ISS:
    """``_max_op``, kept between calls like ``nn.iss`` keeps its plain case."""
    key = None
    if not isinstance(words, ISS) and X is not None:
        words = list(words)
        # (an argmax Arctic is refused by the configuration check)
        plain = type(semiring) is Bayesian or (type(semiring) is Arctic and not semiring._argmax)
        if plain and all(isinstance(w, SimpleWord) for w in words):
            key = ("max", type(semiring).__name__, tuple(str(w) for w in words), mode,
                   str(getattr(X, "device", None)))
    return _cached_op(key, lambda: _max_op(words, mode, semiring))


def max_iss(X, words, mode: ISSMode = ISSMode.SINGLE, *, semiring=None, lengths=None):
    """Arctic (max, +) or Bayesian (max, x) iterated sums ``(N, K, T)`` of the device tensor ``X``
    ``(N, D, T)``, in the row order of ``ISS(words, mode, semiring=semiring).transform(X)`` and
    with its bits; differentiable with respect to ``X``.  ``semiring``: an ``Arctic()`` or a
    ``Bayesian()``; or ``words`` is an ``ISS`` that carries one.

    Row ``w`` at time ``t`` is ``max over i_1 <= ... <= i_p <= t of m_1[i_1] (x) ... (x) m_p[i_p]``
    with ``m_k`` the value of letter k; the gradient is that of the term at the maximiser.  Of
    equal maxima the first wins at every letter - the maximiser whose reversed index tuple
    ``(i_p, ..., i_1)`` is lexicographically smallest, the rule of ``Arctic(argmax=True)`` - which
    is a valid subgradient at a tie.  For Bayesian this holds on positive inputs; where ``X`` has
    negative values the reference's recursion (a running maximum per letter) is not the maximum
    over index tuples, and the gradient is that of the recursion as the reference defines it.
    ``lengths``: per-series lengths ``(N,)``, as ``iss`` takes them."""
    op = _cached_max_op(X, words, mode, semiring)
    _check_max_config(op)
    return _apply(op, X, lengths)


class MaxISSLayer(_Layer):
    """``max_iss`` as a module without parameters; keeps its device programs between calls."""

    def __init__(self, words: Sequence, mode: ISSMode = ISSMode.SINGLE, *, semiring=None) -> None:
        super().__init__(_max_op(words, mode, semiring), _check_max_config)

    @property
    def semiring(self):
        return self.op.semiring

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, {type(self.op.semiring).__name__}"


# ----------------------------------------------------------------------- weighted Reals
def _weighted_op(words, mode, weighting) -> ISS:
    if isinstance(words, ISS):
        if weighting is not None and weighting is not words.weighting:
            raise TypeError("the ISS carries its own weighting")
        return words
    return ISS(list(words), mode=mode, weighting=weighting)


def _cached_weighted_op(X, words, mode, weighting) -> ISS:
    """``_weighted_op``, kept between calls like ``nn.iss`` keeps its plain case."""
    key = None
    if not isinstance(words, ISS) and X is not None:
        words = list(words)
        # (the ISS holds the weighting, so its id names it for as long as the entry lives)
        if weighting is not None and all(isinstance(w, SimpleWord) for w in words):
            key = ("weighted", id(weighting), tuple(str(w) for w in words),
                   tuple(np.asarray(w.alpha, dtype=np.float32).tobytes() for w in words), mode,
                   str(getattr(X, "device", None)))
    return _cached_op(key, lambda: _weighted_op(words, mode, weighting))


def weighted_iss(X, words, mode: ISSMode = ISSMode.SINGLE, *, weighting=None, lengths=None):
    """Weighted Reals iterated sums ``(N, K, T)`` of the device tensor ``X`` ``(N, D, T)``, in the
    row order of ``ISS(words, mode, weighting=weighting).transform(X)`` and with its bits;
    differentiable with respect to ``X``.  ``weighting``: an ``Indices`` or a ``Plateaus``, total or
    not - the weightings whose lookup does not depend on ``X``; or ``words`` is an ``ISS`` that
    carries one.  The letters' alphas are the words' (``word.alpha``).

    The backward pass is ``fr_iss_backward_weighted``: it forms the sums the
    forward pass carries from letter to letter with a prefix scan per inner trie node, then the
    adjoint with suffix scans, the exp factors ``exp(+-g alpha)`` as constants.
    ``lengths``: per-series lengths ``(N,)``, as ``iss`` takes them; series ``n`` is weighted with
    the ``Indices`` / ``Plateaus`` row of a series of ``L_n`` steps, forward and backward."""
    op = _cached_weighted_op(X, words, mode, weighting)
    _check_weighted_config(op)
    return _apply(op, X, lengths)


class WeightedISSLayer(_Layer):
    """``weighted_iss`` as a module without parameters; keeps its device programs between calls."""

    def __init__(self, words: Sequence, mode: ISSMode = ISSMode.SINGLE, *, weighting=None) -> None:
        super().__init__(_weighted_op(words, mode, weighting), _check_weighted_config)

    @property
    def weighting(self):
        return self.op.weighting

    def extra_repr(self) -> str:
        return (f"{super().extra_repr()}, "
                f"{type(self.op.weighting).__name__}{' total' if self.op.weighting.total else ''}")


# ----------------------------------------------------------------------- weighted with the path length
_PATHLEN_NO_LENGTHS = ("lengths= is not taken here: the forward L1 / L2 lookup takes no lengths - the path "
                       "length of a truncated series is normalised by another total")


def _check_pathlen_config(op: ISS) -> None:
    """``_check_config`` for ``pathlen_iss``: raised before any launch."""
    from .iss.weighting import _PathLength
    if isinstance(op, CosWISS):
        raise NotImplementedError("CosWISS has no backward pass here: only the trie walk's ISS has "
                                  "(the cosine weighted sums are nn.cos_iss / nn.CosWISSLayer)")
    w = op.weighting
    if w is None:
        raise NotImplementedError(
            "pathlen_iss differentiates an ISS weighted with L1 or L2: the unweighted iterated sums are "
            "nn.iss / nn.ISSLayer")
    if w._supports_lengths():
        raise NotImplementedError(
            f"the lookup of the weighting {type(w).__name__} is a function of the time step alone: its "
            "backward pass is nn.weighted_iss / nn.WeightedISSLayer")
    if not isinstance(w, _PathLength):
        raise NotImplementedError(
            f"the lookup of the weighting {type(w).__name__} is an arbitrary callable of the input, which "
            "has no derivative here: only L1 and L2 have a gradient through the lookup")
    if w._transform is not None:
        raise NotImplementedError(
            f"{type(w).__name__}(transform=...) applies a Python callable to the path length, which has no "
            "derivative here: only the plain L1 and L2 have a gradient through the lookup")
    if not isinstance(op.semiring, Reals):
        raise NotImplementedError(
            f"the semiring {type(op.semiring).__name__} has no weighted backward pass: only "
            "Reals has")
    _check_words(op)


def _pathlen_lookup(op: ISS, Xc):
    """The ``(N, T)`` lookup of ``Xc`` itself, as the Reals forward pass forms it: here the one
    tensor is the raw and the prepared input, so ``on_prepared`` changes nothing."""
    w = op.weighting
    return nat.pathlen_lookup(Xc, w._norm, 1 if w._relative else 0, float(w._scale), exact=False)


class _PathLengthFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, op):
        Xc = X.contiguous()
        Y = op.transform_device(Xc, lookup_d=_pathlen_lookup(op, Xc))          # (K, N, T)
        ctx.op = op
        ctx.save_for_backward(Xc)
        return Y.permute(1, 0, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        (Xc,) = ctx.saved_tensors
        op = ctx.op
        plan, row_prefix = _prefix_program(op)
        with torch.cuda.device(Xc.device):
            # (the lookup is formed again, not kept; the armed entry carries the gradient through it)
            lookup = _pathlen_lookup(op, Xc)
            _calls["backward"] += 1
            return nat.iss_backward_weighted(plan, Xc, lookup, G, row_prefix,
                                             pathlen=(op.weighting._norm, float(op.weighting._scale))), None


def _apply_pathlen(op: ISS, X, lengths=None):
    if lengths is not None:
        raise NotImplementedError(_PATHLEN_NO_LENGTHS)
    _check_input(op, X)
    with torch.cuda.device(X.device):
        return _PathLengthFunction.apply(X, op)


def pathlen_iss(X, words, mode: ISSMode = ISSMode.SINGLE, *, weighting=None, lengths=None):
    """Reals iterated sums ``(N, K, T)`` of the device tensor ``X`` ``(N, D, T)`` weighted with the
    path length of ``X`` itself, in the row order of ``ISS(words, mode, weighting=weighting)
    .transform(X)`` and with its bits; differentiable with respect to ``X``.  ``weighting``: an
    ``L1`` or an ``L2``, total or not, ``relative`` either way, any ``scale``; or ``words`` is an
    ``ISS`` that carries one.  The lookup ``g = scale r / r[T-1]``, ``r`` the cumulative ``|dx_0|`` or
    ``dx_0^2`` of dimension 0, is a function of ``X``: ``X.grad`` is the full derivative, the part that
    flows through ``g`` into dimension 0 included (``fr_plan_set_grad_pathlen``
    around ``fr_iss_backward_weighted``).  Where an increment of dimension 0 is exactly 0 the ``L1``
    gradient takes ``sign(0) = 0``, the subgradient of ``torch.abs``; a series whose dimension 0 is
    constant has ``g = 0`` and gets no gradient through the lookup.  ``transform=`` on the
    weighting, ``Indices`` / ``Plateaus`` / ``Custom``, a non-Reals semiring, ``CosWISS``, generic
    words and ``lengths=`` raise NotImplementedError."""
    op = _cached_weighted_op(X, words, mode, weighting)
    _check_pathlen_config(op)
    return _apply_pathlen(op, X, lengths)


class PathLengthISSLayer(_Layer):
    """``pathlen_iss`` as a module without parameters; keeps its device programs between calls."""

    def __init__(self, words: Sequence, mode: ISSMode = ISSMode.SINGLE, *, weighting=None) -> None:
        super().__init__(_weighted_op(words, mode, weighting), _check_pathlen_config)

    @property
    def weighting(self):
        return self.op.weighting

    def forward(self, X, lengths=None):
        return _apply_pathlen(self.op, X, lengths)

    def extra_repr(self) -> str:
        return (f"{super().extra_repr()}, "
                f"{type(self.op.weighting).__name__}{' total' if self.op.weighting.total else ''}")


# ----------------------------------------------------------------------- cosine weighted
_COS_NO_LENGTHS = ("lengths= is not taken here: the forward CosWISS takes no lengths, and its angle "
                   "pi (i - j) / (f (T - 1)) is a function of T - a series of another length is another "
                   "weighting, not a truncation")


def _check_cos_config(op: CosWISS) -> None:
    """The refusals of ``cos_iss`` that depend on the configuration alone: raised before any launch."""
    if not isinstance(op, CosWISS):
        raise TypeError(f"cos_iss differentiates a CosWISS, not {type(op).__name__}")
    if op._ffn_size is not None:
        raise NotImplementedError("a CosWISS with ffn_size has no backward pass: the randomised input "
                                  "transform is not differentiated")
    if op._dropout is not None:
        raise NotImplementedError("a CosWISS with dropout has no backward pass yet")
    if not op._native():
        raise NotImplementedError(
            "this CosWISS has no backward pass: the factorised kernels cover exponents 1 ... "
            f"{nat.CosPlan.MAX_EXPONENT} and words of at most {nat.CosPlan.MAX_LETTERS} letters "
            "(and FRUITS_AMD_COSWISS_TERMS=1 switches them off)")


def _cos_series_block(plan, N: int, T: int) -> int:
    """Series per backward call: what the scratch of the call (coswiss_grad_rows) may take of the
    device budget that ``word_batches`` sizes the forward pass by."""
    rows = sum(nat.coswiss_grad_rows(plan))
    return max(1, min(N, _device_budget_bytes() // max(8 * rows * T, 1)))


class _CosFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, op):
        Xc = X.contiguous()
        Y = op.transform_device(Xc)              # (W * F, N, T)
        ctx.op = op
        ctx.save_for_backward(Xc)
        return Y.permute(1, 0, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        (Xc,) = ctx.saved_tensors
        op = ctx.op
        plan = op._plan(0, len(op.words))
        N, T = int(Xc.shape[0]), int(Xc.shape[2])
        rows = np.arange(plan.rows, dtype=np.int32)
        _calls["backward"] += 1
        with torch.cuda.device(Xc.device):
            block = _cos_series_block(plan, N, T)
            if block >= N:
                return nat.iss_backward_cos(plan, Xc, G, rows), None
            # (series are independent and every sum has one association: a split changes no bit)
            dX, work = torch.empty_like(Xc), None
            for s in range(0, N, block):
                e = min(s + block, N)
                if work is None:
                    work = torch.empty((sum(nat.coswiss_grad_rows(plan)) * (e - s) * T,), dtype=torch.float64,
                                       device=Xc.device)
                dX[s:e] = nat.iss_backward_cos(plan, Xc[s:e], G[s:e], rows, work=work)
            return dX, None


def _apply_cos(op: CosWISS, X):
    _check_input(op, X)
    with torch.cuda.device(X.device):
        return _CosFunction.apply(X, op)


def _cos_op(X, words, freqs, exponent, total_weighting, ffn_size, dropout) -> CosWISS:
    if isinstance(words, CosWISS):
        return words
    words = list(words)
    key = None
    if X is not None and ffn_size is None and dropout is None and all(isinstance(w, SimpleWord) for w in words):
        key = ("cos", tuple(str(w) for w in words),
               np.asarray(freqs, dtype=np.float32).tobytes(), int(exponent), bool(total_weighting),
               str(getattr(X, "device", None)))
    return _cached_op(key, lambda: CosWISS(words, freqs, exponent=exponent, total_weighting=total_weighting,
                                           ffn_size=ffn_size, dropout=dropout))


def cos_iss(X, words, freqs=None, exponent: int = 2, total_weighting: bool = False, *, ffn_size=None,
            dropout=None, lengths=None):
    """Cosine weighted iterated sums ``(N, W * F, T)`` of the device tensor ``X`` ``(N, D, T)``, in
    the row order of ``CosWISS(words, freqs, exponent, total_weighting).transform(X)`` - word-major,
    ``F = len(freqs)`` rows per word - and with its bits; differentiable with respect to ``X``.
    ``words`` may also be a ``CosWISS`` that carries the configuration.

    The backward pass is ``fr_iss_backward`` handed the CosWISS plan: per
    (series, word, frequency) one workgroup recomputes the forward recursion and runs its adjoint,
    ``exponent + 1`` suffix scans per letter; the sin / cos tables are constants.  Its scratch is
    ``2 L - 1`` rows ``(N, T)`` per row of the result, so a large batch runs in blocks of series
    sized by the device budget (``FRUITS_AMD_ISS_GIB``) - the bits do not depend on the split.
    Exponents 1 ... 8 and words of at most 16 letters; ``ffn_size``, ``dropout`` and ``lengths=``
    raise NotImplementedError."""
    if lengths is not None:
        raise NotImplementedError(_COS_NO_LENGTHS)
    if not isinstance(words, CosWISS) and freqs is None:
        raise TypeError("cos_iss needs freqs, or a CosWISS that carries them")
    op = _cos_op(X, words, freqs, exponent, total_weighting, ffn_size, dropout)
    _check_cos_config(op)
    return _apply_cos(op, X)


class CosWISSLayer(_Layer):
    """``cos_iss`` as a module without parameters; keeps its device programs between calls."""

    def __init__(self, words: Sequence, freqs=None, exponent: int = 2, total_weighting: bool = False, *,
                 ffn_size=None, dropout=None) -> None:
        if not isinstance(words, CosWISS) and freqs is None:
            raise TypeError("CosWISSLayer needs freqs, or a CosWISS that carries them")
        super().__init__(_cos_op(None, words, freqs, exponent, total_weighting, ffn_size, dropout),
                         _check_cos_config)

    def forward(self, X, lengths=None):
        if lengths is not None:
            raise NotImplementedError(_COS_NO_LENGTHS)
        return _apply_cos(self.op, X)

    def extra_repr(self) -> str:
        op = self.op
        return (f"{len(op.words)} words, {len(op._freqs)} frequencies, exponent {op._exponent}"
                f"{', total' if op._total_weighting else ''}")


# ----------------------------------------------------------------------- features of the rows
_PICK_MAX_FEATURES = 256      # features of a row (csrc/kernels.h, kPickMaxFeatures)


def _check_sieves(sieves, band: bool = False) -> list:
    """The refusals that depend on the sieves alone: raised before any launch.  What remains is
    END, MAX and MIN with integer cuts - the sieves whose feature is ONE element of the row - and,
    for the band features (``band``), MPI with inc 0 ... 8 and CUR / AVG / STD beside them."""
    from .sieving.abstract import FeatureSieve
    if isinstance(sieves, FeatureSieve) or not isinstance(sieves, Sequence):
        raise TypeError("sieves has to be a sequence of sieves")
    sieves = list(sieves)
    if not sieves:
        raise ValueError("sieves has to name at least one sieve")
    have = "MPI, CUR, AVG, STD, END, MAX and MIN" if band else "END, MAX and MIN"
    for sieve in sieves:
        name = type(sieve).__name__
        if not isinstance(sieve, FeatureSieve):
            raise TypeError(f"sieves has to hold sieves, not {name}")
        if name in ("INC", "INT"):
            raise NotImplementedError(
                f"the sieve {sieve} has no backward pass here: the wrappers INC / INT sieve "
                f"increments or sums of the row, not the row - only {have} themselves have")
        if name in ("NPI", "XPI", "LPI", "PPV", "CPV"):
            raise NotImplementedError(
                f"the sieve {sieve} has no backward pass: {name} counts, and the gradient of a "
                "count is zero almost everywhere")
        if not band and name in ("MPI", "CUR", "AVG", "STD"):
            raise NotImplementedError(
                f"the sieve {sieve} has no backward pass here: {name} is no selection of one "
                "element of the row - only END, MAX and MIN have")
        if type(sieve) not in ((END, MAX, MIN, MPI, CUR, AVG, STD) if band else (END, MAX, MIN)):
            raise NotImplementedError(
                f"the sieve {sieve} has no backward pass: only {have} have")
        if type(sieve) is MPI and not 0 <= sieve._inc <= nat.MAX_INC:
            raise NotImplementedError(
                f"the sieve {sieve} has no backward pass: " +
                ("inc < 0 sieves cumulated rows, whose adjoint is not built - " if sieve._inc < 0 else "") +
                f"only inc 0 ... {nat.MAX_INC} has")
        if sieve._has_float_cuts():
            what = "segments depend" if name in ("MPI", "CUR", "AVG", "STD") else "position depends"
            raise NotImplementedError(
                f"the sieve {sieve} has a float (coquantile) cut: its {what} on the "
                "input's path length, which has no backward pass - only integer cuts have")
    F = sum(sieve.nfeatures() for sieve in sieves)
    if F > _PICK_MAX_FEATURES:
        raise ValueError(f"the sieves have {F} features per iterated sum: at most "
                         f"{_PICK_MAX_FEATURES} are {'formed' if band else 'picked'} in one launch")
    return sieves


def _thresholds(sieve) -> np.ndarray:
    """The sieve's sorted value thresholds, constants of the adjoint: those of its q in
    {-1, 0, 1}, or the fitted ones - what ``quantiles_device`` uploads."""
    if not sieve.requires_fitting:
        sieve._get_unfitted_quantiles()
    elif getattr(sieve, "_quantiles", None) is None:
        raise RuntimeError("Sieve has not been fitted properly")
    return np.ascontiguousarray(sieve._quantiles, dtype=np.float64)


class _Head:
    """The sieves of an ``iss_features`` call and their device tables (fr_sieve_pick), kept by
    what they are a function of: the length of the series, the thresholds, the device."""

    _check = staticmethod(_check_sieves)

    def __init__(self, sieves) -> None:
        self.sieves = self._check(sieves)
        self.F = sum(sieve.nfeatures() for sieve in self.sieves)
        self._tables: dict = {}

    def host_tables(self, T: int):
        """(spec (n_sieves, 6) int32, cuts int64, thresholds float64) for series of T steps;
        an END cut outside the series is the IndexError of ``END`` itself."""
        spec, cuts, qs, feat = [], [], [], 0
        for sieve in self.sieves:
            row = sieve._int_cut_row(T)
            q = np.zeros(0) if isinstance(sieve, END) else _thresholds(sieve)
            spec.append([sieve._kind, sum(len(c) for c in cuts), len(row),
                         sum(len(v) for v in qs), len(q), feat])
            cuts.append(row)
            qs.append(q)
            feat += sieve.nfeatures()
        return (np.asarray(spec, dtype=np.int32), np.concatenate(cuts).astype(np.int64),
                np.concatenate(qs).astype(np.float64))

    def tables(self, T: int, device):
        spec, cuts, q = self.host_tables(T)
        key = (T, str(device), q.tobytes())
        hit = self._tables.get(key)
        if hit is None:
            if len(self._tables) >= _OPS_KEPT:
                self._tables.pop(next(iter(self._tables)))
            with torch.cuda.device(device):
                hit = self._tables[key] = (spec, nat.to_device(spec, dtype=np.int32),
                                           nat.to_device(cuts, dtype=np.int64),
                                           nat.to_device(q) if len(q) else None)
        return hit

    def host_series_tables(self, lengths):
        """``host_tables`` for series of these lengths: every kind carries
        ``FR_SIEVE_SERIES_CUTS`` and the cuts are an ``(N, row)`` table - series n's row holds
        every sieve's cut row as the sieve itself resolves it for a series of ``lengths[n]``
        steps (``_series_cut_rows``: lengths.resolve_cuts, and resolve_end_cuts with END's wrap
        and its IndexError for a cut outside a series)."""
        spec, cuts, qs, feat, at = [], [], [], 0, 0
        for sieve in self.sieves:
            rows = sieve._series_cut_rows(lengths)
            q = np.zeros(0) if isinstance(sieve, END) else _thresholds(sieve)
            spec.append([sieve._kind | nat.FR_SIEVE_SERIES_CUTS, at, rows.shape[1],
                         sum(len(v) for v in qs), len(q), feat])
            cuts.append(rows)
            qs.append(q)
            at += rows.shape[1]
            feat += sieve.nfeatures()
        return (np.asarray(spec, dtype=np.int32), np.ascontiguousarray(np.concatenate(cuts, axis=1), dtype=np.int64),
                np.concatenate(qs).astype(np.float64))

    def series_tables(self, lengths, device):
        """The device tables of ``host_series_tables``.  Spec and thresholds are kept like the
        dense ones; the cut table is the batch's and dies with the call."""
        spec, cuts, q = self.host_series_tables(lengths)
        key = ("series", str(device), q.tobytes())
        with torch.cuda.device(device):
            hit = self._tables.get(key)
            if hit is None:
                if len(self._tables) >= _OPS_KEPT:
                    self._tables.pop(next(iter(self._tables)))
                hit = self._tables[key] = (spec, nat.to_device(spec, dtype=np.int32),
                                           nat.to_device(q) if len(q) else None)
            return hit[0], hit[1], nat.to_device(cuts, dtype=np.int64), hit[2]

    def __getstate__(self):
        return {"sieves": self.sieves, "F": self.F, "_tables": {}}


class _FeatureFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, op, head, lengths=None):
        Xc = X.contiguous()
        N, T = int(Xc.shape[0]), int(Xc.shape[2])
        if lengths is None:
            spec, spec_d, cuts_d, q_d = head.tables(T, Xc.device)
        else:
            # (an END cut outside a series: IndexError here, before any launch)
            spec, spec_d, cuts_d, q_d = head.series_tables(lengths, Xc.device)
        if lengths is not None and op.weighting is not None:
            Y = op.transform_device(Xc, lookup_d=op.lookup_device(Xc, lengths))
        else:
            Y = op.transform_device(Xc)          # (K, N, T): dies with this call
        feat, pos = nat.sieve_pick(Y, spec, spec_d, cuts_d, q_d, head.F)
        ctx.op = op
        ctx.lengths = lengths                # (host; None: dense)
        ctx.save_for_backward(Xc, pos, *(() if lengths is None else (nat.to_device(lengths, dtype=np.int32),)))
        return feat.view(N, -1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        Xc, pos, len_d = (*ctx.saved_tensors, None)[:3]
        op = ctx.op
        plan, row_prefix = _prefix_program(op)
        # (N, K * F), tiny: an expanded scalar or a slice is made contiguous, never dense in T
        w = g.to(device=Xc.device, dtype=torch.float64).contiguous().view(pos.shape)
        with torch.cuda.device(Xc.device):
            if op.weighting is not None:
                lookup = op.lookup_device(Xc, ctx.lengths)
                _calls["backward"] += 1
                return (nat.iss_backward_picked(plan, Xc, pos, w, row_prefix, lookup_d=lookup, lengths_d=len_d),
                        None, None, None)
            S = plan.run(Xc, None, layout="KNT")          # (prefixes, N, T), dies with this call
            _calls["backward"] += 1
            return nat.iss_backward_picked(plan, Xc, pos, w, row_prefix, Sd=S, lengths_d=len_d), None, None, None


def _feature_op(X, words, mode, semiring, weighting):
    """(ISS, its configuration check) of an ``iss_features`` call: the configuration decides which
    adjoint runs, exactly as ``iss``, ``max_iss`` and ``weighted_iss`` decide - a weighting: the
    weighted adjoint; else Arctic or Bayesian: the max adjoint; else Reals."""
    carried = words if isinstance(words, ISS) else None
    if weighting is not None or (carried is not None and carried.weighting is not None):
        if semiring is not None and not isinstance(semiring, Reals) and carried is None:
            # (no such adjoint: the weighted check names the semiring)
            return ISS(list(words), mode=mode, semiring=semiring, weighting=weighting), _check_weighted_config
        return _cached_weighted_op(X, words, mode, weighting), _check_weighted_config
    if carried is not None and semiring is None:
        semiring = carried.semiring
    if semiring is not None and not isinstance(semiring, Reals):
        return _cached_max_op(X, words, mode, semiring), _check_max_config
    return _reals_op(X, words, mode, semiring, None), _check_config


_LENGTHS_ELSEWHERE = ("lengths= is not taken here: lengths belong to a batch - pass them to the layer's call, "
                      "FeatureLayer(...)(X, lengths=...), or to nn.iss_features_ragged(X, lengths, ...)")


def _apply_features(op: ISS, head: _Head, X, lengths=None, function=_FeatureFunction):
    for sieve in head.sieves:
        if not isinstance(sieve, END):
            _thresholds(sieve)           # (an unfitted sieve: before the input is looked at)
    _check_input(op, X)
    if op.weighting is None and len(op.words) > 0 and not _prefix_program(op)[0].fits(int(X.shape[2])):
        raise NotImplementedError("the words name more input dimensions than a workgroup stages")
    if int(X.shape[2]) < 1:
        raise ValueError("the features of series without a time step are undefined")
    lengths = _ragged_lengths(lengths, int(X.shape[0]), int(X.shape[2]))
    with torch.cuda.device(X.device):
        return function.apply(X, op, head, lengths)


def iss_features(X, words, mode: ISSMode = ISSMode.SINGLE, sieves=(), *, semiring=None,
                 weighting=None, lengths=None):
    """The selecting features ``(N, K * F)`` of the iterated sums of the device tensor ``X``
    ``(N, D, T)``: what ``sieve.transform_device`` returns on each row of
    ``ISS(words, mode, ...).transform_device(X)``, with its bits, in ``Fruit``'s column order -
    iterated sum, then sieve, then the sieve's own (segment, band) order; differentiable with
    respect to ``X``.

    ``sieves``: ``END``, ``MAX`` and ``MIN`` of ``fruits_amd.sieving`` with integer cuts, with
    thresholds q in {-1, 0, 1} or fitted already - the thresholds are constants of the adjoint.
    ``semiring`` / ``weighting`` choose the iterated sums as ``iss`` (neither), ``max_iss``
    (``Arctic()``, ``Bayesian()``) and ``weighted_iss`` (``Indices``, ``Plateaus``) take them.

    A feature's gradient goes to the one element of its row that it selects: ``END`` the element
    at ``cut - 1``, ``MAX`` / ``MIN`` the FIRST step of the segment that attains the extreme
    inside the band ``q_k < v <= q_(k+1)`` (``np.argmax``'s rule, the tie rule of ``max_iss``).
    An empty segment or band is the feature 0 and carries no gradient.  Only ``X`` and the
    ``(N, K, F)`` int32 positions are kept for the backward pass, whose upstream is those
    positions with the feature gradients.

    Series of unequal lengths: ``iss_features_ragged``, or ``FeatureLayer(...)(X, lengths=...)``;
    ``lengths=`` here raises NotImplementedError."""
    if lengths is not None:
        raise NotImplementedError(_LENGTHS_ELSEWHERE)
    head = _Head(sieves)
    op, check = _feature_op(X, words, mode, semiring, weighting)
    check(op)
    return _apply_features(op, head, X)


def iss_features_ragged(X, lengths, words, mode: ISSMode = ISSMode.SINGLE, sieves=(), *, semiring=None,
                        weighting=None):
    """``iss_features`` of series of unequal lengths: ``lengths`` ``(N,)`` integers in ``1..T``,
    series ``n`` is ``X[n, :, :lengths[n]]`` and row ``n`` of the result is ``iss_features`` of that
    truncated series - ``END`` cuts wrap by ``L_n`` (one outside a series: IndexError, before any
    launch), ``MAX`` / ``MIN`` segments are clipped to ``[0, L_n]``, every selected position is
    ``< L_n``, and ``X.grad[n, :, L_n:]`` is ``+0.0``.  Lengths that all equal ``T`` take the
    dense path."""
    head = _Head(sieves)
    op, check = _feature_op(X, words, mode, semiring, weighting)
    check(op)
    return _apply_features(op, head, X, lengths)


class FeatureLayer(_Layer):
    """``iss_features`` as a module without parameters; keeps its device programs between calls."""

    def __init__(self, words: Sequence, mode: ISSMode = ISSMode.SINGLE, sieves=(), *, semiring=None,
                 weighting=None, lengths=None) -> None:
        if lengths is not None:
            raise NotImplementedError(_LENGTHS_ELSEWHERE)
        head = _Head(sieves)
        # (no X: the layer's ISS is its own, as every layer's)
        op, check = _feature_op(None, words, mode, semiring, weighting)
        super().__init__(op, check)
        self.head = head

    @property
    def sieves(self):
        return self.head.sieves

    def forward(self, X, lengths=None):
        return _apply_features(self.op, self.head, X, lengths)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, {self.head.F} features per iterated sum"


# ----------------------------------------------------------------------- band features of the rows
class _BandHead(_Head):
    """``_Head`` for fr_sieve_heads: the same tables, and the differencing order of each sieve's
    rows as a seventh spec column."""

    _check = staticmethod(lambda sieves: _check_sieves(sieves, band=True))

    def _with_orders(self, spec):
        orders = np.asarray([[sieve._inc] for sieve in self.sieves], dtype=np.int32)
        return np.ascontiguousarray(np.concatenate([spec, orders], axis=1))

    def host_tables(self, T: int):
        spec, cuts, q = super().host_tables(T)
        return self._with_orders(spec), cuts, q

    def host_series_tables(self, lengths):
        spec, cuts, q = super().host_series_tables(lengths)
        return self._with_orders(spec), cuts, q


def _row_map_device(op: ISS, row_prefix, device):
    """The device copy of the prefix program's ``row_prefix``, kept beside the program."""
    key = ("heads_row_map", op.mode, str(device))
    hit = op._plans.get(key)
    if hit is None or hit[0] is not row_prefix:
        with torch.cuda.device(device):
            hit = op._plans[key] = (row_prefix, nat.to_device(row_prefix, dtype=np.int32))
    return hit[1]


class _BandFeatureFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, op, head, lengths=None):
        Xc = X.contiguous()
        N, T = int(Xc.shape[0]), int(Xc.shape[2])
        if lengths is None:
            spec, spec_d, cuts_d, q_d = head.tables(T, Xc.device)
        else:
            # (an END cut outside a series: IndexError here, before any launch)
            spec, spec_d, cuts_d, q_d = head.series_tables(lengths, Xc.device)
        if lengths is not None and op.weighting is not None:
            Y = op.transform_device(Xc, lookup_d=op.lookup_device(Xc, lengths))
        else:
            Y = op.transform_device(Xc)          # (K, N, T): dies with this call
        feat, comp = nat.sieve_heads(Y, spec, spec_d, cuts_d, q_d, head.F)
        ctx.op, ctx.head = op, head
        ctx.lengths = lengths                # (host; None: dense)
        ctx.save_for_backward(Xc, comp, *(() if lengths is None else (nat.to_device(lengths, dtype=np.int32),)))
        return feat.view(N, -1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        Xc, comp, len_d = (*ctx.saved_tensors, None)[:3]
        op, head = ctx.op, ctx.head
        plan, row_prefix = _prefix_program(op)
        w = g.to(device=Xc.device, dtype=torch.float64).contiguous().view(comp.shape)
        with torch.cuda.device(Xc.device):
            # (the tables are kept by the head, a ragged batch's cut rows formed again)
            if ctx.lengths is None:
                tables = head.tables(int(Xc.shape[2]), Xc.device)
            else:
                tables = head.series_tables(ctx.lengths, Xc.device)
            if op.weighting is not None:
                # (the rows again, as the forward pass formed them: the same walk, the same bits)
                lookup = op.lookup_device(Xc, ctx.lengths)
                Y = op.transform_device(Xc, lookup_d=lookup)
                G = nat.sieve_heads_adjoint(Y, *tables, comp, w, lengths_d=len_d)
                del Y
                _calls["backward"] += 1
                return (nat.iss_backward_weighted(plan, Xc, lookup, G, row_prefix, lengths_d=len_d),
                        None, None, None)
            # (the backward pass's own prefix sums hold every row: read through row_prefix)
            S = plan.run(Xc, None, layout="KNT")          # (prefixes, N, T), dies with this call
            G = nat.sieve_heads_adjoint(S, *tables, comp, w, row_map=row_prefix,
                                        row_map_d=_row_map_device(op, row_prefix, Xc.device), lengths_d=len_d)
            _calls["backward"] += 1
            entry = nat.iss_backward if isinstance(op.semiring, Reals) else nat.iss_backward_max
            return entry(plan, Xc, S, G, row_prefix, lengths_d=len_d), None, None, None


_BAND_LENGTHS_ELSEWHERE = ("lengths= is not taken here: lengths belong to a batch - pass them to the layer's call, "
                           "BandFeatureLayer(...)(X, lengths=...), or to nn.iss_band_features_ragged(X, lengths, ...)")


def iss_band_features(X, words, mode: ISSMode = ISSMode.SINGLE, sieves=(), *, semiring=None,
                      weighting=None, lengths=None):
    """The features ``(N, K * F)`` of the iterated sums of the device tensor ``X`` ``(N, D, T)``
    that the heads ``sieves`` return: what ``sieve.transform_device`` returns on each row of
    ``ISS(words, mode, ...).transform_device(X)`` - ``END`` / ``MAX`` / ``MIN`` / ``MPI`` with its
    bits, ``CUR`` / ``AVG`` / ``STD`` with every square rounded -, in ``Fruit``'s column order;
    differentiable with respect to ``X``.

    ``sieves``: ``MPI`` with ``inc`` 0 ... 8, ``CUR`` / ``AVG`` / ``STD``, ``END``, ``MAX``, ``MIN``, with
    integer cuts and thresholds q in {-1, 0, 1} or fitted already - cuts and thresholds are
    constants of the adjoint.  ``semiring`` / ``weighting`` choose the iterated sums as in
    ``iss_features``.

    With ``D = E^inc row`` (``inc`` 2 for ``CUR``), an ``MPI`` feature is the mean of the ``c`` elements
    of ``D`` in its segment and band and gives each of them ``g / c``; a ``CUR`` feature is the sum of
    their squares and gives ``D[t]`` the gradient ``2 g D[t]``; both reach the row through the
    transposed differencing.  An empty band is the feature 0 and carries no gradient.  Only ``X`` and
    one int32 per feature are kept; the dense ``(N, K, T)`` gradient of the rows exists inside the
    backward call alone.

    Series of unequal lengths: ``iss_band_features_ragged``, or ``BandFeatureLayer(...)(X,
    lengths=...)``; ``lengths=`` here raises NotImplementedError."""
    if lengths is not None:
        raise NotImplementedError(_BAND_LENGTHS_ELSEWHERE)
    head = _BandHead(sieves)
    op, check = _feature_op(X, words, mode, semiring, weighting)
    check(op)
    return _apply_features(op, head, X, None, _BandFeatureFunction)


def iss_band_features_ragged(X, lengths, words, mode: ISSMode = ISSMode.SINGLE, sieves=(), *, semiring=None,
                             weighting=None):
    """``iss_band_features`` of series of unequal lengths, as ``iss_features_ragged``: row ``n`` of
    the result is ``iss_band_features`` of ``X[n, :, :lengths[n]]``, and ``X.grad[n, :, L_n:]`` is
    ``+0.0``.  Lengths that all equal ``T`` take the dense path."""
    head = _BandHead(sieves)
    op, check = _feature_op(X, words, mode, semiring, weighting)
    check(op)
    return _apply_features(op, head, X, lengths, _BandFeatureFunction)


class BandFeatureLayer(_Layer):
    """``iss_band_features`` as a module without parameters; keeps its device programs between calls."""

    def __init__(self, words: Sequence, mode: ISSMode = ISSMode.SINGLE, sieves=(), *, semiring=None,
                 weighting=None, lengths=None) -> None:
        if lengths is not None:
            raise NotImplementedError(_BAND_LENGTHS_ELSEWHERE)
        head = _BandHead(sieves)
        op, check = _feature_op(None, words, mode, semiring, weighting)
        super().__init__(op, check)
        self.head = head

    @property
    def sieves(self):
        return self.head.sieves

    def forward(self, X, lengths=None):
        return _apply_features(self.op, self.head, X, lengths, _BandFeatureFunction)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, {self.head.F} features per iterated sum"
