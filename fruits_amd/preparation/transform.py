"""Preparateurs on the MI355X path (mirrors fruits/preparation/transform.py: INC, STD, NRM, MAV,
LAG, FFN, RIN, RDW, JLD, SPE, RPE, CTS, QTC and FUN).  Each runs as a HIP kernel on device
tensors - FUN alone calls the user's function on the host; the numpy-facing ``transform``
uploads, runs and downloads.

The fitted preparateurs (MAV, FFN, RIN, JLD) draw their state in ``_fit`` from numpy's GLOBAL
generator with the reference's calls in the reference's order, so ``np.random.seed(s)`` followed
by ``fit`` gives the reference's state bit for bit.  Their fits look at ``X.shape`` only
(``_fit_needs_shape``): a fruit hands them a zero-copy stand-in of the prepared shape instead of
downloading the prepared fit sample."""
from __future__ import annotations

from typing import Any, Callable, Optional, Union

import numpy as np

from .. import _native as nat
from ..cache import CacheType, SharedSeedCache
from .abstract import Preparateur

__all__ = ["INC", "STD", "NRM", "MAV", "LAG", "FFN", "RIN", "RDW", "JLD", "SPE", "RPE", "CTS",
           "QTC", "FUN"]


class INC(Preparateur):
    """Increments: ``[x_1, ..., x_n] -> [0, x_2 - x_1, ..., x_n - x_{n-1}]``
    (fruits/preparation/transform.py:15-89; kernel: fruits/cache.py:8-13).

    Args:
        shift: lag of the difference; a float is a fraction of the series
            length (rounded up), a callable maps the length to the lag.
        depth: how many times the transform is applied.
        zero_padding: if False the first ``shift`` values are restored from
            the input instead of being zero.
    """

    def __init__(self, shift: Union[int, float, Callable[[int], int]] = 1,
                 depth: int = 1, zero_padding: bool = True) -> None:
        self._shift = shift
        if depth < 1:
            raise ValueError("depth has to be a positive integer > 0")
        self._depth = depth
        self._zero_padding = zero_padding

    @property
    def requires_fitting(self) -> bool:
        return False

    def _lag(self, T: int) -> int:
        if isinstance(self._shift, int):
            return self._shift
        if isinstance(self._shift, float):
            return int(np.ceil(self._shift * T))
        if callable(self._shift):
            return int(self._shift(T))
        raise TypeError(f"Type {type(self._shift)} not supported for argument shift")

    def _supports_lengths(self) -> bool:
        # (an integer lag: a float or a callable is a function of the padded length)
        return isinstance(self._shift, (int, np.integer)) and not isinstance(self._shift, bool)

    def _transform_device(self, Xd, lengths_d=None):
        # (increments are causal: the valid part of a series does not see its tail)
        lag = self._lag(int(Xd.shape[2]))
        out = Xd
        for _ in range(self._depth):
            if self._zero_padding:
                out = nat.increments(out, lag)
            else:
                # the reference restores X[:, :, :shift] after every pass
                # (transform.py:73-74); it needs an integer shift there too
                out = nat.increments(out, lag, head_src=Xd, head=int(self._shift))
        return out

    def _copy(self) -> "INC":
        return INC(self._shift, self._depth, self._zero_padding)

    def __eq__(self, other: Any) -> bool:
        return (isinstance(other, INC) and self._shift == other._shift
                and self._depth == other._depth
                and self._zero_padding == other._zero_padding)

    def __str__(self) -> str:
        return f"INC({self._shift}, {self._depth}, {self._zero_padding})"


class STD(Preparateur):
    """Standardisation ``(x - mean) / (std + eps)`` per series and dimension
    (fruits/preparation/transform.py:92-158).  ``separately=False`` uses one
    mean / std of the whole fit sample."""

    def __init__(self, separately: bool = True, var: bool = True,
                 std_eps: float = 1e-5) -> None:
        self._separately = separately
        self._div_std = var
        self._mean = None
        self._std = None
        self._eps = std_eps

    def _fit_needs_data(self) -> bool:
        return not self._separately

    def _fit(self, X: np.ndarray) -> None:
        if not self._separately:
            self._mean = np.mean(X)
            self._std = np.std(X) if self._div_std else 1

    def _supports_lengths(self) -> bool:
        # (separately=False: one mean / deviation of the whole fit sample, tails included)
        return bool(self._separately)

    def _transform_device(self, Xd, lengths_d=None):
        if self._separately:
            return nat.standardize(Xd, self._div_std, float(self._eps), lengths_d=lengths_d)
        if self._mean is None or self._std is None:
            raise RuntimeError("Missing call of self.fit()")
        return (Xd - float(self._mean)) / (float(self._std) + float(self._eps))

    def _copy(self) -> "STD":
        return STD(self._separately, self._div_std)

    def __eq__(self, other: Any) -> bool:
        return (isinstance(other, STD) and self._separately == other._separately
                and self._div_std == other._div_std)

    def __str__(self) -> str:
        return f"STD({self._separately}, {self._div_std})"


class _DeviceTables:
    """Mixin: the device copies of a preparateur's host tables, kept in ``_programs`` (dropped
    when pickled, like a plan)."""

    def _fresh_transients(self) -> None:
        self._programs = {}

    @staticmethod
    def _upload(host, ints: int) -> tuple:
        kinds = [np.float64] * (len(host) - ints) + [np.int32] * ints
        return tuple(nat.to_device(np.ascontiguousarray(a, dtype=k), dtype=k)
                     for a, k in zip(host, kinds))

    def _device_tables(self, Xd, *host, ints: int = 0):
        """Device copies of the fitted host arrays ``host`` (float64; the last ``ints`` of them
        int32), uploaded once per device for as long as the preparateur holds these very arrays
        (state assigned after a fit is seen)."""
        progs = self.__dict__.setdefault("_programs", {})
        key = str(Xd.device)
        held = progs.get(key)
        if held is None or len(held[0]) != len(host) or any(a is not b for a, b in zip(held[0], host)):
            held = progs[key] = (host, self._upload(host, ints))
        return held[1]

    def _derived_tables(self, Xd, key, build, ints: int = 0):
        """Device copies of the tables ``build()`` returns (a tuple of host arrays; float64, the
        last ``ints`` of them int32): tables that follow from settings or fitted state which
        ``key`` names completely.  Built and uploaded once per device for as long as ``key``
        stays what it was; no host copy is kept."""
        progs = self.__dict__.setdefault("_programs", {})
        slot = ("derived", str(Xd.device))
        held = progs.get(slot)
        if held is None or held[0] != key:
            held = progs[slot] = (key, self._upload(build(), ints))
        return held[1]


class _ShapeFitted(_DeviceTables, Preparateur):
    """A preparateur whose ``fit`` reads ``X.shape`` alone and whose fitted tables live on the
    device once per fit."""

    def _fit_needs_data(self) -> bool:
        return False

    def _fit_needs_shape(self) -> bool:
        return True

    def fit(self, X: np.ndarray) -> None:
        super().fit(X)
        self._programs = {}


class NRM(Preparateur):
    """Normalisation ``(x - min) / (max - min)`` per series and dimension, or with
    ``scale_dim=True`` per series over all its dimensions; constant rows become 0
    (fruits/preparation/transform.py:161-209)."""

    def __init__(self, scale_dim: bool = False) -> None:
        self._scale_dim = scale_dim

    @property
    def requires_fitting(self) -> bool:
        return False

    def _transform_device(self, Xd):
        return nat.prep_normalize(Xd, bool(self._scale_dim))

    def _copy(self) -> "NRM":
        return NRM(scale_dim=self._scale_dim)

    def __eq__(self, other: Any) -> bool:
        return isinstance(other, NRM) and self._scale_dim == other._scale_dim

    def __str__(self) -> str:
        return f"NRM({self._scale_dim})"


class MAV(_ShapeFitted):
    """Moving average over ``width`` time steps, a float being a fraction of the series
    length (fruits/preparation/transform.py:212-274)."""

    def __init__(self, width: Union[int, float] = 5) -> None:
        if isinstance(width, float) and not 0.0 < width < 1.0:
            raise ValueError("If width is a float, it has to be in (0,1)")
        self._w_given = width

    def _fit(self, X: np.ndarray) -> None:
        given = self._w_given
        if isinstance(given, float):       # a fraction of the series length, at least one step
            self._w = max(int(given * X.shape[2]), 1)
        elif given > 0:
            self._w = given
        # width -1 never gets a width here (transform.py:250-256): transform then raises

    def _check_fitted(self) -> None:
        if not hasattr(self, "_w"):
            raise RuntimeError("Missing call of self.fit()")

    def _transform_device(self, Xd):
        self._check_fitted()
        if int(self._w) > int(Xd.shape[2]):      # no window fits the series: all zeros (:237)
            return nat.torch().zeros_like(Xd)
        return nat.prep_moving_average(Xd, int(self._w))

    def _copy(self) -> "MAV":
        return MAV(self._w_given)

    def __eq__(self, other: Any) -> bool:
        return isinstance(other, MAV) and self._w_given == other._w_given

    def __str__(self) -> str:
        return f"MAV({self._w_given})"


class LAG(Preparateur):
    """Lead-lag transform: every dimension ``[x_1, ..., x_n]`` becomes the two dimensions
    ``[x_1, x_2, x_2, ..., x_n]`` and ``[x_1, x_1, x_2, ..., x_n]`` of length ``2n - 1``
    (fruits/preparation/transform.py:277-309)."""

    @property
    def requires_fitting(self) -> bool:
        return False

    def _transform_device(self, Xd):
        return nat.prep_leadlag(Xd)

    def _copy(self) -> "LAG":
        return LAG()

    def __eq__(self, other: Any) -> bool:
        return isinstance(other, LAG)

    def __str__(self) -> str:
        return "LAG()"


class FFN(_ShapeFitted):
    """Two-layer feed-forward network with gaussian weights applied to every time step:
    ``W2 relu(W1 (x - mean) + b)`` (fruits/preparation/transform.py:312-388).

    Args:
        d_out: number of output dimensions.
        d_hidden: nodes of the hidden layer, ``2 * input dimensions`` if None.
        center: subtract every dimension's mean over time first.
        relu_out: a ReLU on the output too.
    """

    def __init__(self, d_out: int = 1, d_hidden: Optional[int] = None, center: bool = True,
                 relu_out: bool = False) -> None:
        self._d_hidden = d_hidden
        self._d_out = d_out
        self._center = center
        self._relu_out = relu_out

    def _fit(self, X: np.ndarray) -> None:
        n_in = X.shape[1]
        hidden = 2 * n_in if self._d_hidden is None else self._d_hidden
        # three gaussian draws in the reference's order: first layer, its biases, second layer
        # (transform.py:346-360)
        shapes = ((hidden, n_in), (hidden, ), (self._d_out, hidden))
        self._weights1, self._biases, self._weights2 = (
            np.random.normal(loc=0, scale=1.0, size=shape) for shape in shapes)

    def _check_fitted(self) -> None:
        if not hasattr(self, "_weights1"):
            raise RuntimeError("FFN was not fitted")

    def _transform_device(self, Xd):
        self._check_fitted()
        W1, b, W2 = self._device_tables(Xd, self._weights1, self._biases, self._weights2)
        return nat.prep_ffn(Xd, W1, b, W2, bool(self._center), bool(self._relu_out))

    def _copy(self) -> "FFN":
        return FFN(d_out=self._d_out, d_hidden=self._d_hidden, center=self._center,
                   relu_out=self._relu_out)

    def __str__(self) -> str:
        return f"FFN({self._d_out}, {self._d_hidden}, {self._center}, {self._relu_out})"


def _spread(n_in: int, n_out: int) -> np.ndarray:
    """Sizes of ``n_out`` groups that share ``n_in`` slots as evenly as possible, the larger
    groups first (transform.py:495-504, 694-703); more groups than slots is an error."""
    if n_out > n_in:
        raise ValueError(f"Output dimensions ({n_out}) should be <= input dimensions ({n_in})")
    small, larger = divmod(n_in, n_out)
    sizes = np.full(n_out, small, dtype=np.int32)
    sizes[:larger] += 1
    return sizes


def _shuffled_dims(n_in: int) -> np.ndarray:
    """A random order of the input dimensions: one ``np.random.choice`` without replacement,
    the reference's call (transform.py:505-507, 704-706)."""
    return np.random.choice(n_in, size=n_in, replace=False).astype(np.int32)


def _draw_centred(rows: int, width: int) -> np.ndarray:
    """Standard-normal weights, every row shifted to mean zero."""
    weights = np.random.normal(size=(rows, width))
    return weights - weights.mean(axis=1, keepdims=True)


def _draw_sum_one(rows: int, width: int) -> np.ndarray:
    """Uniform weights on [-1, 1] pushed so that every row sums to one without leaving the
    interval: what a row lacks is handed out in proportion to each weight's distance from the
    border, so weights near zero move most.  A draw with a row that has (almost) no room left is
    thrown away and drawn again."""
    while True:
        weights = np.random.uniform(-1., 1., size=(rows, width))
        room = 1.0 - np.abs(weights)
        row_room = np.sum(room, axis=1)
        if not np.any(row_room < 1e-5):
            lacking = 1.0 - np.sum(weights, axis=1)
            return weights + room * (lacking / row_room)[:, np.newaxis]


class RIN(_ShapeFitted):
    """Random increments ``y_i = x_i - (k_w x_{i-1} + ... + k_1 x_{i-w})`` with a kernel drawn
    in ``fit`` (fruits/preparation/transform.py:391-568).

    Args:
        width: kernel length (shortened to ``T - 1``), or a callable of the series length.
        adaptive_width: the input counts as padded with ``width`` zeros, so the first outputs
            use a truncated kernel instead of being zero.
        out_dim: number of output dimensions (<= input dimensions), each convolving a nearly
            equal share of randomly chosen input dimensions; -1: as many as the input has.
        force_sum_one: uniform weights on [-1, 1] forced to sum to one instead of centred
            gaussian weights.
        kernel: a fixed ``(D, w)`` kernel; everything but ``adaptive_width`` is then ignored.
    """

    def __init__(self, width: Union[int, Callable[[int], int]] = 1, adaptive_width: bool = False,
                 out_dim: int = -1, force_sum_one: bool = False,
                 kernel: Optional[np.ndarray] = None) -> None:
        self._width = width
        self._adaptive_width = adaptive_width
        self._out_dim = out_dim
        self._force_sum_one = force_sum_one
        self._const_kernel = kernel

    def _fit(self, X: np.ndarray) -> None:
        n_in, length = int(X.shape[1]), int(X.shape[2])
        if self._const_kernel is not None:
            # a given kernel: one slot per dimension, in order; everything but adaptive_width
            # is ignored and nothing is drawn (transform.py:485-489)
            self._kernel = self._const_kernel.copy()
            self._ndim_per_kernel = np.ones(n_in, dtype=np.int32)
            self._dims_per_kernel = np.arange(n_in, dtype=np.int32)
            return
        if callable(self._width):
            width = self._width(length)
        else:
            width = min(self._width, length - 1)      # (shortened to T - 1)
        self._ndim_per_kernel = _spread(n_in, self._out_dim if self._out_dim > 0 else n_in)
        # the reference's draws in its order: the dimension order, then the weights
        # (transform.py:505-523)
        self._dims_per_kernel = _shuffled_dims(n_in)
        draw = _draw_sum_one if self._force_sum_one else _draw_centred
        self._kernel = draw(n_in, width)

    def _check_fitted(self) -> None:
        if not hasattr(self, "_kernel"):
            raise RuntimeError("RIN preparateur misses a .fit() call")

    def _transform_device(self, Xd):
        self._check_fitted()
        t = nat.torch()
        N, D, T = (int(v) for v in Xd.shape)
        kernel = np.ascontiguousarray(self._kernel, dtype=np.float64)
        ndim = np.ascontiguousarray(self._ndim_per_kernel, dtype=np.int32)
        dims = np.ascontiguousarray(self._dims_per_kernel, dtype=np.int32)
        if kernel.ndim != 2 or kernel.shape[0] < dims.size:
            raise ValueError("RIN kernel has to be a (dimensions, width) array")
        w = int(kernel.shape[1])
        if not self._adaptive_width and w >= T:
            # no output index reaches the kernel's width (transform.py:460): all zeros
            return t.zeros((N, ndim.size, T), dtype=Xd.dtype, device=Xd.device)
        kd, nd, dd = self._device_tables(Xd, self._kernel, self._ndim_per_kernel,
                                         self._dims_per_kernel, ints=2)
        return nat.prep_fir(Xd, kd, w, nd, dd, ndim, dims, bool(self._adaptive_width))

    def _copy(self) -> "RIN":
        return RIN(width=self._width, adaptive_width=self._adaptive_width, out_dim=self._out_dim,
                   force_sum_one=self._force_sum_one, kernel=self._const_kernel)

    def _settings(self) -> tuple:
        return (self._width, self._adaptive_width, self._out_dim, self._force_sum_one)

    def __eq__(self, other: Any) -> bool:
        if not isinstance(other, RIN) or self._settings() != other._settings():
            return False
        # (two given kernel arrays of several weights: the truth value of their ``==`` raises
        # ValueError, as in the reference - transform.py:560)
        return bool(self._const_kernel == other._const_kernel)

    def __str__(self) -> str:
        return (f"RIN({self._width}, {self._adaptive_width}, "
                f"{self._out_dim}, {self._force_sum_one}, {self._const_kernel})")


class RDW(_ShapeFitted):
    """Random dimension weights: every dimension is raised to a random exponent, the same for
    all time steps; the exponents sum to one (fruits/preparation/transform.py:571-613).

    Args:
        dist: ``"dirichlet"`` draws the exponents from a Dirichlet distribution whose parameters
            are proportional to the largest mean absolute value of each dimension in the fit
            sample - that fit reads the data; anything else draws them uniformly.
    """

    def __init__(self, dist: str = "dirichlet") -> None:
        self._dist = dist

    def _fit_needs_data(self) -> bool:
        return self._dist == "dirichlet"

    def _fit_needs_shape(self) -> bool:
        return self._dist != "dirichlet"

    def _fit(self, X: np.ndarray) -> None:
        if self._dist == "dirichlet":
            alphas = np.abs(X).mean(axis=0).max(axis=1)
            used = alphas != 0
            alphas[used] = alphas[used] / np.max(alphas[used])
            if not used.all():       # (a dimension that is zero everywhere: transform.py:594-595)
                alphas += 1e-5
            self._weights = np.random.dirichlet(alphas)
        else:
            drawn = np.random.random(X.shape[1])
            self._weights = drawn / np.sum(drawn)

    def _check_fitted(self) -> None:
        self._weights      # (AttributeError without a fit, as in the reference: transform.py:602)

    def _transform_device(self, Xd):
        self._check_fitted()
        if np.size(self._weights) != int(Xd.shape[1]):
            raise ValueError(f"RDW was fitted on {np.size(self._weights)} dimensions, "
                             f"got {int(Xd.shape[1])}")
        wd, = self._device_tables(Xd, self._weights)
        return nat.prep_pointwise(nat.FR_PW_POW, Xd, wd)

    def _copy(self) -> "RDW":
        return RDW(self._dist)

    def __eq__(self, other: Any) -> bool:
        return isinstance(other, RDW) and other._dist == self._dist

    def __str__(self) -> str:
        return f"RDW({self._dist!r})"


class JLD(_ShapeFitted):
    """Johnson-Lindenstrauss dimensionality reduction: every time step is multiplied with
    random gaussian vectors (fruits/preparation/transform.py:616-746).

    Args:
        dim: number of output dimensions; a float ``f`` in (0, 1) stands for the smallest
            integer ``>= 24 log(d) / (3 f^2 - 2 f^3)``.
        distribute: every output dimension combines only its own nearly equal share of the
            input dimensions (needs ``input_dim >= output_dim``).
        bias: add a gaussian bias to every projected dimension.
    """

    def __init__(self, dim: Union[int, float] = 0.99, distribute: bool = False,
                 bias: bool = False) -> None:
        if isinstance(dim, float) and not (0 < dim < 1):
            raise ValueError("'dim' has to be an integer or a float in (0, 1)")
        self._d = dim
        self._distribute = distribute
        self._bias = bias

    def _output_dims(self, n_in: int) -> int:
        if not isinstance(self._d, float):
            return self._d
        f = self._d       # smallest integer >= 24 log(d) / (3 f^2 - 2 f^3)  (transform.py:688-690)
        return int(24 * np.log(n_in) / (3 * f**2 - 2 * f**3)) + 1

    def _fit(self, X: np.ndarray) -> None:
        n_in = int(X.shape[1])
        n_out = self._output_dims(n_in)
        # draws in the reference's order: the dimension order when distributing, the weights,
        # then the bias (transform.py:693-722)
        if self._distribute:
            self._ndim_per_kernel = _spread(n_in, n_out)
            self._dims_per_kernel = _shuffled_dims(n_in)
            n_weights = n_in
        else:       # every output dimension reads every input dimension
            self._ndim_per_kernel = np.full(n_out, n_in, dtype=np.int32)
            self._dims_per_kernel = np.tile(np.arange(n_in, dtype=np.int32), n_out)
            n_weights = n_in * n_out
        self._kernel = np.random.standard_normal(n_weights)
        self._bias_weights = (np.random.standard_normal(n_out) if self._bias
                              else np.zeros(n_out, dtype=np.float64))

    def _check_fitted(self) -> None:
        self._kernel      # (the reference has no check of its own: AttributeError, transform.py:725-727)

    def _transform_device(self, Xd):
        self._check_fitted()
        ndim = np.ascontiguousarray(self._ndim_per_kernel, dtype=np.int32)
        dims = np.ascontiguousarray(self._dims_per_kernel, dtype=np.int32)
        kd, bd, nd, dd = self._device_tables(Xd, self._kernel, self._bias_weights,
                                             self._ndim_per_kernel, self._dims_per_kernel,
                                             ints=2)
        return nat.prep_project(Xd, kd, bd, nd, dd, ndim, dims)

    def _copy(self) -> "JLD":
        return JLD(dim=self._d, distribute=self._distribute, bias=self._bias)

    def __eq__(self, other: Any) -> bool:
        return (isinstance(other, JLD) and self._d == other._d
                and self._distribute == other._distribute and self._bias == other._bias)

    def __str__(self) -> str:
        return f"JLD({self._d}, {self._distribute}, {self._bias})"


class _TimeMasked(_DeviceTables):
    """Mixin of the preparateurs that keep or zero whole time steps of every series alike
    (DIL, DOT, PDD, CTS(pseudo_shift=True)): ``_time_mask(T)`` says which steps stay, the device
    gets it as ``ceil(T / 32)`` 32-bit words, bit ``t % 32`` of word ``t // 32``.
    ``_mask_state()`` names everything besides ``T`` that the mask follows from (hashable): the
    words are built and uploaded again only when it changes."""

    def _time_mask(self, T: int) -> np.ndarray:
        raise NotImplementedError

    def _mask_state(self) -> tuple:
        raise NotImplementedError

    def _mask_words(self, T: int) -> np.ndarray:
        keep = np.zeros(-(-T // 32) * 32, dtype=bool)
        keep[:T] = self._time_mask(T)
        return np.packbits(keep, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)

    def _masked_device(self, Xd):
        T = int(Xd.shape[2])
        md, = self._derived_tables(Xd, (T, self._mask_state()), lambda: (self._mask_words(T), ),
                                   ints=1)
        return nat.prep_mask(Xd, md)


def _seed_cache(prep, Xd) -> SharedSeedCache:
    """The cache ``prep`` is attached to.  Wrapped in DIM / NEW it has none: the reference's
    wrappers call the wrapped preparateur's public ``transform`` (wrapper.py:41, 88), which makes
    a temporary cache of the batch it is handed - so does this."""
    cache = getattr(prep, "_cache", None)
    if cache is None:
        cache = SharedSeedCache()
        cache.adopt_device_input(Xd)
    return cache


def _phase_scale(length, freq: float) -> float:
    """``T ** f`` of ``sin(t / T ** f)`` for an integer length ``T``."""
    return float(length) ** freq


class SPE(_DeviceTables, Preparateur):
    """Sinusoidal positional embedding ``y_t = x_t * sin(t / T**f)``, ``t = 0, ..., T - 1``, or
    with ``operation="additive"`` the sum instead (fruits/preparation/transform.py:749-835).

    Args:
        freq: the exponent ``f``, usually between 0 and 1.
        operation: ``"multiplicative"`` or ``"additive"``.
        function: applied to the scaled time steps in place of the sine (called on the host).
        step_transform: ``"L1"`` or ``"L2"``: the cumulative path length of the cache's input
            takes the place of ``t`` - every series then has its own wave, and ``T`` is the
            series' total path length.  The sines are taken on the device.
        max_length: a fixed ``T``.
    """

    def __init__(self, freq: float, operation: str = "multiplicative",
                 function: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                 step_transform: Optional[str] = None, max_length: Optional[int] = None) -> None:
        self._freq = freq
        self._operation = operation
        self._function = function
        self._step_transform = step_transform
        self._max_length = max_length

    def _mode(self) -> int:
        try:
            return {"multiplicative": nat.FR_PW_MUL, "additive": nat.FR_PW_ADD}[self._operation]
        except (KeyError, TypeError):
            raise ValueError(f"Unknown operation given: {self._operation}") from None

    def _transform_device(self, Xd):
        N, T = int(Xd.shape[0]), int(Xd.shape[2])
        if self._step_transform is None:
            length = T if self._max_length is None else self._max_length
            scale = _phase_scale(length, self._freq)
            if self._function is not None:       # (called on every transform, as in the reference)
                wave = np.ascontiguousarray(self._function(np.arange(T) / scale), dtype=np.float64)
                return nat.prep_pointwise(self._mode(), Xd, nat.to_device(wave.reshape(1, T)))
            wd, = self._derived_tables(Xd, (T, length, self._freq),
                                       lambda: (np.sin(np.arange(T) / scale).reshape(1, T), ))
            return nat.prep_pointwise(self._mode(), Xd, wd)
        path = _seed_cache(self, Xd).get_device(CacheType.ISS, self._step_transform)
        rows = int(path.shape[0])
        if int(path.shape[1]) != T or not (rows == N or rows == 1 or N == 1):
            raise ValueError(f"operands could not be broadcast together: a batch of shape "
                             f"{tuple(Xd.shape)} and path lengths of shape {tuple(path.shape)}")
        if self._max_length is None:
            phase = path / path[:, -1:] ** self._freq
        else:
            phase = path / _phase_scale(self._max_length, self._freq)
        if self._function is None:
            return nat.prep_pointwise(self._mode(), Xd, phase.contiguous(), flags=nat.FR_PW_FLAG_SIN)
        # a user's function of the phase: to the host, through the callable and back
        wave = np.ascontiguousarray(self._function(nat.to_host(phase)), dtype=np.float64)
        return nat.prep_pointwise(self._mode(), Xd, nat.to_device(wave.reshape(rows, T)))

    def _copy(self) -> "SPE":
        return SPE(freq=self._freq, operation=self._operation, function=self._function,
                   step_transform=self._step_transform, max_length=self._max_length)

    def _settings(self) -> tuple:
        return (self._freq, self._operation, self._function, self._step_transform, self._max_length)

    def __eq__(self, other: Any) -> bool:
        return isinstance(other, SPE) and self._settings() == other._settings()

    def __str__(self) -> str:
        return (f"SPE({self._freq}, {self._operation}, {self._function}, "
                f"{self._step_transform}, {self._max_length})")


class RPE(_DeviceTables, Preparateur):
    """Rotational positional embedding: the two dimensions of every time step ``t`` are rotated
    by the angle ``t / T**f`` (fruits/preparation/transform.py:838-907).

    Args:
        freq: the exponent ``f``, usually between 0 and 1.
        max_length: a fixed ``T`` in place of the series length.
    """

    def __init__(self, freq: float, max_length: Optional[int] = None) -> None:
        self._freq = freq
        self._max_length = max_length

    def _angles(self, T: int) -> np.ndarray:
        length = T if self._max_length is None else self._max_length
        return np.arange(T) / _phase_scale(length, self._freq)

    def _transform_device(self, Xd):
        if int(Xd.shape[1]) != 2:
            raise ValueError(f"RPE input has to have 2 dimensions, got {int(Xd.shape[1])}")
        T = int(Xd.shape[2])
        cd, sd = self._derived_tables(Xd, (T, self._max_length, self._freq),
                                      lambda: (np.cos(self._angles(T)), np.sin(self._angles(T))))
        return nat.prep_pointwise(nat.FR_PW_ROTATE, Xd, cd, sd)

    def _copy(self) -> "RPE":
        return RPE(freq=self._freq, max_length=self._max_length)

    def __eq__(self, other: Any) -> bool:
        return (isinstance(other, RPE) and self._freq == other._freq
                and self._max_length == other._max_length)

    def __str__(self) -> str:
        return f"RPE({self._freq}, {self._max_length})"


class CTS(_TimeMasked, Preparateur):
    """Constant time shift: the series moves ``s`` steps to the left and its last value fills
    the end, ``y[:-s] = x[s:]``, ``y[-s:] = x[-1]`` (fruits/preparation/transform.py:910-958).

    Args:
        s: the number of steps, at least 1; a float in (0, 1) is a fraction of the length.
        pseudo_shift: zero the first ``s`` values instead of shifting.
    """

    def __init__(self, s: Union[float, int], pseudo_shift: bool = False) -> None:
        self._s = s
        self._pseudo_shift = pseudo_shift

    def _steps(self, T: int) -> int:
        if 0 < self._s < 1:
            return max(1, int(self._s * T))
        return int(self._s)

    def _time_mask(self, T: int) -> np.ndarray:
        keep = np.ones(T, dtype=bool)
        keep[:self._steps(T)] = False
        return keep

    def _mask_state(self) -> tuple:
        return (self._s, )

    def _transform_device(self, Xd):
        if self._pseudo_shift:
            return self._masked_device(Xd)
        steps = self._steps(int(Xd.shape[2]))
        if steps < 1:     # (the reference's slices then differ in length: transform.py:943)
            raise ValueError(f"CTS needs a shift of at least one time step, got {steps}")
        return nat.prep_pointwise(nat.FR_PW_SHIFT, Xd, shift=steps)

    def _copy(self) -> "CTS":
        return CTS(s=self._s, pseudo_shift=self._pseudo_shift)

    def __eq__(self, other: Any) -> bool:
        return (isinstance(other, CTS) and self._s == other._s
                and self._pseudo_shift == other._pseudo_shift)

    def __str__(self) -> str:
        return f"CTS({self._s}, {self._pseudo_shift})"


class QTC(Preparateur):
    """Quantile cut: ``min(q, x_t)`` with ``q`` a quantile of the fit sample
    (fruits/preparation/transform.py:961-1015).

    Args:
        q: which quantile, in (0, 1).
        lower: ``max(q, x_t)`` instead.
        bound: the value the cut parts are set to, ``x[x > q] = bound``; the quantile if None.
    """

    def __init__(self, q: float, lower: bool = False, bound: Optional[float] = None) -> None:
        self._q = q
        self._lower = lower
        self._bound = bound

    def _fit(self, X: np.ndarray) -> None:
        self._quantile = np.quantile(X, self._q)

    def _check_fitted(self) -> None:
        self._quantile      # (AttributeError without a fit, as in the reference: transform.py:993)

    def _transform_device(self, Xd):
        self._check_fitted()
        q = float(self._quantile)
        return nat.prep_pointwise(nat.FR_PW_CLIP, Xd, q=q,
                                  v=q if self._bound is None else float(self._bound),
                                  flags=nat.FR_PW_FLAG_LOWER if self._lower else 0)

    def _copy(self) -> "QTC":
        return QTC(q=self._q, lower=self._lower, bound=self._bound)

    def __eq__(self, other: Any) -> bool:
        return (isinstance(other, QTC) and self._q == other._q and self._lower == other._lower
                and self._bound == other._bound)

    def __str__(self) -> str:
        return f"QTC({self._q}, {self._lower}, {self._bound})"


class FUN(Preparateur):
    """Applies a function to the ``(N, D, T)`` dataset
    (fruits/preparation/transform.py:1018-1048).  The function works on numpy arrays: inside a
    fruit the batch is downloaded, handed to ``f`` and the result uploaded - a host round trip
    per call.

    Args:
        f: maps a float64 array of shape ``(N, D, T)`` to one of shape ``(N, D', T')``.
    """

    def __init__(self, f: Callable[[np.ndarray], np.ndarray]) -> None:
        self._function = f

    @property
    def requires_fitting(self) -> bool:
        return False

    def _transform_device(self, Xd):
        result = self._function(nat.to_host(Xd))
        if not isinstance(result, np.ndarray) or result.dtype != np.float64 or result.ndim != 3:
            raise TypeError("the function of FUN has to return a float64 array of shape (N, D, T)")
        return nat.to_device(result)

    def _copy(self) -> "FUN":
        return FUN(self._function)

    def __eq__(self, other: Any) -> bool:
        return False

    def __str__(self) -> str:
        return f"FUN({self._function})"
