"""fruits_amd - the FRUITS iterated-sums hot path on AMD MI355X (gfx950).

Same public surface as the reference package for the path
``INC -> ISS (Reals, SimpleWords, optional Indices / L1 weighting) -> NPI / END``
(plus NEW, DIM, STD, NRM, MAV, LAG, FFN, RIN, JLD, the sieves MPI, XPI, LPI, MAX, MIN, CUR, AVG, STD, PPV,
CPV and the sieve wrappers INC / INT, the Arctic semiring and CosWISS): ``fruits_amd.ISS(...).fit_transform(X)`` and
``fruits_amd.Fruit.fit / transform``.  All arithmetic runs in hand-written HIP
kernels behind the C ABI of ``include/fruits_hip.h``; there is no CPU fallback.
``sieving.AVG`` and ``sieving.STD`` return CUR's numbers, as the reference's do
(fruits/sieving/segment.py:309, 352).
"""
from . import cache, callback, iss, preparation, seed, sieving
from .fruit import Fruit, FruitSlice
from .iss import semiring, words
from .iss.cos import CosWISS
from .iss.iss import ISS, ISSMode

__version__ = "0.1.0"


def __getattr__(name: str):
    # ``fruits_amd.nn`` (the differentiable ISS) imports torch and torch.nn: loaded on first use
    if name == "nn":
        import importlib
        return importlib.import_module(".nn", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def release_scratch() -> None:
    """Frees the device and page-locked scratch a device-side ``Fruit.fit`` keeps for the next
    one (fr_release_scratch); not in the reference."""
    from . import _native
    _native.release_scratch()
