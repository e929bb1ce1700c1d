"""`python tools/grad_golden.py [directory]` from the root of the tree: records the gradients the
backward pass computes on real-valued inputs, for the tests that hold its bits still
(`test_max_backward_keeps_its_bits` of tests/test_grad_max_gpu.py, `test_weighted_backward_keeps_its_bits`
of tests/test_grad_weighted_gpu.py).  One `grad_<adjoint>_before_shared_frame.npz` per adjoint -
arctic, bayesian, weighted_nontotal, weighted_total - with the array `dX`, into `directory`
(default tests/golden).

The files under tests/golden were written ONCE, on an MI355X, by a checkout of the commit BEFORE
the adjoints' kernels were folded into one frame: they are what that commit
computed, and the tests compare them bit for bit.  Running this on a later commit records that
commit, which proves nothing about it - do so only to pin a deliberate change of the arithmetic.

The inputs are those of the tests, built the same way: N = 3, D = 3, T = kGradChunk + 6, the four
words of the bound tests, EXTENDED (10 rows); X is drawn first, then G, from one generator."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, D, T, K = 3, 3, 1024 + 6, 10
WORDS = ["[1][2][3]", "[11][2]", "[1][-2]", "[12][2][3][1]"]
NAME = "grad_{}_before_shared_frame.npz"


def max_inputs(semiring):
    """(X, G) of the Arctic or the Bayesian golden: a trend keeps the running maxima rising all
    along the series, so that more than a thousand entries of the gradient are heads."""
    rng = np.random.default_rng([12, semiring == "Arctic"])
    if semiring == "Arctic":
        X = rng.standard_normal((N, D, T)) + 0.02 * np.arange(T)
    else:
        X = 1 + 0.25 * rng.random((N, D, T)) + 0.001 * np.arange(T)
    return X, rng.standard_normal((N, K, T))


def weighted_inputs():
    """(X, G) of both weighted goldens."""
    rng = np.random.default_rng(12)
    X = rng.standard_normal((N, D, T))
    return X, rng.standard_normal((N, K, T))


def main(directory):
    import torch
    import fruits_amd as fr
    from fruits_amd import _native as nat
    from fruits_amd import nn
    from fruits_amd.iss.weighting import Indices
    from test_grad_weighted_gpu import drawn_alphas

    nat.require_device()
    os.makedirs(directory, exist_ok=True)

    def record(name, X, G, forward, floor):
        Xd = torch.from_numpy(X).cuda().requires_grad_(True)
        Y = forward(Xd)
        assert tuple(Y.shape) == (N, K, T), Y.shape
        Y.backward(torch.from_numpy(G).cuda())
        dX = Xd.grad.cpu().numpy()
        assert np.isfinite(dX).all() and (dX != 0).sum() > floor, (name, int((dX != 0).sum()))
        np.savez_compressed(os.path.join(directory, NAME.format(name)), dX=dX)
        print(f"{name}: {int((dX != 0).sum())} non-zero of {dX.size}, largest {np.abs(dX).max():.6g}")

    words = [fr.words.SimpleWord(s) for s in WORDS]
    for semiring in ("Arctic", "Bayesian"):
        sr = fr.semiring.Arctic() if semiring == "Arctic" else fr.semiring.Bayesian()
        X, G = max_inputs(semiring)
        record(semiring.lower(), X, G,
               lambda Xd: nn.max_iss(Xd, words, fr.ISSMode.EXTENDED, semiring=sr), 1000)
    weighted = [fr.words.SimpleWord(s) for s in WORDS]
    for w, a in zip(weighted, drawn_alphas(WORDS, seed=12)):
        w.alpha = a
    X, G = weighted_inputs()
    for total in (False, True):
        op = fr.ISS(weighted, mode=fr.ISSMode.EXTENDED, weighting=Indices(total=total))
        record("weighted_total" if total else "weighted_nontotal", X, G,
               lambda Xd: nn.weighted_iss(Xd, op), 9000)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
