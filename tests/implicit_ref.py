"""numpy restatement of PPV / CPV (fruits/sieving/implicit.py:114-129, 169-190) on (N, T) rows
and given thresholds: what the device tests compare against.  test_implicit.py holds it to the
reference's recorded outputs (tests/golden/golden_implicit.*), exactly."""
import numpy as np


def indicator(X, q, segments, j):
    """The indicator of feature ``j``: closed below, the thresholds in the order given."""
    if segments:
        return np.logical_and(q[j] <= X, X < q[j + 1])
    return X >= q[j]


def nfeatures(q, segments):
    return len(q) - 1 if segments else len(q)


def ppv(X, q, segments=False):
    out = np.zeros((X.shape[0], nfeatures(q, segments)))
    with np.errstate(invalid="ignore"):
        for j in range(out.shape[1]):
            out[:, j] = np.sum(indicator(X, q, segments, j), axis=1)
            out[:, j] /= X.shape[1]
    return out


def cpv(X, q, segments=False):
    out = np.zeros((X.shape[0], nfeatures(q, segments)))
    n = X.shape[1] + X.shape[1] % 2
    with np.errstate(invalid="ignore"):
        for j in range(out.shape[1]):
            ind = indicator(X, q, segments, j)
            # rising edges at t >= 1: the first difference is zero-padded (fruits/cache.py:8-13)
            rise = ind[:, 1:] & ~ind[:, :-1]
            out[:, j] = 2 * np.sum(rise, axis=-1) / n
    return out


def transform(kind, X, q, segments=False):
    return (ppv if kind == "PPV" else cpv)(X, np.asarray(q, dtype=np.float64), segments)


def exposure(A, q, segments=False, rel=1e-10):
    """(N, F) numbers of elements of every row of ``A`` within ``rel * max|row|`` of a finite
    threshold of feature j - the rule of SieveOracle.exposure (oracle/ref_numpy.py) for the
    closed-below tests: a re-associated scan may put such an element on the other side, so a
    PPV count may differ by that many and CPV's edge count too (flipping one indicator moves
    the number of rising edges by at most one).  Element 0 is computed without an addition on
    every path: left out."""
    q = np.asarray(q, dtype=np.float64)
    tol = rel * np.abs(A).max(axis=1, keepdims=True)
    out = np.zeros((A.shape[0], nfeatures(q, segments)), dtype=np.int64)
    for j in range(out.shape[1]):
        near = np.zeros(A.shape, dtype=bool)
        for thr in ((q[j], q[j + 1]) if segments else (q[j],)):
            if np.isfinite(thr):
                near |= np.abs(A - thr) <= tol
        near[:, 0] = False
        out[:, j] = near.sum(axis=1)
    return out


def edge_rows(T, rng):
    """(rows, T) small integers in [-2, 2] with the rows that matter for a closed-below test and
    for CPV's edges: random ones, all-in and all-out rows, rows that start inside a component,
    alternating rows, and one with NaN, +inf and -inf."""
    rows = [rng.integers(-2, 3, T).astype(np.float64) for _ in range(3)]
    rows.append(np.full(T, 2.0))                       # above every threshold
    rows.append(np.full(T, -2.0))                      # below
    rows.append(np.where(np.arange(T) % 2 == 0, 1.0, -1.0))   # starts inside, alternates
    rows.append(np.where(np.arange(T) % 2 == 0, -1.0, 1.0))
    rows.append(np.where(np.arange(T) < (T + 1) // 2, 0.0, -1.0))   # one component from t = 0
    special = rng.integers(-2, 3, T).astype(np.float64)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 0.0, np.inf)):
        if T > 1:
            special[(1 + 3 * i) % T] = v
    rows.append(special)
    return np.stack(rows)
