"""Numpy restatement of the iterated sums of GENERIC words - words of named letter functions,
fruits/iss/words/letters.py - as the reference's slow path computes them
(fruits/iss/semiring.py:54-75).  Test infrastructure: written from the recursion itself, held to
the reference's recorded outputs (tests/golden/golden_words.npz) by tests/test_words_host.py.

The recursion, for one series Z (D, T) and a word of extended letters e_0 .. e_{L-1}:

    tmp = one                                  (1 for Reals and Bayesian, 0 for Arctic)
    for k, e_k:  C = one (x) l_1(Z) (x) l_2(Z) ...        the letters of e_k, left to right
                 k > 0: tmp = (0, tmp[0], ..., tmp[T-2])  one step to the right
                 tmp[k:] = acc(tmp[k:] (x) C[k:])         cumsum, or a running maximum
                 the row of prefix k + 1 is tmp

so the sum is over strictly increasing positions and the first k positions of the row of prefix
k + 1 stay exactly 0.0 - for Reals and Bayesian.  Arctic overrides the slow path
(fruits/iss/semiring.py:428-446) with one that neither shifts nor restricts to [k:]:

    for k, e_k:  tmp = running maximum of (tmp + C)

i.e. positions i1 <= i2 <= ..., like its fast kernel.  No weighting enters in any of them.

A word is written as a string, ``"[ABS(1)DIM(2)][ReLU(1)]"``; ``[]`` is an extended letter
without letters.  ``LETTERS`` maps a name to ``f(X, i) -> (T,)``.
"""
import numpy as np

LETTERS = {
    "DIM": lambda X, i: X[i, :],
    "ABS": lambda X, i: np.abs(X[i, :]),
    "ReLU": lambda X, i: X[i, :] * (X[i, :] > 0),
    "SQ": lambda X, i: X[i, :] * X[i, :],
}

ONE = {"Reals": 1.0, "Arctic": 0.0, "Bayesian": 1.0}


def register(package) -> None:
    """Registers the custom letters above with ``package.words`` - once per process, a second
    registration of a name raises."""
    have = package.words.letters.get_available()
    for name, fn in LETTERS.items():
        if name not in have:
            package.words.letter(name=name)(fn)


def is_generic(word: str) -> bool:
    return "[]" in word or any(c.isalpha() for c in word)


def parse(word: str):
    """``"[ABS(1)DIM(2)][]"`` -> [[("ABS", 0), ("DIM", 1)], []]"""
    out = []
    for body in word.split("]")[:-1]:
        letters = []
        for piece in body[1:].split(")")[:-1]:
            name, dim = piece.split("(")
            letters.append((name, int(dim) - 1))
        out.append(letters)
    return out


def prefixes(Z: np.ndarray, word: str, semiring: str = "Reals") -> np.ndarray:
    """(L, T): the rows of all prefixes of ``word`` on one series Z (D, T)."""
    T = Z.shape[1]
    els = parse(word)
    times = semiring != "Arctic"
    tmp = np.full(T, ONE[semiring])
    rows = np.zeros((len(els), T))
    for k, el in enumerate(els):
        C = np.full(T, ONE[semiring])
        for name, dim in el:
            v = np.asarray(LETTERS[name](Z, dim), dtype=np.float64)
            C = C * v if times else C + v
        if semiring == "Arctic":
            tmp = np.maximum.accumulate(tmp + C)
            rows[k] = tmp
            continue
        if k > 0:
            tmp = np.concatenate([[0.0], tmp[:-1]])
        if k < T:
            head = tmp[k:] * C[k:] if times else tmp[k:] + C[k:]
            tmp[k:] = np.cumsum(head) if semiring == "Reals" else np.maximum.accumulate(head)
        rows[k] = tmp
    return rows


def cache_plan(strings):
    """fruits/iss/cache.py:21-43 on the words' strings: rows every word emits in EXTENDED mode."""
    plan = []
    for i, s in enumerate(strings):
        letters = s.split("[")[1:]
        depth, first, prefix = len(letters), 0, ""
        for el in letters:
            prefix += "[" + el
            hit = next((k for k in range(first, i) if strings[k].startswith(prefix)), None)
            if hit is None:
                break
            first = hit
            depth -= 1
        plan.append(depth)
    return plan


def iss_transform(X: np.ndarray, words, mode: str = "SINGLE", semiring: str = "Reals") -> np.ndarray:
    """(K, N, T) rows of a list of generic words, in the reference's order
    (fruits/iss/iss.py:21-67)."""
    depths = cache_plan(words) if mode == "EXTENDED" else [1] * len(words)
    N, _, T = X.shape
    out = np.zeros((sum(depths), N, T))
    k0 = 0
    for w, d in zip(words, depths):
        for n in range(N):
            out[k0:k0 + d, n] = prefixes(X[n], w, semiring)[len(parse(w)) - d:]
        k0 += d
    return out


def head_lengths(words, mode: str = "SINGLE", semiring: str = "Reals"):
    """Per emitted row the number of leading positions that are exactly 0.0: p - 1 for the
    prefix of length p (none for Arctic, which does not shift)."""
    depths = cache_plan(words) if mode == "EXTENDED" else [1] * len(words)
    out = []
    for w, d in zip(words, depths):
        L = len(parse(w))
        out += [0 if semiring == "Arctic" else p - 1 for p in range(L - d + 1, L + 1)]
    return out
