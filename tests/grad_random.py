"""Random cases for the backward pass: word lists, shapes, modes, alphas and sieves drawn from a
seed, with inputs on which every sum is exact and real-valued ones (tests/test_grad_random_host.py,
tests/test_grad_random_gpu.py).  No GPU code, no torch.

Not a conftest: the modules that need it import it by name.

``case(seed)`` is ONE description for all five adjoints (``KINDS``): the same words and the same
shape, so a failure points at a kind or at the tables.  Everything is a pure function of the seed,
drawn from ``np.random.default_rng([2026, seed, ...])``.

What a case holds that the curated word sets of the other gradient tests do not: letters of up to
four occurrences of dimensions (exponents up to 4 and down to -4, mixed signs, three and four
dimensions in one letter), empty letters (``[2-2]``: the exponents cancel and the plan compiler
emits no factor), tries six deep, a "bush" (one prefix with 5 to 8 one-letter continuations), words
that occur two and three times (SINGLE: one node is several output rows), dimensions no word names.

Two departures from independent uniform draws, both so that the default seeds cover what
``test_grad_random_host.py`` counts:

* T is stratified - 23 consecutive seeds ``23 b ... 23 b + 22`` take the 23 lengths of ``T_POOL``
  in an order drawn for the block b - because 24 independent draws miss several of 23 values.
  (24 cases cannot hold each of 23 lengths twice: every length occurs once in any 23 consecutive
  seeds, twice in 46.)
* with probability 0.3 the letters draw from the dimensions 1 ... D-1 only, so that dimension D
  is one no word names.

No shape is avoided because the device refuses it: none was refused.
"""
import dataclasses
import functools

import numpy as np

import iss_grad_max_ref as gm
import iss_grad_ref as gr
from iss_grad_ref import orc

KINDS = ("reals", "arctic", "bayesian", "nontotal", "total")
# the edges of the lane (4 steps), wave (256) and chunk (1024) maps of csrc/kernels_grad.hip, whose
# suffix map is the forward one reversed
T_POOL = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1019, 1020, 1021, 1023, 1024, 1025, 1027,
          2047, 2048, 2049, 2051, 3073)
N_POOL = (1, 2, 3, 8, 9, 261)        # 261: more workgroups than one round; only with T <= 257
ALPHA_POOL = 12
CHUNK = 1024
DEFAULT_SEEDS = 24                   # FRUITS_TEST_RANDOM_CASES of tests/test_grad_random_gpu.py


@dataclasses.dataclass(frozen=True)
class Case:
    seed: int
    N: int
    D: int
    T: int
    mode: str                        # "SINGLE" | "EXTENDED"
    strings: tuple                   # the words
    alphas: tuple                    # per word a tuple of float32 values (as floats), one per letter
    tiny: bool = False

    def describe(self):
        """One line that reproduces the case."""
        which = "tiny_case" if self.tiny else "case"
        return (f"[grad_random.{which}({self.seed}): N={self.N} D={self.D} T={self.T} {self.mode} "
                f"words={list(self.strings)}]")

    def alpha_arrays(self):
        return [np.array(a, dtype=np.float32) for a in self.alphas]

    def zero_alphas(self):
        return [np.zeros(len(a), dtype=np.float32) for a in self.alphas]


# ------------------------------------------------------------------ words
def _letter(rng, dims):
    """A letter: 1 to 4 occurrences of dimensions, each negated with probability 0.2; with
    probability 0.05 a cancelling pair instead - an empty letter."""
    if rng.random() < 0.05:
        d = int(rng.integers(1, dims + 1))
        return f"[{d}-{d}]"
    el = ""
    for _ in range(int(rng.integers(1, 5))):
        d = int(rng.integers(1, dims + 1))
        el += f"-{d}" if rng.random() < 0.2 else str(d)
    return f"[{el}]"


def _words(rng, dims, most_words, most_letters, bush):
    words = ["".join(_letter(rng, dims) for _ in range(int(rng.integers(1, most_letters + 1))))
             for _ in range(int(rng.integers(1, most_words + 1)))]
    if rng.random() < 0.5:
        # one or two words again, once or twice: the same row up to three times
        for i in rng.choice(len(words), size=min(int(rng.integers(1, 3)), len(words)), replace=False):
            words += [words[int(i)]] * int(rng.integers(1, 3))
    if bush and rng.random() < 0.3:
        # one random prefix with 5 to 8 distinct one-letter continuations
        stem = words[int(rng.integers(0, len(words)))]
        letters = stem.split("]")[:-1]
        keep = int(rng.integers(0, min(len(letters), most_letters - 1) + 1))
        prefix = "".join(l + "]" for l in letters[:keep])
        tails = set()
        while len(tails) < int(rng.integers(5, 9)):
            tails.add(_letter(rng, dims))
        words += [prefix + t for t in sorted(tails)]
    return words


def _block_order(block):
    return np.random.default_rng([2026, 10 ** 6, block]).permutation(len(T_POOL))


def _make(seed, tiny):
    rng = np.random.default_rng([2026, seed, int(tiny)])
    if tiny:
        D = int(rng.integers(1, 4))
        T = int(rng.integers(1, 7))
        N = int(rng.integers(1, 3))
    else:
        D = int(rng.integers(1, 7))
        T = T_POOL[int(_block_order(seed // len(T_POOL))[seed % len(T_POOL)])]
        N = int(rng.choice(N_POOL, p=(0.13, 0.13, 0.2, 0.15, 0.15, 0.24)))
        if N == 261 and T > 257:
            N = int(rng.choice(N_POOL[:-1]))
    dims = D - 1 if D >= 2 and rng.random() < 0.3 else D
    words = _words(rng, dims, 4, 3, False) if tiny else _words(rng, dims, 12, 6, True)
    mode = "EXTENDED" if rng.random() < 0.6 else "SINGLE"
    # one alpha per letter and word from a pool of 12 float32 values in [0.25, 2] (a plan names at
    # most 63 distinct alphas, csrc/plan.cpp); tiny: 1 and 2, for exp tables of exact powers of two
    pool = (np.array([1.0, 2.0], dtype=np.float32) if tiny
            else rng.uniform(0.25, 2.0, ALPHA_POOL).astype(np.float32))
    alphas = tuple(tuple(float(a) for a in rng.choice(pool, len(orc.parse_word(s)))) for s in words)
    return Case(seed, N, D, T, mode, tuple(words), alphas, tiny)


@functools.lru_cache(maxsize=None)
def case(seed):
    """The case of a seed: immutable, shared by all kinds and tests."""
    return _make(int(seed), False)


@functools.lru_cache(maxsize=None)
def tiny_case(seed):
    """The same letters - exponents to +-4, empty letters - in 1 to 4 words of up to three letters
    on T <= 6: what the brute-force definitions take."""
    return _make(int(seed), True)


def keep(cache, key, value, most=6):
    """Stores ``value`` and drops the oldest entries beyond ``most``: the inputs of a case are
    shared by its tests, which run seed by seed, and a soak of 200 seeds must not hold them all."""
    cache[key] = value
    while len(cache) > most:
        cache.pop(next(iter(cache)))


def with_shape(c, N, T):
    return dataclasses.replace(c, N=N, T=T)


# ------------------------------------------------------------------ what a case holds
def rows_of(c):
    return gr.output_prefixes(list(c.strings), c.mode)


def nodes_of(c):
    return gm._nodes_of(rows_of(c))


def divided(c):
    """Dimensions (0-based) some word divides by."""
    return sorted({d for s in c.strings for row in orc.parse_word(s) for d, e in enumerate(row) if e < 0})


def heaviest(c):
    """W: the largest sum of |exponents| of an output row."""
    return max(sum(abs(e) for el in r for e in el) for r in rows_of(c))


def raw_letters(c):
    """Every letter as drawn, with its depth: (depth, [signed occurrences])."""
    out = []
    for s in c.strings:
        for depth, body in enumerate(s[1:-1].split("]["), 1):
            occ, sign = [], 1
            for ch in body:
                if ch == "-":
                    sign = -1
                else:
                    occ.append(sign * int(ch))
                    sign = 1
            out.append((depth, occ))
    return out


def coverage(c):
    """The properties test_grad_random_host.py counts over the default seeds, as a dict of bools."""
    rows = rows_of(c)
    nodes = nodes_of(c)
    kids = {v: sum(1 for w in nodes if len(w) == len(v) + 1 and w[:-1] == v) for v in nodes}
    emitted = {v: sum(1 for r in rows if r == v) for v in nodes}
    exps = [e for v in nodes for e in v[-1] if e != 0]
    letters = raw_letters(c)
    empty = [depth for depth, occ in letters if all(occ.count(d) == occ.count(-d) for d in occ)]
    deepest = max(len(v) for v in nodes)
    named = {d for v in nodes for d, e in enumerate(v[-1]) if e != 0}
    return {
        "an exponent >= 3": any(e >= 3 for e in exps),
        "an exponent <= -2": any(e <= -2 for e in exps),
        "a letter of mixed sign": any(min(v[-1], default=0) < 0 < max(v[-1], default=0) for v in nodes),
        "a letter over >= 3 dimensions": any(sum(1 for e in v[-1] if e) >= 3 for v in nodes),
        "an empty letter at depth 1": 1 in empty,
        "an empty letter at depth >= 2": any(d >= 2 for d in empty),
        "a trie of depth 5": deepest == 5,
        "a trie of depth 6": deepest == 6,
        "a node with >= 5 children": max(kids.values()) >= 5,
        "a node that is >= 3 output rows": max(emitted.values()) >= 3,
        "a SINGLE-mode inner node that is no row":
            c.mode == "SINGLE" and any(kids[v] and not emitted[v] for v in nodes),
        "an inner node that is a row": any(kids[v] and emitted[v] for v in nodes),
        "a dimension that no word names": len(named) < c.D,
    }


# ------------------------------------------------------------------ inputs on which every sum is exact
@dataclasses.dataclass(frozen=True)
class Exact:
    X: np.ndarray                    # (N, D, T), read-only
    G: np.ndarray                    # (N, K, T) integers from {-3 ... 3}, read-only
    alphas: list                     # zeros (the weighted kinds run at alpha = 0)
    N: int
    T: int                           # the case's, or smaller after a reduction
    q: int                           # every term is a multiple of 2^-q
    stage: int                       # 0: the full alphabet; 1, 2: narrowed
    reduced: bool                    # whether the alphabet was narrowed or T moved down
    proof: tuple                     # (largest gradient magnitude, largest forward magnitude)

    def case(self, c):
        """The case at the shape these inputs have."""
        return with_shape(c, self.N, self.T)


GROUP = {"reals": "reals", "nontotal": "reals", "total": "reals", "arctic": "arctic", "bayesian": "bayesian"}
_EXACT = {}


def _exact_draw(c, group, stage):
    """(X, G) of the case's full shape for an alphabet stage; a shorter T takes their first steps."""
    rng = np.random.default_rng([2026, c.seed, int(c.tiny), 2 + stage, KINDS.index(group)])
    N, D, T = c.N, c.D, c.T
    G = rng.integers(-3, 4, size=(N, len(rows_of(c)), T)).astype(np.float64)
    if group == "bayesian":
        # powers of two from [1/4, 2]; narrowed: from [1/2, 2]; at last: ones
        lo = (-2, -1, 0)[stage]
        hi = (2, 2, 1)[stage]
        return 2.0 ** rng.integers(lo, hi, size=(N, D, T)).astype(np.float64), G
    if group == "arctic":
        # integers; series 1, 4, ... on a rising staircase t // 5, series 2, 5, ... on a falling one
        X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
        X[1::3] += np.arange(T) // 5
        X[2::3] -= np.arange(T) // 5
        return X, G
    if stage == 0:
        X = rng.integers(-2, 3, size=(N, D, T)).astype(np.float64)
        for d in divided(c):
            X[:, d] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=(N, T))
    else:
        X = rng.integers(-1, 2, size=(N, D, T)).astype(np.float64)
        for d in divided(c):
            X[:, d] = rng.choice([-1.0, 1.0], size=(N, T))
    return X, G


def magnitudes(c, group, X, G):
    """(largest gradient magnitude, largest forward magnitude), from the references alone."""
    strings = list(c.strings)
    if group == "bayesian":
        back = gm.iss_grad_max(X, G, strings, c.mode, "Bayesian", magnitude=True)
        fwd = orc.iss_transform(X, strings, c.mode, semiring="Bayesian")
    else:
        back = gr.iss_grad(X, G, strings, c.mode, magnitude=True)
        fwd = orc.iss_transform(np.abs(X), strings, c.mode)
    return float(np.max(back, initial=0.0)), float(np.max(fwd, initial=0.0))


def exact_inputs(c, kind):
    """Integer-valued (dyadic) X and G of the case for which every partial sum on either side is
    exact, with the proof of that, taken from the references alone.

    Reals, and the weighted kinds at alpha = 0: X from {-2 ... 2}, from {+-0.5, +-1, +-2} in the
    dimensions some word divides by, G from {-3 ... 3}.  A term is a product of G and of powers
    x^e, so a multiple of 2^-q with q = W + 1 (W: the heaviest row's sum of |exponents|; + 1: the
    derivative of x^e, e < 0, has |e| + 1 factors 1/x).  Sums of multiples of 2^-q are exact in
    any order while they stay below 2^53 2^-q, and every partial sum of signed terms is bounded
    by the sum of their magnitudes: admitted when

        iss_grad(..., magnitude=True).max() * 2^q <= 2^53     and
        orc.iss_transform(|X|).max() * 2^q <= 2^53            (the forward sums)

    Bayesian: powers of two from [1/4, 2], two bits per elementary letter: q = 2 (W + 1), the
    same two conditions on iss_grad_max(magnitude=True) and on the forward rows.  Arctic: small
    integers (staircases as in tests/test_grad_max_gpu.py), whose sums are exact - admitted as
    drawn.

    A case that is not admitted is reduced, deterministically: first the alphabet is narrowed - to
    {-1, 0, 1}, {+-1} in divided dimensions (q stays W + 1); Bayesian to [1/2, 2], one bit per
    elementary letter, q = W + 1 - then T moves down ``T_POOL`` to the largest length that is
    admitted (the inputs are the first T steps of the same draw, so the magnitudes fall with T).
    Bayesian has a last resort, all ones (q = 0), for rows so heavy that 2^q alone exceeds 2^53.
    Every seed ends in an admitted case; a RuntimeError if not - never a skip."""
    group = GROUP[kind]
    key = (c, group)
    if key not in _EXACT:
        keep(_EXACT, key, _admit(c, group))
    return _EXACT[key]


def _admit(c, group):
    W = heaviest(c)
    stages = {"reals": (0, 1), "arctic": (0,), "bayesian": (0, 1, 2)}[group]
    lengths = [c.T] if c.tiny else [t for t in T_POOL if t <= c.T][::-1]
    for stage in stages:
        q = {"reals": W + 1, "arctic": 0, "bayesian": (2 * (W + 1), W + 1, 0)[stage]}[group]
        Xf, Gf = _exact_draw(c, group, stage)

        def attempt(T):
            X, G = np.ascontiguousarray(Xf[:, :, :T]), np.ascontiguousarray(Gf[:, :, :T])
            if group == "arctic":
                return X, G, (float(np.abs(X).max()), 0.0), True
            short = with_shape(c, c.N, T)
            proof = magnitudes(short, group, X, G)
            return X, G, proof, max(proof) * 2.0 ** q <= 2.0 ** 53

        # the full length; failing that, on the narrowed alphabet (Bayesian: on all ones too) the
        # largest admitted length below it - by bisection: the magnitudes fall with T
        found = None
        res = attempt(lengths[0])
        if res[3]:
            found = (lengths[0], res)
        elif stage > 0 and len(lengths) > 1:
            lo, hi = 0, len(lengths) - 1          # (lengths falls) lo: not admitted; hi: to be seen
            res = attempt(lengths[hi])
            if res[3]:
                found = (lengths[hi], res)
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    res = attempt(lengths[mid])
                    if res[3]:
                        hi, found = mid, (lengths[mid], res)
                    else:
                        lo = mid
        if found is not None:
            T, (X, G, proof, _) = found
            for a in (X, G):
                a.setflags(write=False)
            return Exact(X, G, c.zero_alphas(), c.N, T, q, stage, stage > 0 or T != c.T, proof)
    raise RuntimeError(f"no admitted exact inputs for {group} {c.describe()}")


# ------------------------------------------------------------------ real-valued inputs
_REAL = {}


def real_inputs(c, kind):
    """(X, G, alphas), read-only.  Reals and weighted: standard normal X, pushed to |x| >= 0.5 in
    the dimensions some word divides by, five exact zeros per other dimension; G standard normal;
    the alphas are the case's own.  Arctic: standard normal plus a trend 0.02 t.  Bayesian:
    uniform in [0.25, 1]."""
    group = GROUP[kind]
    key = (c, group)
    if key not in _REAL:
        rng = np.random.default_rng([2026, c.seed, int(c.tiny), 7, KINDS.index(group)])
        N, D, T = c.N, c.D, c.T
        if group == "arctic":
            X = rng.standard_normal((N, D, T)) + 0.02 * np.arange(T)
        elif group == "bayesian":
            X = 0.25 + 0.75 * rng.random((N, D, T))
        else:
            X = rng.standard_normal((N, D, T))
            div = divided(c)
            for d in div:
                small = np.abs(X[:, d]) < 0.5
                X[:, d] = np.where(small, np.copysign(np.abs(X[:, d]) + 0.5, X[:, d]), X[:, d])
            for d in sorted(set(range(D)) - set(div)):
                X[rng.integers(0, N, 5), d, rng.integers(0, T, 5)] = 0.0
        G = rng.standard_normal((N, len(rows_of(c)), T))
        for a in (X, G):
            a.setflags(write=False)
        keep(_REAL, key, (X, G))
    X, G = _REAL[key]
    return X, G, c.alpha_arrays()


# ------------------------------------------------------------------ sieves
def sieves_of(c):
    """1 to 5 sieve specs ``(name, cuts, q)`` (q None: the default band) of END, MAX and MIN for
    series of c.T steps: integer cuts, -1 among them, a sieve with a segment that starts past 0
    where T >= 2, a cut at each side of a chunk edge where the series has one; MAX and MIN take
    q = (-1, 0, 1) with probability 0.3.  At most 5 * 8 * 2 features: far below 256."""
    rng = np.random.default_rng([2026, c.seed, int(c.tiny), 3])
    T = c.T
    out = []
    for _ in range(int(rng.integers(1, 6))):
        name = str(rng.choice(["END", "MAX", "MIN"]))
        inner = sorted({int(v) for v in rng.integers(1, T + 1, size=int(rng.integers(0, 4)))} - {T})
        cuts = inner + ([-1] if rng.random() < 0.7 or not inner else [])
        q = (-1, 0, 1) if name != "END" and rng.random() < 0.3 else None
        out.append([name, cuts, q])
    if not any(-1 in s[1] for s in out):
        out[0][1].append(-1)
    if T >= 2 and not any(len(s[1]) >= 2 for s in out):
        out[-1][1] = sorted({max(T // 2, 1)} | (set(out[-1][1]) - {-1, T})) + [-1]
    edge = [v for v in (CHUNK, CHUNK + 1) if v < T]
    if edge:
        keep = set(out[0][1]) - {-1}
        out[0][1] = sorted(keep | set(edge)) + ([-1] if -1 in out[0][1] else [])
    return tuple((name, tuple(cuts), q) for name, cuts, q in out)


def full_sieves(T):
    """Exactly 256 features on series of T >= 128 steps: 128 ENDs, and a MAX of 64 segments in two
    bands."""
    assert T >= 128
    ends = tuple(int(v) for v in np.linspace(1, T - 1, 127).astype(int)) + (-1,)
    assert len(set(ends)) == 128
    return (("END", ends, None), ("MAX", ends[1::2], (-1, 0, 1)))


def nfeatures(specs):
    return sum(len(cuts) * (1 if name == "END" else (len(q) - 1 if q else 1)) for name, cuts, q in specs)


def reference_specs(specs):
    """The specs as tests/features_grad_ref.py takes them: thresholds in place of q."""
    out = []
    for name, cuts, q in specs:
        if name == "END":
            out.append((name, cuts))
        else:
            qs = (-1, 1) if q is None else q
            out.append((name, cuts, tuple(np.inf if v == 1 else (-np.inf if v == -1 else 0.0) for v in qs)))
    return out
