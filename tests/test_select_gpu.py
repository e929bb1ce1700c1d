"""The rank selection of Fruit.fit (fr_select_ranks, csrc/kernels_select.hip) pass by pass.

The reference throughout is ``np.sort(orc.pre_transform(A[r], inc).ravel())[k]`` and the comparison
is ``assert_array_equal``: the kernels form the same differences in the same order, so there is no
tolerance anywhere (inputs are finite; the sign of a zero is not compared).  Every case asserts in
numpy the precondition that makes it reach the path it is about - the split of the time axis, an
over-full bucket of several values, an untracked successor - so that a later change of data or
constants cannot quietly turn it into a test of the usual path."""
import os

import numpy as np
import pytest

from oracle import ref_numpy as orc

pytestmark = pytest.mark.gpu

# The library exposes none of these; they mirror csrc/kernels.h ...
SMALL_CAP = 4096      # kSelSmallCap: candidates of one 24-bit bucket that a workgroup settles
TRACK_JOBS = 2        # kSelTrackJobs: successors per group and order that the gather pass tracks
GROUP_MAX = 8         # kSelGroupMax: jobs of one group
MAX_INC = 8           # kMaxInc
# ... and select_ranks_mi in csrc/kernels_select.hip (the launch's blocks per group)
BLOCK_ELEMS = 256 * 16
BLOCKS_PER_GROUP = 512
BLOCKS_IN_ALL = 4096  # kSelBlocks
BUCKET_SHIFT = 40     # kSelSmallShift: a bucket is the leading 64 - 40 bits of an order key


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


def order_keys(v):
    """csrc/walk_types.h: order_key."""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where((b >> np.uint64(63)) != 0, ~b, b | (np.uint64(1) << np.uint64(63)))


def buckets(v):
    return order_keys(v) >> np.uint64(BUCKET_SHIFT)


def device_groups(jobs):
    """The device jobs of a call and their groups, as fr_select_ranks_begin lays them out: sorted by
    (row, order, rank); a duplicate shares its predecessor's job, a rank one above its predecessor's
    rides on it as its successor; up to GROUP_MAX jobs of one row form a group.  A list of groups,
    each a list of [row, inc, rank, wants_successor]."""
    groups, prev, prev_via = [], None, False
    for cur in sorted(tuple(j) for j in jobs):
        if prev is not None and prev[:2] == cur[:2]:
            if prev[2] == cur[2]:
                continue
            if not prev_via and prev[2] + 1 == cur[2]:
                groups[-1][-1][3] = True
                prev, prev_via = cur, True
                continue
        if groups and groups[-1][0][0] == cur[0] and len(groups[-1]) < GROUP_MAX:
            groups[-1].append([cur[0], cur[1], cur[2], False])
        else:
            groups.append([[cur[0], cur[1], cur[2], False]])
        prev, prev_via = cur, False
    return groups


def untracked_successors(groups):
    """Jobs whose successor the gather pass does not track: beyond the first TRACK_JOBS of their
    group and order."""
    n = 0
    for g in groups:
        pos, last = 0, None
        for _, inc, _, succ in g:
            pos = pos + 1 if inc == last else 0
            last = inc
            n += bool(succ and pos >= TRACK_JOBS)
    return n


def grid_of(N, T, n_groups):
    """Blocks per group of the data passes (select_ranks_mi)."""
    bpj = min(-(-N * T // BLOCK_ELEMS), BLOCKS_PER_GROUP)
    if bpj * n_groups > BLOCKS_IN_ALL:
        bpj = -(-BLOCKS_IN_ALL // n_groups)
    return max(bpj, 1)


def ranks_of(n):
    return sorted({max(k, 0) for k in (0, n - 1, n - 2, n // 2 - 1, n // 2, 3 * n // 4)})


class Block:
    """A (rows, N, T) block on the device and the sorted differenced rows it is checked against
    (each sorted once)."""

    def __init__(self, A):
        from fruits_amd import _native as nat
        assert np.isfinite(A).all()
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.Ad = nat.to_device(self.A)
        self._sorted = {}

    def sorted(self, row, inc):
        if (row, inc) not in self._sorted:
            self._sorted[(row, inc)] = np.sort(orc.pre_transform(self.A[row], inc).ravel())
        return self._sorted[(row, inc)]

    def check(self, jobs, note=""):
        """Selects `jobs` ((row, inc, rank) triples, in this order) and compares with the sort."""
        from fruits_amd import _native as nat
        rows, incs, ranks = (list(x) for x in zip(*jobs))
        want = np.array([self.sorted(r, i)[k] for r, i, k in jobs])
        got = nat.select_ranks(self.Ad, rows, incs, ranks)
        wrong = [f"row {r} inc {i} rank {k}: got {g!r}, sorted {w!r}"
                 for (r, i, k), g, w in zip(jobs, got, want) if not g == w]
        np.testing.assert_array_equal(
            got, want, err_msg=f"{note} block {self.A.shape}: {len(wrong)} of {len(jobs)} wrong: "
                               + "; ".join(wrong[:12]))
        return got


# ------------------------------------------------------------------ 1. the time axis is split
SPLIT_SHAPES = [(2, 4097), (2, 5000), (3, 6000), (3, 9000), (4, 4097), (1, 9000), (20, 5000), (5, 40000)]


def drifting_walk(rng, R, N, T):
    """A random walk that drifts upwards plus an offset per series: the top ranks lie in the last
    time part of the last series, the lowest in the first part of the first, and the increments
    are independent draws - whatever part of whatever series a pass leaves out, some rank moves."""
    steps = rng.standard_normal((R, N, T)) + 0.25
    return steps.cumsum(axis=2) + (0.25 * T + 8.0 * np.sqrt(T)) * np.arange(N)[None, :, None]


@pytest.mark.parametrize("N,T", SPLIT_SHAPES, ids=lambda v: str(v))
def test_time_split(fr, N, T):
    """Fewer series than blocks per group: every block takes a time part of one series
    (csrc/select_partition.h).  Orders 0 and 1 alone (their own kernel instances), 0 / 1 / 2
    together and 8 alone; the ranks at the top equal the sort only if every part of every series
    was counted."""
    blk = Block(drifting_walk(np.random.default_rng(N * 100003 + T), 1, N, T))
    for incs in ((0,), (1,), (0, 1, 2), (8,)):
        jobs = [(0, inc, k) for inc in incs for k in ranks_of(N * T)]
        grid = grid_of(N, T, len(device_groups(jobs)))
        assert N < grid, (N, T, grid)          # the precondition of the split
        blk.check(jobs, f"time split, grid {grid}, orders {incs}:")


@pytest.mark.parametrize("groups_per_row", [1, 21])
def test_time_split_many_groups(fr, groups_per_row):
    """(3, 9000) on 40 row blocks.  One group per row block: 40 groups of 7 blocks each (7 x 40 is
    far from the cap of BLOCKS_IN_ALL).  21 groups per row block (56 ranks per order, 168 jobs per
    row block): 840 groups, and the cap lowers the 7 blocks per group to 5 - still more than the 3
    series, and no multiple of them."""
    N, T, R = 3, 9000, 40
    n = N * T
    blk = Block(drifting_walk(np.random.default_rng(40), R, N, T))
    if groups_per_row == 1:
        jobs = [(r, r % 3, k) for r in range(R) for k in ranks_of(n)]
    else:
        spread = [int(k) for k in np.linspace(0, n - 1, 56)]
        jobs = [(r, inc, k) for r in range(R) for inc in (0, 1, 2) for k in spread]
    n_groups = len(device_groups(jobs))
    grid, uncapped = grid_of(N, T, n_groups), grid_of(N, T, 1)
    assert n_groups == R * groups_per_row and N < grid
    if groups_per_row == 1:
        assert grid == uncapped == 7
    else:
        assert uncapped * n_groups > BLOCKS_IN_ALL and grid == 5 and grid % N != 0
    blk.check(jobs, f"time split, {n_groups} groups, grid {grid}:")
    fr.release_scratch()     # (6720 candidate lists)


# ------------------------------------------------------------------ 2. differencing orders 3 .. 8
HIGH_SHAPES = [(1, 2), (3, 5), (7, 129), (17, 1024), (3, 1500)]
INC_SETS = [(3,), (4,), (5,), (6,), (7,), (8,), (0, 3, 8), (1, 2, 5), tuple(range(MAX_INC + 1))]
HIGH_CASES = [(N, T, kind) for N, T in HIGH_SHAPES for kind in ("normal", "walk")] + \
             [(N, T, "ramps") for N, T in HIGH_SHAPES if T >= 129]


def integer_ramps(rng, N, T):
    """Integer-valued, piecewise linear with a kink at 2 % of the elements: the differences of
    order >= 2 vanish exactly away from the kinks - the ties sit at level k, not at level 0."""
    kink = np.where(rng.random((N, T)) < 0.02, rng.integers(-3, 4, size=(N, T)), 0)
    slope = kink.cumsum(axis=1) + rng.integers(1, 4, size=(N, 1))
    return (slope.cumsum(axis=1) + rng.integers(-5, 6, size=(N, 1))).astype(np.float64)


@pytest.mark.parametrize("N,T,kind", HIGH_CASES, ids=lambda v: str(v))
def test_high_orders(fr, N, T, kind):
    """Orders 3 .. 8 (the kMaxInc kernel instances: nine difference levels per element in every
    pass), each alone and mixed with lower ones; series no longer than the order included."""
    rng = np.random.default_rng(N * 7919 + T + len(kind))
    if kind == "ramps":
        A = integer_ramps(rng, N, T)[None]
        n = N * T
        for inc in range(3, MAX_INC + 1):      # the precondition: ties at level inc ...
            assert np.count_nonzero(orc.pre_transform(A[0], inc) == 0.0) > n // 2, inc
        assert np.unique(A[0], return_counts=True)[1].max() < n // 10      # ... and not at level 0
    else:
        A = rng.standard_normal((1, N, T))
        if kind == "walk":
            A = A.cumsum(axis=2)
    blk = Block(A)
    for incs in INC_SETS:
        assert max(incs) > 2                   # beyond the instances for orders 0, 1, 2
        jobs = [(0, inc, k) for inc in incs for k in ranks_of(N * T)]
        if len(incs) > GROUP_MAX:
            assert len(device_groups(jobs)) > 1     # several groups on one row block
        blk.check(jobs, f"{kind}, orders {incs}:")


# ------------------------------------------------------------------ 3. all eight digits
def planted_bucket(rng, inc, sign, distinct, pop):
    """A block whose order-`inc` values hold `pop` elements in the bucket of sign * 1.0, of `distinct`
    values sign * (1 + j 2^-45), j = 0 .. distinct - 1: they share the leading 24 bits of their keys
    and differ in the last two digits (negative keys are complemented).  Two elements each in the
    buckets next to it on either side; nothing else in it.
    inc = 0: the data itself, (8, 1024).  inc = 1: (128, 64), a cumulative sum of such values and of
    eighths - every partial sum is a multiple of 2^-45 below 256, so it is exact and the first
    differences are the values again."""
    N, T = ((8, 1024), (128, 64))[inc]
    V = (rng.standard_normal((N, T)) * 3.0) if inc == 0 else rng.integers(-24, 25, size=(N, T)) / 8.0
    target = buckets(np.array([sign * 1.0]))[0]
    V[buckets(V) == target] = sign * 2.5
    # (d1[0] is the zero padding)
    free = np.arange(N * T) if inc == 0 else np.flatnonzero(np.arange(N * T) % T != 0)
    where = rng.permutation(free)[:pop + 4]
    js = np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=pop - distinct)])
    flat = V.reshape(-1)
    flat[where[:pop]] = sign * (1.0 + js * 2.0 ** -45)
    flat[where[pop:pop + 2]] = sign * (1.0 + 2.0 ** -12)     # the bucket next to it, away from zero
    flat[where[pop + 2:]] = sign * (1.0 - 2.0 ** -13)        # ... and towards zero (another exponent)
    A = V if inc == 0 else V.cumsum(axis=1)
    P = orc.pre_transform(A, inc)
    if inc == 1:
        np.testing.assert_array_equal(P[:, 1:], V[:, 1:])     # the construction worked
    return A[None], P.ravel(), target


EIGHT_DIGIT_CASES = [(distinct, 6000) for distinct in (1, 2, 3, 200)] + [(3, SMALL_CAP), (3, SMALL_CAP + 1)]


@pytest.mark.parametrize("inc", [0, 1])
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["positive", "negative"])
@pytest.mark.parametrize("distinct,pop", EIGHT_DIGIT_CASES, ids=lambda v: str(v))
def test_all_eight_digits(fr, distinct, pop, sign, inc):
    """One 24-bit bucket holds more candidates than a workgroup settles, of several values: the
    gather pass cannot resolve the jobs and the five low-digit histogram passes decide them
    (select_hist_kernel<MI, 0>); their successors come from the last digit's histogram, or from the
    successor pass.  Exactly SMALL_CAP candidates are still settled in the workgroup, one more is
    not.  One value alone (`distinct` 1) is resolved by the gather pass for two jobs of a group;
    the third goes through the digits."""
    rng = np.random.default_rng(distinct * 131 + pop + 7 * inc + (sign < 0))
    A, P, target = planted_bucket(rng, inc, sign, distinct, pop)
    blk = Block(A)
    S = blk.sorted(0, inc)
    inside = np.flatnonzero(buckets(S) == target)
    b0, b1 = int(inside[0]), int(inside[-1]) + 1
    # the preconditions: the bucket's population and its values
    assert b1 - b0 == pop == np.count_nonzero(buckets(P) == target)
    values, starts = np.unique(S[b0:b1], return_index=True)
    assert len(values) == distinct
    starts = [b0 + int(s) for s in starts] + [b1]
    pairs = [b0 - 1, b1 - 1]                   # into the bucket from below; its last element
    for i in sorted({0, 1, distinct // 2, distinct - 1} & set(range(distinct))):
        s, e = starts[i], starts[i + 1]
        if e - s >= 2:
            pairs.append(s + (e - s - 2) // 2)  # both inside one run of equal values
        if i + 1 < distinct:
            pairs.append(e - 1)                # the last copy of a value: the successor is the next value
    singles = [b0 + pop // 3, b0 + pop // 5, b0 + 1]
    jobs = [(0, inc, k + d) for k in sorted(set(pairs)) for d in (0, 1)] + [(0, inc, k) for k in singles]
    assert buckets(S[b1 - 1:b1 + 1]).tolist() != [target, target]       # the successor lies in another bucket
    groups = device_groups(jobs)
    in_bucket = max(sum(b0 <= k < b1 for _, _, k, _ in g) for g in groups)
    assert in_bucket >= 3                      # more than the two jobs GatherBig holds
    blk.check(jobs, f"bucket of {pop} candidates, {distinct} values, order {inc}:")


# ------------------------------------------------------------------ 4. successors
def successor_block(rng, inc):
    """Multiples of 2^-20 (a cumulative sum of them is exact): a background of 3 N(0, 1), 5000
    copies of 0.5, and 50 values in the bucket of 4.0.  inc = 0: (2, 4100); inc = 1: the
    cumulative sum over (130, 64)."""
    N, T = ((2, 4100), (130, 64))[inc]
    q = 2.0 ** -20
    V = np.round(rng.standard_normal((N, T)) * 3.0 / q) * q
    free = np.flatnonzero(np.arange(N * T) % T != 0) if inc else np.arange(N * T)
    where = rng.permutation(free)
    flat = V.reshape(-1)
    flat[where[:5000]] = 0.5
    flat[where[5000:5050]] = 4.0 + rng.integers(1, 1024, size=50) * q
    A = V if inc == 0 else V.cumsum(axis=1)
    if inc == 1:
        np.testing.assert_array_equal(orc.pre_transform(A, 1)[:, 1:], V[:, 1:])
    return A[None]


@pytest.mark.parametrize("inc", [0, 1])
def test_successors(fr, inc):
    """Neighbouring ranks (k, k + 1) ride on one job: the next order statistic comes from the
    gather pass for the first TRACK_JOBS pairs of a group and order, from select_succ_kernel for the
    others.  Pairs across the sign, across a power of two, from the largest element of a small
    bucket, from the last of more than SMALL_CAP copies of a value and inside such a run; then the
    same ranks as jobs of their own."""
    rng = np.random.default_rng(77 + inc)
    blk = Block(successor_block(rng, inc))
    S = blk.sorted(0, inc)
    bk = buckets(S)
    b4 = np.flatnonzero(bk == buckets(np.array([4.0]))[0])
    half = (int(np.searchsorted(S, 0.5, "left")), int(np.searchsorted(S, 0.5, "right")))
    ks = {
        "largest negative": int(np.count_nonzero(S < 0)) - 1,
        "last non-positive": int(np.count_nonzero(S <= 0)) - 1,     # (the largest negative, or a zero)
        "below 2": int(np.count_nonzero(S < 2.0)) - 1,
        "below -2": int(np.count_nonzero(S <= -2.0)) - 1,
        "largest of a small bucket": int(b4[-1]),
        "last copy": half[1] - 1,
        "inside the copies": half[0] + 100,
    }
    # the preconditions
    k = ks["largest negative"]
    assert S[k] < 0 <= S[k + 1]
    k = ks["last non-positive"]
    assert S[k] <= 0 < S[k + 1]
    k = ks["below 2"]
    assert S[k] < 2.0 <= S[k + 1] and np.frexp(S[k])[1] != np.frexp(S[k + 1])[1]
    k = ks["below -2"]
    assert S[k] <= -2.0 < S[k + 1] and np.frexp(S[k])[1] != np.frexp(S[k + 1])[1]
    assert 2 <= len(b4) <= SMALL_CAP
    assert half[1] - half[0] > SMALL_CAP and S[ks["inside the copies"] + 1] == 0.5
    for name, k in ks.items():
        if name != "inside the copies":
            assert bk[k] != bk[k + 1], name    # the successor lies in another bucket
    first = sorted(set(ks.values()))
    assert len(first) >= 6 > TRACK_JOBS
    assert all(b - a > 2 for a, b in zip(first, first[1:]))     # no pair rides on another
    pairs = [(0, inc, k + d) for k in first for d in (0, 1)]
    groups = device_groups(pairs)
    assert sum(len(g) for g in groups) == len(first) and untracked_successors(groups) >= 4
    got = blk.check(pairs, f"pairs, order {inc}:")
    # the same ranks apart: the k alone and the k + 1 alone, duplicated, in shuffled order
    for d in (0, 1):
        alone = [(0, inc, k + d) for k in first] * 2
        alone = [alone[i] for i in rng.permutation(len(alone))]
        assert not any(j[3] for g in device_groups(alone) for j in g)     # nobody rides
        again = blk.check(alone, f"ranks k + {d} alone, order {inc}:")
        for job, v in zip(alone, again):
            assert v == got[pairs.index(job)]


@pytest.mark.parametrize("N,T", [(1, 33), (3, 1500)], ids=lambda v: str(v))
def test_successors_in_a_partial_wave(fr, N, T):
    """Series whose length is no multiple of a wave: the tail of the time range runs with some
    lanes switched off, and select_succ_kernel must not reduce over them.  Eight pairs (k, k + 1)
    of one order on one row block whose successors lie in other buckets: six of them untracked,
    five of them further jobs of their level in the successor pass."""
    rng = np.random.default_rng(N + T)
    blk = Block(rng.standard_normal((1, N, T)) * 1e3)
    S = blk.sorted(0, 0)
    bk = buckets(S)
    n = N * T
    assert T % 64 != 0
    first = [int(k) for k in np.linspace(1, n - 3, 8)]
    assert all(b - a > 2 for a, b in zip(first, first[1:]))
    assert sum(bk[k] != bk[k + 1] for k in first[TRACK_JOBS:]) >= 3     # the successor pass has several jobs
    pairs = [(0, 0, k + d) for k in first for d in (0, 1)]
    groups = device_groups(pairs)
    assert len(groups) == 1 and untracked_successors(groups) == len(first) - TRACK_JOBS
    blk.check(pairs, "pairs in a partial wave:")


# ------------------------------------------------------------------ 5. whole series per block
@pytest.mark.parametrize("N,T", [(300, 2), (513, 8), (601, 33), (4097, 2)], ids=lambda v: str(v))
def test_whole_series_per_block(fr, N, T):
    """At least as many series as blocks: block b takes the series b, b + grid, ... - on shapes where
    the series are no multiple of the grid."""
    blk = Block(drifting_walk(np.random.default_rng(N + T), 1, N, T))
    for incs in ((0,), (2,)):
        jobs = [(0, inc, k) for inc in incs for k in ranks_of(N * T)]
        grid = grid_of(N, T, len(device_groups(jobs)))
        assert N >= grid
        if N * T > BLOCK_ELEMS:
            assert grid > 1 and N % grid != 0
        blk.check(jobs, f"grid {grid}, orders {incs}:")


# ------------------------------------------------------------------ random cases
def alternating(rng, N, T):
    """0, v, 0, v', ...: with v = 1 + j 2^-45 the differences of order k >= 1 are about +-2^(k-1),
    half of the elements each, with distinct low bits - two over-full buckets of many values at
    every order (and the one of 1.0 at order 0)."""
    return (np.arange(T) % 2) * (1.0 + rng.integers(0, 200, size=(N, T)) * 2.0 ** -45)


@pytest.mark.parametrize("seed", range(int(os.environ.get("FRUITS_TEST_RANDOM_CASES", "12"))))
def test_select_ranks_random_orders(fr, seed):
    """fr_select_ranks on random row blocks against a sort, like test_select_ranks_random, over what
    that one leaves out: orders up to 8, series long enough for the time split, and - in a third
    of the cases - a bucket of more than SMALL_CAP candidates of many values."""
    rng = np.random.default_rng(9000 + seed)
    planted = seed % 3 == 0
    while True:
        N, T = int(rng.choice([1, 2, 3, 17])), int(rng.choice([2, 33, 1024, 4097, 6000]))
        if not planted or N * T >= 3 * SMALL_CAP:
            break
    R = int(rng.integers(1, 3))
    A = rng.standard_normal((R, N, T))
    if seed % 2:
        A = A.cumsum(axis=2)
    incs = sorted({int(i) for i in rng.integers(0, MAX_INC + 1, size=2)})
    if planted:
        A[0] = alternating(rng, N, T)
    blk = Block(A)
    jobs = []
    for r in range(R):
        for inc in incs:
            n = N * T
            ks = {0, n - 1, n // 2, max(n // 2 - 1, 0), min(n // 2 + 1, n - 1), n // 4, (3 * n) // 4,
                  int(rng.integers(0, n)), int(rng.integers(0, n))}
            if planted and r == 0:
                S = blk.sorted(0, inc)
                ids, first, count = np.unique(buckets(S), return_index=True, return_counts=True)
                many = [i for i in np.argsort(-count) if len(np.unique(S[first[i]:first[i] + count[i]])) > 1]
                b0, pop = int(first[many[0]]), int(count[many[0]])
                assert pop > SMALL_CAP, (inc, pop)        # the precondition: over-full, several values
                ks |= {b0, b0 + pop // 2, b0 + pop // 2 + 1, b0 + pop - 1, min(b0 + pop, n - 1)}
            jobs += [(r, inc, k) for k in sorted(ks)]
    blk.check(jobs, f"seed {seed}, orders {incs}, planted {planted}:")


# ------------------------------------------------------------------ end to end
def test_fit_with_time_split_equals_host_fit(fr, monkeypatch):
    """test_device_fit_equals_host_fit at a size where the selection splits the time axis: a fit
    sample of three series of 6000 elements.  The thresholds from the device's order statistics
    are bit-identical to np.quantile's on the downloaded rows."""
    X = np.random.default_rng(6000).standard_normal((3, 2, 6000)).cumsum(axis=2) / 8.0
    assert X.shape[0] < grid_of(X.shape[0], X.shape[2], 3)
    qs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("FRUITS_AMD_DEVICE_FIT", flag)
        fruit = fr.Fruit()
        fruit.add(fr.ISS([fr.words.SimpleWord(w) for w in ("[1]", "[2]", "[1][2]")]))
        fruit.add(fr.sieving.NPI(q=(0.3, 1.0), inc=1), fr.sieving.END)
        fruit.get_slice().fit_sample_size = 1.0
        np.random.seed(3)
        fruit.fit(X)
        slc = fruit.get_slice()
        # (the device fit keeps the thresholds as arrays, the host fit as a list of sieve copies)
        assert (type(slc._sieves_extended).__name__ == "_FittedRows") == (flag == "1")
        qs.append([np.asarray(row[0]._quantiles) for row in slc._sieves_extended])
    assert len(qs[0]) == len(qs[1]) == 3
    for u, v in zip(qs[0], qs[1]):
        assert np.isfinite(u[0])               # (the band's upper end, q = 1, is +inf)
        np.testing.assert_array_equal(u, v)
