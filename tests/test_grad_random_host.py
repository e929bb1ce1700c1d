"""The random cases of the backward-pass tests (tests/grad_random.py) without a GPU: the generator
is a pure function of the seed, every default seed of every kind ends in admitted exact inputs,
the default seeds hold what the curated word sets lack, and the long-double oracles of the three
adjoint recursions equal the definitions in exact arithmetic on random tiny cases."""
import numpy as np
import pytest

import grad_random as rnd
import iss_grad_max_ref as gm
import iss_grad_ref as gr
import iss_grad_weighted_ref as gw

SEEDS = range(rnd.DEFAULT_SEEDS)
TINY_SEEDS = range(50)


# ---------------------------------------------------------------- determinism and admission
def test_case_is_a_pure_function_of_the_seed():
    for seed in (0, 7, 23, 199):
        a, b = rnd._make(seed, False), rnd._make(seed, False)
        assert a == b and a is not b and rnd.case(seed) == a
        assert rnd.sieves_of(a) == rnd.sieves_of(b)
        for kind in ("reals", "bayesian"):
            xa, ga, _ = rnd.real_inputs(a, kind)
            rnd._REAL.clear()
            xb, gb, _ = rnd.real_inputs(b, kind)
            assert np.array_equal(xa, xb) and np.array_equal(ga, gb)
        assert f"case({seed})" in a.describe() and str(list(a.strings)) in a.describe()
    assert rnd.case(0) != rnd.case(1)
    # the shapes come from the pools; 261 series only on the short lengths
    for seed in range(3 * len(rnd.T_POOL)):
        c = rnd.case(seed)
        assert c.T in rnd.T_POOL and c.N in rnd.N_POOL and 1 <= c.D <= 6, c.describe()
        assert c.N != 261 or c.T <= 257, c.describe()
        assert 1 <= len(c.strings) <= 12 + 4 + 8 and all(1 <= len(a) <= 6 for a in c.alphas)
        assert len({a for al in c.alphas for a in al}) <= rnd.ALPHA_POOL
        assert all(0.25 <= a <= 2.0 and np.float32(a) == a for al in c.alphas for a in al)


def test_every_default_seed_is_admitted(capsys):
    """``exact_inputs`` ends in an admitted case for every default seed and kind - none is left
    out - by the conditions of its docstring, checked here again from the references."""
    reduced = {}
    for seed in SEEDS:
        c = rnd.case(seed)
        for kind in rnd.KINDS:
            e = rnd.exact_inputs(c, kind)
            short = e.case(c)
            K = len(rnd.rows_of(c))
            assert e.X.shape == (c.N, c.D, e.T) and e.G.shape == (c.N, K, e.T), c.describe()
            assert e.T in rnd.T_POOL and e.T <= c.T and e.N == c.N
            assert e.reduced == (e.stage > 0 or e.T != c.T)
            assert all((a == 0).all() for a in e.alphas)
            assert (e.G == np.round(e.G)).all() and np.abs(e.G).max(initial=0) <= 3
            group = rnd.GROUP[kind]
            if group == "arctic":
                assert (e.X == np.round(e.X)).all() and not e.reduced
                continue
            assert max(rnd.magnitudes(short, group, e.X, e.G)) * 2.0 ** e.q <= 2.0 ** 53, c.describe()
            W = rnd.heaviest(c)
            if group == "bayesian":
                assert e.q == (2 * (W + 1), W + 1, 0)[e.stage]
                lo = (0.25, 0.5, 1.0)[e.stage]
                assert (np.log2(e.X) == np.round(np.log2(e.X))).all() and e.X.min() >= lo and e.X.max() <= 2
            else:
                assert e.q == W + 1
                assert set(np.unique(np.abs(e.X))) <= ({0.0, 0.5, 1.0, 2.0} if e.stage == 0 else {0.0, 1.0})
                assert all((e.X[:, d] != 0).all() for d in rnd.divided(c))
            reduced[group] = reduced.get(group, 0) + e.reduced
    with capsys.disabled():
        print(f"\ngrad_random: {len(SEEDS)} default seeds x {len(rnd.KINDS)} kinds admitted, 0 left out; "
              "reduced (alphabet narrowed or T moved down): "
              + ", ".join(f"{g} {n // (3 if g == 'reals' else 1)}" for g, n in sorted(reduced.items())))


# ---------------------------------------------------------------- coverage, from the generator alone
def test_default_seeds_cover_what_the_curated_sets_lack(capsys):
    counts, lengths, batches = {}, {}, {}
    for seed in SEEDS:
        c = rnd.case(seed)
        for name, holds in rnd.coverage(c).items():
            counts[name] = counts.get(name, 0) + bool(holds)
        lengths[c.T] = lengths.get(c.T, 0) + 1
        batches[c.N] = batches.get(c.N, 0) + 1
    with capsys.disabled():
        print(f"\ngrad_random coverage over the {len(SEEDS)} default seeds:")
        for name, n in counts.items():
            print(f"  {n:3d}  {name}")
        print("  T: " + ", ".join(f"{t} x{lengths.get(t, 0)}" for t in rnd.T_POOL))
        print("  N: " + ", ".join(f"{n} x{batches.get(n, 0)}" for n in rnd.N_POOL))
    assert len(counts) == 13
    for name, n in counts.items():
        assert n >= 2, f"{name}: {n} of the default seeds"
    for n in rnd.N_POOL:
        assert batches.get(n, 0) >= 2, f"N = {n}: {batches.get(n, 0)} of the default seeds"
    # 24 cases hold 24 lengths, the list has 23: each cannot occur twice.  The generator takes
    # them in turn - every one at least once in the default seeds, and twice in twice as many
    for t in rnd.T_POOL:
        assert lengths.get(t, 0) >= 1, f"T = {t}: none of the default seeds"
    twice = {}
    for seed in range(2 * len(rnd.T_POOL)):
        twice[rnd.case(seed).T] = twice.get(rnd.case(seed).T, 0) + 1
    assert all(twice[t] == 2 for t in rnd.T_POOL)


def test_coverage_reads_the_words():
    c = rnd.Case(0, 1, 4, 5, "SINGLE", ("[1-1][2]", "[111][2-2]", "[111]", "[111]", "[111]", "[1-2-23]"),
                 ((1.0, 1.0),) * 2 + ((1.0,),) * 4)
    cov = rnd.coverage(c)
    assert cov["an exponent >= 3"] and cov["an exponent <= -2"] and cov["a letter of mixed sign"]
    assert cov["a letter over >= 3 dimensions"] and cov["an empty letter at depth 1"]
    assert cov["an empty letter at depth >= 2"] and cov["a node that is >= 3 output rows"]
    assert cov["a SINGLE-mode inner node that is no row"] and cov["an inner node that is a row"]
    assert cov["a dimension that no word names"]
    assert not cov["a trie of depth 5"] and not cov["a node with >= 5 children"]
    # the oracles' view of an empty letter: a letter without exponents
    assert gr.output_prefixes(["[1-1][2]"])[0] == ((), (0, 1))
    assert rnd.heaviest(c) == 4 and rnd.divided(c) == [1]


def test_sieves_of_a_case():
    import features_grad_ref as fg
    for seed in range(2 * len(rnd.T_POOL)):
        c = rnd.case(seed)
        specs = rnd.sieves_of(c)
        assert 1 <= len(specs) <= 5 and 1 <= rnd.nfeatures(specs) <= 256, c.describe()
        assert rnd.nfeatures(specs) == fg.nfeatures(rnd.reference_specs(specs))
        cuts = [cut for _, cs, _ in specs for cut in cs]
        assert -1 in cuts and all(cut == -1 or 1 <= cut < c.T for cut in cuts)
        assert all(len(set(cs)) == len(cs) >= 1 for _, cs, _ in specs)
        if c.T >= 2:
            assert any(len(cs) >= 2 for _, cs, _ in specs), c.describe()
        for edge in (rnd.CHUNK, rnd.CHUNK + 1):
            assert (edge in specs[0][1]) == (edge < c.T), c.describe()
    full = rnd.full_sieves(300)
    assert rnd.nfeatures(full) == fg.nfeatures(rnd.reference_specs(full)) == 256


def test_at_least_half_of_the_max_cases_have_ties():
    """The exact inputs of the max semirings are there for the tie rule: of the default seeds at
    least half have an exact tie (``smallest_gap == 0.0``), per semiring."""
    for kind, semiring in (("arctic", "Arctic"), ("bayesian", "Bayesian")):
        ties = 0
        for seed in SEEDS:
            c = rnd.case(seed)
            e = rnd.exact_inputs(c, kind)
            ties += gm.smallest_gap(e.X, list(c.strings), c.mode, semiring) == 0.0
        assert 2 * ties >= len(SEEDS), (kind, ties)


# ---------------------------------------------------------------- the oracles on random tiny cases
def power_tables(T, seed):
    """Exp tables of exact powers of two for the alphas 1 and 2 (tests/test_grad_weighted_host.py)."""
    j = np.cumsum(np.random.default_rng([seed, T]).integers(0, 2, size=T)).astype(np.float64)
    return ({a: 2.0 ** (a * j) for a in (1.0, 2.0)}, {a: 2.0 ** (-a * j) for a in (1.0, 2.0)})


@pytest.mark.parametrize("seed", TINY_SEEDS)
def test_oracles_equal_the_definitions_on_random_tiny_cases(seed):
    """``iss_grad``, ``iss_grad_max`` and ``iss_grad_weighted`` against the brute-force definitions
    in exact rationals: the full letter alphabet - exponents to +-4, mixed signs, empty letters -
    in up to three letters on T <= 6."""
    c = rnd.tiny_case(seed)
    strings, what = list(c.strings), c.describe()
    assert c.T <= 6 and all(len(r) <= 3 for r in rnd.rows_of(c))
    e = rnd.exact_inputs(c, "reals")
    want = gr.grad_bruteforce(e.X, e.G, strings, c.mode)
    got = gr.as_fractions(gr.iss_grad(e.X, e.G, strings, c.mode))
    assert (got == want).all(), f"iss_grad {what}"
    # weighted, both bodies, with the case's alphas (1 and 2) and tables of powers of two
    alphas = c.alpha_arrays()
    Ep, Em = power_tables(c.T, seed)
    assert len(gw.output_nodes(strings, alphas, c.mode)) == e.G.shape[1]
    for total in (False, True):
        want = gw.grad_weighted_bruteforce(e.X, e.G, strings, alphas, Ep, Em, total, c.mode)
        got = gr.as_fractions(gw.iss_grad_weighted(e.X, e.G, strings, alphas, None, total, c.mode,
                                                   tables=(Ep, Em)))
        assert (got == want).all(), f"iss_grad_weighted total={total} {what}"
    for kind, semiring in (("arctic", "Arctic"), ("bayesian", "Bayesian")):
        e = rnd.exact_inputs(c, kind)
        want = gm.grad_max_bruteforce(e.X, e.G, strings, c.mode, semiring)
        got = gr.as_fractions(gm.iss_grad_max(e.X, e.G, strings, c.mode, semiring))
        assert (got == want).all(), f"iss_grad_max {semiring} {what}"


def test_tiny_cases_keep_the_alphabet():
    cases = [rnd.tiny_case(seed) for seed in TINY_SEEDS]
    exps = [e for c in cases for v in rnd.nodes_of(c) for e in v[-1]]
    assert max(exps) == 4 and min(exps) <= -3
    assert sum(rnd.coverage(c)["an empty letter at depth 1"] for c in cases) >= 2
    assert sum(rnd.coverage(c)["an empty letter at depth >= 2"] for c in cases) >= 2
    assert {c.T for c in cases} == {1, 2, 3, 4, 5, 6}
    assert all(a in (1.0, 2.0) for c in cases for al in c.alphas for a in al)
