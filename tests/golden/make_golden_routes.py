"""Recorder of tests/golden/slice_routes_before_one_ladder.{npz,json}: one slice per route a
fitted ``FruitSlice`` can take to its features, transformed dense, with per-series lengths and as
the word shares of 2 and 3 ranks.

The two files were written ONCE, on an MI355X, by this script on a checkout of commit c0a6229
("Per-series lengths in the differentiable ISS: a ragged backward pass") - the commit before the
three copies of the route ladder (``FruitSlice.transform_device``, ``_transform_ragged``,
``parallel._device_block``) became one.  It uses only names both commits have: ``Fruit.fit``,
``Fruit.transform(lengths=)``, ``parallel.shard_words``, ``column_map``, ``_device_block``.
tests/test_slice_routes_gpu.py imports the cases and the runner from here, so the test does what
the recorder did.

    python tests/golden/make_golden_routes.py [directory]

npz: ``<case>/<mode>`` the (N, F) features, ``x`` the input.  json: per ``<case>/<mode>`` the
ordered ABI entries the transform called - those that take a stream (include/fruits_hip.h) and
``fr_pipeline_set_preparation`` - and, for the sharded modes, how many times the SECOND transform
of the same slice and batch called ``fr_pipeline_set_preparation``; ``labels`` per case.
"""
import contextlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
NAME = "slice_routes_before_one_ladder"

N, D, T = 6, 2, 260
LENGTHS = (260, 1, 64, 65, 257, 130)       # (257: across the 256-step chunk boundary)
WORLDS = (2, 3)
SET_PREPARATION = "fr_pipeline_set_preparation"

# name -> (what the slice is, whether it also runs with per-series lengths)
CASES = {
    "a_raw": ("INC -> ISS(of_weight(2, 2)) -> NPI, END: one launch on the raw batch", True),
    "b_raw_std_indices": ("INC, STD -> ISS weighted by Indices -> NPI, END: raw batch, with lookup", True),
    "c_prepared": ("STD, INC (no fused chain) -> ISS -> NPI, END: one launch on the prepared input", True),
    "d_generic": ("INC -> ISS of generic words over Reals -> NPI, END: virtual rows", False),
    "e_chain": ("INC -> ISS -> ISS weighted -> NPI, END: one launch per row of the chain", False),
    "f_ffn": ("INC -> CosWISS with the randomised ffn -> NPI, END: word by word", False),
    "g_materialised": ("INC -> ISS -> NPI, LPI, END: LPI does not fuse", True),
    "h_mpi": ("INC -> ISS -> MPI, NPI, END: band sums", True),
}


def case_input():
    return np.random.default_rng([N, D, T]).standard_normal((N, D, T))


def build_fruit(fr, name):
    """The fitted fruit (one slice) of case ``name``."""
    P, S, W = fr.preparation, fr.sieving, fr.words
    fruit = fr.Fruit(name)
    simple = W.of_weight(2, dim=2)
    default_sieves = [S.NPI(q=(0.5, 1.0)), S.END()]
    if name == "a_raw":
        seeds = [P.INC(), fr.ISS(simple), *default_sieves]
    elif name == "b_raw_std_indices":
        seeds = [P.INC(), P.STD(), fr.ISS(simple, weighting=fr.iss.weighting.Indices(scale=2.0)),
                 *default_sieves]
    elif name == "c_prepared":
        seeds = [P.STD(), P.INC(), fr.ISS(simple), *default_sieves]
    elif name == "d_generic":
        if "routes_sq" not in W.letters.get_available():     # (a letter evaluated on the host)
            W.letter(name="routes_sq")(lambda X, i: X[i, :] ** 2)
        built = W.Word("no brackets")
        for body in ("ABS(1)", "DIM(2)"):
            built.multiply(W.ExtendedLetter(body))
        generic = [built, W.Word("[DIM(1)DIM(2)]"), W.Word("[ABS(2)]"), W.Word("[ABS(1)][routes_sq(2)ABS(1)]")]
        seeds = [P.INC(), fr.ISS(generic, mode=fr.ISSMode.EXTENDED), *default_sieves]
    elif name == "e_chain":
        seeds = [P.INC(),
                 fr.ISS([W.SimpleWord(s) for s in ("[1]", "[12]", "[2][1]")], mode=fr.ISSMode.EXTENDED),
                 fr.ISS([W.SimpleWord(s) for s in ("[1]", "[1][1]", "[11]")],
                        weighting=fr.iss.weighting.Indices(scale=2.0)),
                 *default_sieves]
    elif name == "f_ffn":
        seeds = [P.INC(),
                 fr.CosWISS(freqs=[0.1, 0.35], words=[W.SimpleWord(s) for s in ("[1]", "[1][2]", "[2][1][1]", "[2]")],
                            exponent=2, ffn_size=5),
                 *default_sieves]
    elif name == "g_materialised":
        seeds = [P.INC(), fr.ISS(simple), S.NPI(q=(0.5, 1.0)), S.LPI(q=(0.5, 1.0)), S.END()]
    elif name == "h_mpi":
        seeds = [P.INC(), fr.ISS(simple), S.MPI(q=(0.5, 1.0)), *default_sieves]
    else:
        raise KeyError(name)
    fruit.add(*seeds)
    fruit.get_slice().fit_sample_size = 1.0
    np.random.seed(list(CASES).index(name))
    fruit.fit(case_input())
    return fruit


def stream_entries():
    """The entries of include/fruits_hip.h with a ``void *stream`` parameter."""
    with open(os.path.join(ROOT, "include", "fruits_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return [name for name, args in re.findall(r"\b(fr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\bvoid\s*\*\s*stream\b", args)]


@contextlib.contextmanager
def abi_calls(nat):
    """The ordered list of the ABI entries called inside the block: the functions of the loaded
    library wrapped (as tests/test_streams_gpu.py wraps them), and put back."""
    L, seen, kept = nat.lib(), [], {}
    for name in [*stream_entries(), SET_PREPARATION]:
        kept[name] = getattr(L, name)

        def spy(*a, _o=kept[name], _n=name):
            seen.append(_n)
            return _o(*a)
        setattr(L, name, spy)
    try:
        yield seen
    finally:
        for name, fn in kept.items():
            setattr(L, name, fn)


def sharded(fr, slc, X, world):
    """The slice's features from the shares of ``world`` ranks, rank after rank on one device,
    reassembled through ``column_map`` (tests/test_hip_parity.py, word-sharded cases)."""
    from fruits_amd import parallel as par
    from fruits_amd.cache import SharedSeedCache
    iss = slc.get_iss()[0]
    strings = [str(w) for w in iss.words]
    depths = [iss._depth(i) for i in range(len(strings))]
    per_sum = sum(s.nfeatures() for s in slc.get_sieves())
    parts = par.shard_words(strings, depths, world)
    maps = par.column_map(parts, depths, per_sum)
    out = np.zeros((X.shape[0], slc.nfeatures()))
    for r in range(world):
        cache = SharedSeedCache(X)
        block = par._device_block(slc, iss, cache.input_device(X), cache, parts[r], depths, per_sum)
        assert block.shape[1] == len(maps[r])
        out[:, maps[r]] = block.cpu().numpy()
    return np.nan_to_num(out)


def modes_of(fruit, name):
    out = ["dense"] + (["ragged"] if CASES[name][1] else [])
    if len(fruit.get_slice().get_iss()) == 1:
        out += [f"world{w}" for w in WORLDS]
    return out


def run_case(fr, name, setenv=os.environ.__setitem__):
    """{mode: (features, ABI calls, set_preparation calls of a second sharded transform or None)}
    of case ``name``, the modes in this fixed order on ONE fitted fruit, and its labels."""
    from fruits_amd import _native as nat
    # (the library's own kernel instances, nothing compiled at run time: what a launch takes must
    # not depend on the machine's disk cache)
    setenv("FRUITS_HIP_JIT", "0")
    setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    X = case_input()
    fruit = build_fruit(fr, name)
    slc = fruit.get_slice()
    out = {}
    for mode in modes_of(fruit, name):
        again = None
        with abi_calls(nat) as calls:
            if mode == "dense":
                feats = fruit.transform(X)
            elif mode == "ragged":
                feats = fruit.transform(X, lengths=np.array(LENGTHS))
            else:
                feats = sharded(fr, slc, X, int(mode[5:]))
        if mode.startswith("world"):
            with abi_calls(nat) as second:
                np.testing.assert_allclose(sharded(fr, slc, X, int(mode[5:])), feats, rtol=1e-12, atol=1e-300)
            again = second.count(SET_PREPARATION)
        out[mode] = (feats, list(calls), again)
    return out, [fruit.label(i) for i in range(fruit.nfeatures())]


def main(out_dir):
    sys.path.insert(0, ROOT)
    import fruits_amd as fr
    from fruits_amd import _native as nat
    nat.require_device()
    arrays, record = {"x": case_input()}, {"lengths": list(LENGTHS), "cases": {}}
    for name in CASES:
        got, labels = run_case(fr, name)
        record["cases"][name] = {"labels": labels, "modes": {}}
        for mode, (feats, calls, again) in got.items():
            arrays[f"{name}/{mode}"] = feats
            record["cases"][name]["modes"][mode] = {"calls": calls, "set_preparation_again": again}
            print(f"{name}/{mode}: {feats.shape}, {len(calls)} calls "
                  f"({calls.count(SET_PREPARATION)} set_preparation, again {again}): "
                  f"{[c for c in calls if c != 'fr_memcpy_h2d']}")
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, NAME + ".npz"), **arrays)
    with open(os.path.join(out_dir, NAME + ".json"), "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
