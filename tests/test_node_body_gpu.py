"""The node body of the fused walk keeps its bits: every form that evaluates a trie node against
what the commit BEFORE the three node bodies of walk_fused.h became one computed.

``tests/golden/node_body_before_one_copy.npz`` was written once, on an MI355X, by
``tools/node_body_golden.py`` on a checkout of that commit (``fnode`` served the record loop, the
immediates kernel, the chain of a piece and the lean materialising walk, ``fnode_shaped`` the node
shapes of a large plan, ``fwalk_static`` the straight-line plans and the bodies of the pieces).
``meta`` holds the cases, their shapes and seeds, ``summed_run_to_run`` the largest relative
difference two runs of the recorder showed in the band-sum columns.

A case (``CASES``; the recorder imports them from here, tests/test_node_body_host.py decodes their
records) is one FORM of the walk on one word set, weighting, semiring and series length:

* ``record``      no kernel of the pipeline's own: the generic instance, family ``fused``;
* ``immediates``  ``prepare(N, plan_too=False)`` under ``fused_static=0``: the sieves as constants,
                  the plan decoded record by record, family ``fused_jit``;
* ``static``      ``prepare(N)``: the plan as straight-line code, one group per series;
* ``static_g2``   ... two groups (everywhere else the host chooses: several, for so few series);
* ``shaped``      ``pieces=0`` on a plan of more than 128 nodes: the node shapes as constants;
* ``pieces``      a plan of >= 30 nodes cut into pieces of <= 8 nodes: chains by the record loop,
                  bodies as straight-line code, family ``fused_pieces``;
* ``lean``        ``Plan.run`` on a plan of more than 32 nodes: the materialising walk with the
                  store epilogue, family ``lean``.

Lengths: 300 (one 512 piece), 1024 (a full chunk), 1025 (two chunks: the carry slots ``slot`` and
``slot + 1``).  Six series (sixteen for the shaped cases, as test_fused_jit_shaped_within_bound),
two dimensions, seeded N(0, 1) input; positive (U[0, 1) + 0.25) for Bayesian.

A feature case fits a fruit under ``sieve_set`` - a differencing sieve for the TOTALINC instances,
END - asserts the recorded thresholds, runs ``Fruit.transform``, asserts the kernel family from
``last_launch()`` (and ``jit_loaded()`` / ``pieces_loaded()``) and compares: every column bit for
bit except the band sums of real numbers (label MPI), whose wave partials meet in LDS in arrival
order - the project's bar rtol 1e-12, atol 1e-300.  The exact columns are seven of eight (at least
half: asserted).

A lean case compares the whole (K, N, T) tensor bit for bit.  The golden holds, per case, the
SHA-256 of every output row's (N, T) plane - equal digests are equal bits, and a row that moved is
named - and the values at the positions where the parts of a scan meet (``PROBES``), which say how
far it moved: seven tensors of 60 rows by 6 series by 1025 doubles are 20 MB, a committed file
holds 1 MiB."""
import hashlib
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "node_body_before_one_copy.npz")
N_SERIES, N_SHAPED, DIMS = 6, 16, 2
SUMMED = ("MPI", "CUR", "AVG", "STD")      # band sums of real numbers: wave partials, arrival order

# levels 0, 1, 2 and 3; an only child (F_CHAIN); one to four inline factors, five (the factor
# table) and a reciprocal letter (the factor table too); tests/test_node_body_host.py asserts it
WORDS = ["[1]", "[1][1]", "[1][2]", "[1][2][1]", "[12][1]", "[112][2]", "[1122][1]", "[11122][2]",
         "[1][-2][11][2]"]
# SINGLE mode: nodes without output rows, a word twice - both output rows inline in the record -
# and a word three times: the third row from the emit-row table
WORDS_SINGLE = WORDS + ["[1][-2][11][2]"] * 2 + ["[1][2]"]


def _of_weight(w, dim):
    from oracle import ref_numpy as orc
    return orc.of_weight_strings(w, dim)


def words_of(case):
    """The word strings of a case.  ``many``: more than 32 nodes in two dimensions (the lean walk's
    plans, and the plan cut into pieces): of_weight(<= 3, 2) and the words above; ``large``: more
    than 128 nodes (test_fused_bounds_gpu.py LARGE_PLAN)."""
    many = _of_weight(1, 2) + _of_weight(2, 2) + _of_weight(3, 2)
    return {"small": WORDS, "single": WORDS_SINGLE,
            "many": many + [w for w in WORDS if w not in many],
            "many_single": many + [w for w in WORDS_SINGLE if w not in many],
            "large": _of_weight(5, 2)[::4] + ["[1][-2][11][2]"]}[case["words"]]


W_INDICES = {"kind": "Indices", "scale": 2.0}
W_TOTAL = {"kind": "Indices", "scale": 2.0, "total": True}
WEIGHTINGS = {"none": None, "indices": W_INDICES, "total": W_TOTAL}
FORMS = {
    # form: (family, FRUITS_HIP_DEBUG, groups per series - 0: the host's own choice, several)
    "record": ("fused", "packed=0", 0),
    "immediates": ("fused_jit", "packed=0,fused_static=0", 0),
    "static": ("fused_jit", "packed=0,groups=1", 1),
    "static_g2": ("fused_jit", "packed=0,groups=2", 2),
    "shaped": ("fused_jit", "packed=0,pieces=0", 0),
    "pieces": ("fused_pieces", "packed=0,pieces=1,piece_min=30,piece_nodes=8", 0),
    "lean": ("lean", "packed=0", 0),
}


def _case(form, weighting, T, semiring="Reals", words=None, single=False):
    words = words or {"shaped": "large", "pieces": "many", "lean": "many"}.get(form, "small")
    if single:
        words = "many_single" if words == "many" else "single"
    name = "_".join([form, weighting] + ([semiring.lower()] if semiring != "Reals" else [])
                    + (["single"] if single else []) + [f"T{T}"])
    return dict(name=name, form=form, weighting=weighting, T=T, semiring=semiring, words=words,
                single=single, family=FORMS[form][0], debug=FORMS[form][1], groups=FORMS[form][2],
                N=N_SHAPED if form == "shaped" else N_SERIES)


def _cases():
    out = []
    # Reals on every form: no weighting, the second scan (Indices), the total rescale
    lengths = {"record": (300, 1024, 1025), "immediates": (1024, 300, 1025), "static": (300, 1025, 1024),
               "static_g2": (1025, 300, 1024), "shaped": (300, 1025, 1024), "pieces": (1025, 300, 1024),
               "lean": (300, 1025, 1024)}
    for form, Ts in lengths.items():
        for weighting, T in zip(WEIGHTINGS, Ts):
            out.append(_case(form, weighting, T))
    out.append(_case("record", "indices", 1025))      # (the second scan's carry slot, record loop)
    # Arctic, Bayesian and SINGLE mode on the record loop, the straight-line form and the lean walk
    for form, Ts in (("record", (1025, 300, 1025, 300)), ("static", (1024, 1025, 300, 1025)),
                     ("lean", (1025, 1024, 1025, 300))):
        out.append(_case(form, "none", Ts[0], semiring="Arctic"))
        out.append(_case(form, "none", Ts[1], semiring="Bayesian"))
        out.append(_case(form, "indices", Ts[2], single=True))
        out.append(_case(form, "total", Ts[3], semiring="Arctic"))
    return out


CASES = _cases()


def make_iss(fr, case):
    spec = WEIGHTINGS[case["weighting"]]
    weighting = None if spec is None else getattr(fr.iss.weighting, spec["kind"])(
        **{k: v for k, v in spec.items() if k != "kind"})
    return fr.ISS([fr.words.SimpleWord(s) for s in words_of(case)],
                  mode=fr.ISSMode.SINGLE if case["single"] else fr.ISSMode.EXTENDED,
                  semiring=getattr(fr.semiring, case["semiring"])(), weighting=weighting)


def sieve_set(fr, T):
    S = fr.sieving
    c = max(T // 3, 1)
    return [S.NPI(inc=0, q=(0.25, 0.75)), S.NPI(inc=1), S.NPI(inc=2, q=(0.5, 1.0)), S.XPI(q=(0.5, 1.0)),
            S.MAX(cut=[c, -1], q=(0.1, 0.9)), S.MIN(cut=[c, -1], q=(0.1, 0.9)), S.END(),
            S.MPI(inc=1, q=(0.25, 1.0))]


def case_input(case):
    N, T = case["N"], case["T"]
    rng = np.random.default_rng([CASES.index(case), N, T])
    return rng.random((N, DIMS, T)) + 0.25 if case["semiring"] == "Bayesian" else rng.standard_normal((N, DIMS, T))


PROBES = (0, 1, 63, 64, 255, 256, 511, 512, 1023, 1024)


def probe_positions(T):
    return np.array(sorted({p for p in PROBES if p < T} | {T - 1}))


def row_digests(out):
    """(K, 32) uint8: the SHA-256 of every output row's (N, T) plane of a (K, N, T) tensor."""
    out = np.ascontiguousarray(out)
    return np.stack([np.frombuffer(hashlib.sha256(out[k].tobytes()).digest(), dtype=np.uint8)
                     for k in range(out.shape[0])])


def run_lean(fr, case, setenv):
    """The (K, N, T) tensor of a lean case; asserts the kernel family."""
    import torch
    from fruits_amd import _native as nat
    setenv("FRUITS_HIP_JIT", "0")
    setenv("FRUITS_HIP_DEBUG", case["debug"])
    X = case_input(case)
    iss = make_iss(fr, case)
    plan = iss._plan(0, len(iss.words))
    assert plan.nodes > 32, case["name"]
    iss._attach_cache(X)
    Xd = nat.to_device(X)
    out = plan.run(Xd, iss.lookup_device(Xd))
    torch.cuda.synchronize()
    ran = plan.last_launch()
    assert ran["family"] == "lean", (case["name"], ran)
    got = nat.to_host(out)
    assert got.shape == (plan.rows, case["N"], case["T"])
    return got


def run_features(fr, case, setenv):
    """(thresholds, (N, F) features, feature labels) of a feature case; asserts the kernel."""
    from test_epilogue_gpu import fitted_thresholds
    setenv("FRUITS_AMD_AUTO_PREPARE", "0")
    setenv("FRUITS_HIP_JIT", "1")
    setenv("FRUITS_HIP_DEBUG", case["debug"])
    T, N, form = case["T"], case["N"], case["form"]
    X = case_input(case)
    fruit = fr.Fruit(case["name"])
    fruit.add(make_iss(fr, case))
    fruit.add(*sieve_set(fr, T))
    slc = fruit.get_slice()
    slc.fit_sample_size = 1.0
    np.random.seed(4)
    fruit.fit(X)
    thresholds = fitted_thresholds(slc)
    pipe = slc._fused(T)
    assert pipe is not None, case["name"]
    assert pipe.jit_loaded() == 0 and pipe.pieces_loaded() == 0
    if form == "shaped":
        assert pipe.plan.nodes > 128
    elif form == "pieces":
        cover = pipe.plan.pieces(8)
        assert pipe.plan.nodes >= 30 and cover is not None and len(cover["types"]) >= 2
    else:
        assert pipe.plan.nodes <= 128
    if form != "record":
        pipe.prepare(N, plan_too=form != "immediates")
    feats = fruit.transform(X)
    assert slc._fused(T) is pipe
    ran = pipe.last_launch()
    assert ran["family"] == case["family"] and case["groups"] in (0, ran["G"]), (case["name"], ran)
    if form == "record":
        assert pipe.jit_loaded() == 0 and pipe.pieces_loaded() == 0
    elif form == "immediates":
        assert pipe.jit_loaded() >= 1 and pipe.jit_loaded(static_only=True) == 0 and pipe.pieces_loaded() == 0
    elif form == "pieces":
        assert pipe.pieces_loaded() == len(cover["types"])
    else:
        assert pipe.jit_loaded(static_only=True) == 1 and pipe.pieces_loaded() == 0
    labels = [fruit.label(i) for i in range(fruit.nfeatures())]
    assert feats.shape == (N, len(labels)) and np.isfinite(feats).all()
    return thresholds, feats, labels


def summed_columns(labels):
    """The band-sum columns: the kind is the first three letters of a label's last part."""
    return np.array([lb.rsplit(" | ", 1)[-1][:3] in SUMMED for lb in labels])


def largest_relative(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
    return float(np.nanmax(rel, initial=0.0))


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_the_golden_holds_these_cases(golden):
    meta = json.loads(str(golden["meta"]))
    assert [c["name"] for c in meta["cases"]] == [c["name"] for c in CASES]
    for c in CASES:
        keys = ("digests", "probes") if c["form"] == "lean" else ("features", "thresholds")
        assert all(c["name"] + "/" + k in golden for k in keys), c["name"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_node_body_keeps_its_bits(fr, golden, monkeypatch, case):
    t0 = time.perf_counter()
    name = case["name"]
    if case["form"] == "lean":
        got = run_lean(fr, case, monkeypatch.setenv)
        at = probe_positions(case["T"])
        digests = row_digests(got)
        moved = np.flatnonzero((digests != golden[name + "/digests"]).any(axis=1))
        print(f"node body {name}: tensor {got.shape}, rows that moved: {moved.tolist()}, largest relative "
              f"difference at the probes {largest_relative(got[:, :, at], golden[name + '/probes']):.3g} "
              f"seconds={time.perf_counter() - t0:.2f}")
        np.testing.assert_array_equal(got[:, :, at], golden[name + "/probes"], err_msg=name + ": probes")
        np.testing.assert_array_equal(digests, golden[name + "/digests"], err_msg=name + ": row digests")
        return
    if case["form"] != "record":
        from test_hip_parity import _require_hiprtc
        strs = ["[1][2]", "[11][2][1]"]          # (test_epilogue_gpu.py's: any plan with a static schedule)
        _require_hiprtc(fr.ISS([fr.words.SimpleWord(s) for s in strs], mode=fr.ISSMode.EXTENDED)._plan(0, 2))
    thresholds, feats, labels = run_features(fr, case, monkeypatch.setenv)
    np.testing.assert_array_equal(thresholds, golden[name + "/thresholds"], err_msg=name + ": thresholds")
    want = golden[name + "/features"]
    assert feats.shape == want.shape, name
    summed = summed_columns(labels)
    assert 2 * int((~summed).sum()) >= len(labels) and summed.any(), name
    moved = largest_relative(feats[:, summed], want[:, summed])
    print(f"node body {name}: F={len(labels)} exact={int((~summed).sum())} summed={int(summed.sum())} "
          f"largest relative difference {moved:.3g} (two runs of the recorder: "
          f"{float(golden['summed_run_to_run']):.3g}) seconds={time.perf_counter() - t0:.2f}")
    for c in np.flatnonzero(~summed):
        np.testing.assert_array_equal(feats[:, c], want[:, c], err_msg=f"{name}: {labels[c]}")
    np.testing.assert_allclose(feats[:, summed], want[:, summed], rtol=1e-12, atol=1e-300, err_msg=name)
