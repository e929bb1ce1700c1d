"""Every route a fitted ``FruitSlice`` takes to its features (``FruitSlice._run``)
against what the commit BEFORE the three copies of the route ladder became one computed and
launched - dense, with per-series lengths, and as the word shares of 2 and 3 ranks.

``tests/golden/slice_routes_before_one_ladder.npz`` / ``.json`` were written once, on an MI355X, by
``tests/golden/make_golden_routes.py`` on a checkout of that commit; the cases, the input and the
runner are imported from there, so a case here does what the recorder did: one slice per rung of
the ladder, N = 6, D = 2, T = 260, lengths (260, 1, 64, 65, 257, 130).

Per case and mode:

* the features equal the recorded ones bit for bit - but for the ``MPI`` band columns, whose sums
  are float atomics (order varies run to run): the suite's rtol 1e-12, atol 1e-300
  (test_hip_parity.py);
* the ordered list of the stream-taking ABI entries the transform called is the recorded one: the
  same route, the same launches;
* ``fr_pipeline_set_preparation`` is called at most as often as recorded, and not at all by the
  second sharded transform of the same slice and batch shape (``Pipeline.ensure_preparation``).
"""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_golden_routes",
                                               os.path.join(GOLDEN, "make_golden_routes.py"))
routes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(routes)


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native
    _native.require_device()
    return fruits_amd


@pytest.fixture(scope="module")
def recorded():
    arrays = np.load(os.path.join(GOLDEN, routes.NAME + ".npz"))
    with open(os.path.join(GOLDEN, routes.NAME + ".json")) as f:
        record = json.load(f)
    np.testing.assert_array_equal(arrays["x"], routes.case_input())
    assert tuple(record["lengths"]) == routes.LENGTHS
    assert list(record["cases"]) == list(routes.CASES)
    return arrays, record["cases"]


def test_every_route_and_mode_is_recorded(recorded):
    """The fixture holds what the issue asks for: every case dense, the five cases the gate of a
    ragged batch admits with lengths, every single-ISS case as the shares of 2 and 3 ranks."""
    _, cases = recorded
    sharded = [f"world{w}" for w in routes.WORLDS]
    for name, (_, with_lengths) in routes.CASES.items():
        want = ["dense"] + (["ragged"] if with_lengths else []) + ([] if name == "e_chain" else sharded)
        assert list(cases[name]["modes"]) == want, name
    assert sum(with_lengths for _, with_lengths in routes.CASES.values()) == 5
    # the routes themselves, read off the recorded launches of the dense mode
    runs = {name: cases[name]["modes"]["dense"]["calls"].count("fr_pipeline_run") for name in cases}
    assert runs["a_raw"] == runs["b_raw_std_indices"] == runs["c_prepared"] == runs["d_generic"] == 1
    assert runs["h_mpi"] == 1 and runs["g_materialised"] == 0
    assert runs["e_chain"] == 4 and runs["f_ffn"] == 4       # rows of the chain in front; words
    for name in ("a_raw", "b_raw_std_indices", "h_mpi"):     # raw: no prepared tensor is written
        assert "fr_increments" not in cases[name]["modes"]["dense"]["calls"], name
    assert "fr_increments" in cases["c_prepared"]["modes"]["dense"]["calls"]


@pytest.mark.parametrize("name", list(routes.CASES))
def test_route(fr, recorded, monkeypatch, name):
    arrays, cases = recorded
    want = cases[name]
    got, labels = routes.run_case(fr, name, monkeypatch.setenv)
    assert labels == want["labels"]
    assert list(got) == list(want["modes"])
    summed = np.array(["MPI" in lb for lb in labels])
    assert summed.any() == (name == "h_mpi")
    prep = routes.SET_PREPARATION
    for mode, (feats, calls, again) in got.items():
        ref, rec = arrays[f"{name}/{mode}"], want["modes"][mode]
        print(f"[routes] {name}/{mode}: {feats.shape}, {len(calls)} ABI calls, set_preparation "
              f"{calls.count(prep)} (recorded {rec['calls'].count(prep)}), again {again} "
              f"(recorded {rec['set_preparation_again']})")
        assert feats.shape == ref.shape
        np.testing.assert_array_equal(feats[:, ~summed], ref[:, ~summed], err_msg=f"{name}/{mode}")
        np.testing.assert_allclose(feats[:, summed], ref[:, summed], rtol=1e-12, atol=1e-300,
                                   err_msg=f"{name}/{mode}")
        assert [c for c in calls if c != prep] == [c for c in rec["calls"] if c != prep], f"{name}/{mode}"
        assert calls.count(prep) <= rec["calls"].count(prep), f"{name}/{mode}"
        if mode.startswith("world"):
            assert again == 0, f"{name}/{mode}"
