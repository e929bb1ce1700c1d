"""The mixed static launch changes no value: whole-series units of the one-group program in front,
the finer units of the same plan's multi-group program (its tail program) behind them.  Every case
runs one plan on one input with FRUITS_HIP_DEBUG tail=0 (never mixed) and with the forced or the
default split; the (K, N, T) tensors are bit-identical, the first two and the last two series (the
last ones are tail series) agree with the oracle, and the plan reports how many series the launch
split (fr_plan_info, FR_INFO_STATIC_TAIL)."""
import numpy as np
import pytest

from conftest import gen_input

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fr():
    import fruits_amd
    from fruits_amd import _native as nat
    nat.require_device()
    return fruits_amd


def _both_ways(fr, monkeypatch, iss, words, X, knob, note):
    """(tensor rows of series 0, 1, N-2, N-1 of the split run; series split without / with it)."""
    import torch
    from fruits_amd import _native as nat
    N, _, T = X.shape
    Xd = nat.to_device(X)
    plan = iss._plan(0, len(words))
    plan.prepare(N, T)
    out, split = {}, {}
    for arm in ("off", "on"):
        if arm == "off":
            monkeypatch.setenv("FRUITS_HIP_DEBUG", "tail=0")
        elif knob is None:
            monkeypatch.delenv("FRUITS_HIP_DEBUG", raising=False)
        else:
            monkeypatch.setenv("FRUITS_HIP_DEBUG", f"tail={knob}")
        buf = torch.full((plan.rows, N, T), float("nan"), dtype=torch.float64, device=Xd.device)
        plan.run(Xd, None, out=buf)
        torch.cuda.synchronize()
        out[arm] = buf
        split[arm] = plan.static_tail_series()
    monkeypatch.delenv("FRUITS_HIP_DEBUG", raising=False)
    a, b = out["off"], out["on"]
    assert not torch.isnan(a).any(), note
    assert not torch.isnan(b).any(), note
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), note
    return nat.to_host(b[:, [0, 1, N - 2, N - 1]]), split["off"], split["on"]


def _check_oracle(X, words, mode, ends):
    from oracle import ref_numpy as orc
    N = X.shape[0]
    ref = orc.iss_transform(X[[0, 1, N - 2, N - 1]], [str(w) for w in words], mode)
    scale = np.abs(ref).max(axis=2, keepdims=True)
    assert np.max(np.abs(ends - ref) / scale) < 1e-9


@pytest.mark.parametrize("N,T,knob,expect", [
    (24, 1024, 8, 8),        # XCD-aware decode of the tail (S % 8 == 0), whole part non-empty
    (21, 1024, 5, 5),        # plain decode, odd counts
    (16, 1024, 16, 16),      # no whole part
    (16, 1024, 1, 1),        # a single split series
    (24, 600, 8, 8),         # ragged chunk through both programs
    (2048, 1024, None, 512),   # the default rule: the mixed launch is what runs (1536 resident)
    (1537, 1024, None, 1),     # S = 1
    (1536, 1024, None, 0),     # one resident round: no tail, unchanged
])
def test_of_weight_2_3_extended(fr, monkeypatch, N, T, knob, expect):
    words = fr.words.of_weight(2, dim=3)
    X = gen_input({"seed": 3 * N + T, "dist": "normal", "shape": [N, 3, T]})
    iss = fr.ISS(words, mode=fr.ISSMode.EXTENDED)
    ends, off, on = _both_ways(fr, monkeypatch, iss, words, X, knob, f"N={N} T={T} tail={knob}")
    assert off == 0
    assert on == expect
    _check_oracle(X, words, "EXTENDED", ends)


@pytest.mark.parametrize("weight,dim,mode,expect", [
    (2, 2, "SINGLE", 8),      # programs 13 / 14: another pair, SINGLE-mode emits
    (3, 1, "EXTENDED", 8),    # programs 19 / 20: groups of unequal length, one staged row
    (1, 1, "EXTENDED", 0),    # program 0 has no tail program: the knob is ignored
])
def test_other_word_sets(fr, monkeypatch, weight, dim, mode, expect):
    words = fr.words.of_weight(weight, dim=dim)
    X = gen_input({"seed": 10 * weight + dim, "dist": "normal", "shape": [24, dim, 1024]})
    iss = fr.ISS(words, mode=getattr(fr.ISSMode, mode))
    plan = iss._plan(0, len(words))
    assert plan.static_program_index() > 0
    ends, off, on = _both_ways(fr, monkeypatch, iss, words, X, 8, f"of_weight({weight},{dim}) {mode}")
    assert off == 0
    assert on == expect
    _check_oracle(X, words, mode, ends)


def test_run_time_compiled_program_ignores_the_knob(fr, monkeypatch, tmp_path):
    """The 7-word plan of test_jit_static_bit_identical: its static program is compiled at run time
    and has no tail program."""
    monkeypatch.setenv("FRUITS_HIP_JIT_CACHE", str(tmp_path / "jit"))
    monkeypatch.setenv("FRUITS_HIP_JIT", "1")
    strs = ["[1][2]", "[12][1]", "[2]", "[1][1][2]", "[3][1]", "[33]", "[2][3][1]"]
    words = [fr.words.SimpleWord(s) for s in strs]
    N = 1601
    X = gen_input({"seed": N, "dist": "normal", "shape": [N, 3, 1024]})
    iss = fr.ISS(words, mode=fr.ISSMode.EXTENDED)
    ends, off, on = _both_ways(fr, monkeypatch, iss, words, X, 64, "jit")
    assert iss._plan(0, len(words)).jit_loaded() > 0
    assert off == 0 and on == 0
    _check_oracle(X, words, "EXTENDED", ends)
