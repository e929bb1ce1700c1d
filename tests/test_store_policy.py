"""The cache policy of the output stores changes no value: the (K, N, T) tensor is bit-identical
with the write-through instances of the static programs (the default, FRUITS_HIP_DEBUG unset) and
without them (wt=0), on every materialising path and on both sides of the windows where the host
asks for them."""
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


def _both_ways(fr, monkeypatch, words, X, dim_note="", iss=None):
    """The tensor without and with the write-through instances (same plan, same input)."""
    import torch
    from fruits_amd import _native as nat
    N, _, T = X.shape
    Xd = nat.to_device(X)
    iss = iss or fr.ISS(words, mode=fr.ISSMode.EXTENDED)
    plan = iss._plan(0, len(words))
    plan.prepare(N, T)
    out = {}
    for wt in ("0", "1"):
        monkeypatch.setenv("FRUITS_HIP_DEBUG", f"wt={wt}")
        buf = torch.full((plan.rows, N, T), float("nan"), dtype=torch.float64, device=Xd.device)
        plan.run(Xd, None, out=buf)
        torch.cuda.synchronize()
        out[wt] = buf
    monkeypatch.delenv("FRUITS_HIP_DEBUG")
    a, b = out["0"], out["1"]
    assert not torch.isnan(a).any(), dim_note
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), dim_note
    return nat.to_host(b[:, :4])


@pytest.mark.parametrize("N,T", [
    (2048, 1024),   # the headline: one group, cache-sized window (sc1 instance)
    (3072, 1024),   # three groups, the batch streams through HBM (nt sc1 instance)
    (1536, 1024),   # one group, cache-sized window
    (512, 1024),    # small batch: plain stores either way
    (2048, 1000),   # ragged T: no static program
    (512, 256),
    (512, 4096),
])
def test_aot_static_bit_identical(fr, monkeypatch, N, T):
    from oracle import ref_numpy as orc
    words = fr.words.of_weight(2, dim=3)
    X = gen_input({"seed": N + T, "dist": "normal", "shape": [N, 3, T]})
    head = _both_ways(fr, monkeypatch, words, X, f"N={N} T={T}")
    ref = orc.iss_transform(X[:4], [str(w) for w in words], "EXTENDED")
    scale = np.abs(ref).max(axis=2, keepdims=True)
    assert np.max(np.abs(head - ref) / scale) < 1e-9


def test_jit_static_bit_identical(fr, monkeypatch, tmp_path):
    """A plan outside the standard word sets runs a static program compiled at run time."""
    monkeypatch.setenv("FRUITS_HIP_JIT_CACHE", str(tmp_path / "jit"))
    monkeypatch.setenv("FRUITS_HIP_JIT", "1")
    strs = ["[1][2]", "[12][1]", "[2]", "[1][1][2]", "[3][1]", "[33]", "[2][3][1]"]
    words = [fr.words.SimpleWord(s) for s in strs]
    for N in (1601, 2048):
        X = gen_input({"seed": N, "dist": "normal", "shape": [N, 3, 1024]})
        _both_ways(fr, monkeypatch, words, X, f"jit N={N}")


def test_tiled_48_words_bit_identical(fr, monkeypatch, tmp_path):
    """The metric's 48-word reading: of_weight(2,3) tiled to 48 words, SINGLE mode."""
    monkeypatch.setenv("FRUITS_HIP_JIT_CACHE", str(tmp_path / "jit"))
    w15 = fr.words.of_weight(2, dim=3)
    words = [w15[i % 15] for i in range(48)]
    X = gen_input({"seed": 48, "dist": "normal", "shape": [1024, 3, 1024]})
    _both_ways(fr, monkeypatch, words, X, "48 words", iss=fr.ISS(words))


@pytest.mark.parametrize("N,T", [(512, 1024), (256, 1000)])
def test_lean_walk_bit_identical(fr, monkeypatch, N, T):
    """of_weight(4,2) (K = 115): no static program, the lean materialising walk."""
    words = fr.words.of_weight(4, dim=2)
    X = gen_input({"seed": 7 + N, "dist": "normal", "shape": [N, 2, T]})
    _both_ways(fr, monkeypatch, words, X, f"lean N={N} T={T}")
