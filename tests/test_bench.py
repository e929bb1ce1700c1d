"""bench.py's contract: a plain run prints one JSON line with the headline alone, and
--dump-outputs writes what its last timed step computed, the same on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from oracle import ref_numpy as orc


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(tmp_path):
    import bench
    import fruits_amd as fr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["higher_is_better"] is True
    assert res["unit"] == "iterated-sum elements/s" and res["dtype"] == "f64" and res["value"] > 0
    # what moved behind --full stays out of a plain run
    for key in ("cpu_baseline", "extras", "word_sharded_config4"):
        assert key not in res
    assert "batches" not in res["roofline"] and "secondary" not in res["roofline"]

    got = np.load(tmp_path / "iss_knt_sample.npy")
    assert got.dtype == np.float64 and got.shape == (18, bench.DUMP_SERIES, bench.N_STEPS_T)
    assert got.nbytes <= 64 << 20
    # bench.py's own input batch and sample, against the oracle
    X = np.random.default_rng(0).standard_normal((bench.N_SERIES, bench.N_DIMS, bench.N_STEPS_T))
    pick = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(bench.N_SERIES, bench.DUMP_SERIES,
                                                                 replace=False))
    ref = orc.iss_transform(X[pick], [str(w) for w in fr.words.of_weight(2, dim=bench.N_DIMS)], "EXTENDED")
    scale = np.abs(ref).max(axis=2, keepdims=True)
    assert float(np.max(np.abs(got - ref) / scale)) < 1e-12
