"""Times the fused slice of BASELINE config 3's shape - INC -> ISS(of_weight(4, 2), EXTENDED) on
(2048, 3, 1024) - with one sieve set: warm-up, many launches between events, median of batches.
Run from the root of the tree to be measured (the parent commit's for its NPI figure):
    python tools/bench_implicit.py SET [auto_prepare]      SET: implicit | npi | ppv_only | cpv3"""
import json
import os
import sys

os.environ["FRUITS_AMD_AUTO_PREPARE"] = sys.argv[2] if len(sys.argv) > 2 else "0"
sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import fruits_amd as fr  # noqa: E402
from fruits_amd import _native as nat  # noqa: E402
from fruits_amd.cache import SharedSeedCache  # noqa: E402

S = fr.sieving
SETS = {
    "implicit": lambda: [S.PPV([0.2, 0.5, 0.8]), S.CPV(0.5)],
    "ppv_only": lambda: [S.PPV([0.2, 0.5, 0.8, 0.9])],
    "cpv3": lambda: [S.PPV(0.5), S.CPV([0.2, 0.5, 0.8])],
    "npi": lambda: [S.NPI(q=(0.2, 0.5, 0.8, 1.0)), S.NPI(inc=1)],
}
name = sys.argv[1]
t = nat.torch()
nat.require_device()
X = np.random.default_rng(0).standard_normal((2048, 3, 1024))
fruit = fr.Fruit(name)
fruit.add(fr.preparation.INC)
fruit.add(fr.ISS(fr.words.of_weight(4, dim=2), mode=fr.ISSMode.EXTENDED))
fruit.add(*SETS[name]())
slc = fruit.get_slice()
slc.fit_sample_size = 1.0
np.random.seed(0)
fruit.fit(X[:256])
cache = SharedSeedCache(X)
assert slc._fused(X.shape[2]) is not None
for _ in range(5):
    slc.transform_device(X, cache=cache)
t.cuda.synchronize()
times = []
for _ in range(21):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        slc.transform_device(X, cache=cache)
    b.record()
    t.cuda.synchronize()
    times.append(a.elapsed_time(b) / 10)
pipe = slc._fused(X.shape[2])
print(json.dumps({"tree": os.path.basename(os.getcwd()), "set": name, "auto_prepare": os.environ["FRUITS_AMD_AUTO_PREPARE"],
                  "ms_median": round(float(np.median(times)), 4), "ms_min": round(float(np.min(times)), 4),
                  "ms_max": round(float(np.max(times)), 4), "family": pipe.last_launch()["family"],
                  "features": int(pipe.n_features)}), flush=True)
