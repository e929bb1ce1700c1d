"""MAX / MIN / XPI against NPI / MPI in the fused walk, and LPI (materialising path): one fitted
slice INC -> ISS(of_weight(2, 3), EXTENDED) per sieve set on (2048, 3, 1024), timed with events
around FruitSlice.transform_device (the input already on the device), median of batches after a
warm-up.  Prints one JSON line per sieve set and the ratio MAX/MIN/XPI : NPI/MPI.

    python tools/bench_sieves.py [--batches 15] [--per-batch 5] [--only NAME]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fruits_amd as fr  # noqa: E402
from fruits_amd import _native as nat  # noqa: E402
from fruits_amd.cache import SharedSeedCache  # noqa: E402
from fruits_amd.sieving import END, LPI, MAX, MIN, MPI, NPI, XPI  # noqa: E402

SETS = {
    "npi_mpi_end": lambda: [NPI(), MPI(), END()],
    "max_min_xpi_end": lambda: [MAX(), MIN(), XPI(), END()],
    "lpi_end": lambda: [LPI(), END()],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--per-batch", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    t = nat.torch()
    nat.require_device()
    X = np.random.default_rng(0).standard_normal((2048, 3, 1024))
    res = {}
    for name, sieves in SETS.items():
        if args.only and name != args.only:
            continue
        fruit = fr.Fruit(name)
        fruit.add(fr.preparation.INC)
        fruit.add(fr.ISS(fr.words.of_weight(2, dim=3), mode=fr.ISSMode.EXTENDED))
        fruit.add(*sieves())
        slc = fruit.get_slice()
        slc.fit_sample_size = 1.0
        np.random.seed(0)
        fruit.fit(X[:256])
        cache = SharedSeedCache(X)
        fused = slc._fused(X.shape[2]) is not None
        per = max(1, args.per_batch // (5 if not fused else 1))
        for _ in range(3):                    # warm-up (module loads, compiled kernels)
            slc.transform_device(X, cache=cache)
        t.cuda.synchronize()
        times = []
        for _ in range(args.batches):
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per):
                slc.transform_device(X, cache=cache)
            b.record()
            t.cuda.synchronize()
            times.append(a.elapsed_time(b) / per)
        res[name] = float(np.median(times))
        print(json.dumps({"set": name, "fused": fused, "ms_median": round(res[name], 4),
                          "ms_min": round(float(np.min(times)), 4),
                          "ms_max": round(float(np.max(times)), 4),
                          "batches": args.batches, "per_batch": per}), flush=True)
    if "npi_mpi_end" in res and "max_min_xpi_end" in res:
        print(json.dumps({"ratio_max_min_xpi_to_npi_mpi":
                          round(res["max_min_xpi_end"] / res["npi_mpi_end"], 3)}))


if __name__ == "__main__":
    main()
