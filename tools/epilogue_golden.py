"""`python tools/epilogue_golden.py [file]` from the root of the tree: records the features every
kernel family with a fused sieve epilogue computes on the cases of tests/test_epilogue_gpu.py, for
`test_epilogue_keeps_its_bits` there.  Writes `file` (default
tests/golden/epilogue_before_one_copy.npz): per case `<name>/thresholds` and `<name>/features`,
`meta` (a JSON string: the cases, their shapes and the seed of each input) and `summed_run_to_run`.

The file under tests/golden was written ONCE, on an MI355X, by a checkout of the commit BEFORE the
two copies of the epilogue (the second copy in walk_device.h, `fop` of walk_fused.h) became one: it is
what that commit computed.  Running this on a later commit records that commit, which proves
nothing about it - do so only to pin a deliberate change of the arithmetic.

Every case runs twice.  The two runs must agree bit for bit in the thresholds and in every column
the test compares exactly; the largest relative difference they show in the band-sum columns of
the cooperative cases (wave partials that meet in LDS in arrival order) is `summed_run_to_run`,
which the test prints beside its own.

The file is about 175 KB, compressed: 40 cases of 6 or 7 series by 96 to 130 features, roughly half of
them real numbers that do not compress.  Two words (five rows, one node with a second scan) and two
CosWISS words by two frequencies are the fewest that reach every path; it stays well under the limit
for a committed file."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(path):
    import fruits_amd as fr
    from fruits_amd import _native as nat
    import test_epilogue_gpu as te

    nat.require_device()
    out, moved, cases = {}, 0.0, []
    for i, case in enumerate(te.CASES):
        name = case["name"]
        th, feats, labels = te.run_case(fr, case, os.environ.__setitem__)
        th2, again, _ = te.run_case(fr, case, os.environ.__setitem__)
        np.testing.assert_array_equal(th, th2, err_msg=name)
        summed = te.summed_columns(labels) if case["cooperative"] else np.zeros(len(labels), dtype=bool)
        np.testing.assert_array_equal(feats[:, ~summed], again[:, ~summed], err_msg=name)
        if case["cooperative"]:
            assert 2 * int((~summed).sum()) >= len(labels), (name, int(summed.sum()), len(labels))
        here = te.largest_relative(feats[:, summed], again[:, summed])
        moved = max(moved, here)
        out[name + "/thresholds"], out[name + "/features"] = th, feats
        X, _ = te.case_input(case)
        cases.append(dict(case, shape=list(X.shape), seed=[i, X.shape[0], case["T"]]))
        print(f"{name}: features {feats.shape}, {int(summed.sum())} summed, {th.size} thresholds, "
              f"two runs differ by {here:.3g}", flush=True)
    out["meta"] = np.array(json.dumps({"cases": cases, "series": te.N_SERIES}))
    out["summed_run_to_run"] = np.array(moved)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"{path}: {len(cases)} cases, {os.path.getsize(path)} bytes, summed_run_to_run {moved:.3g}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1
         else os.path.join(ROOT, "tests", "golden", "epilogue_before_one_copy.npz"))
