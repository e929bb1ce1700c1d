"""`python tools/node_body_golden.py [file]` from the root of the tree: records what every form of
the fused walk's node body computes on the cases of tests/test_node_body_gpu.py, for
`test_node_body_keeps_its_bits` there.  Writes `file` (default
tests/golden/node_body_before_one_copy.npz): per feature case `<name>/thresholds` and
`<name>/features`, per lean case `<name>/digests` (the SHA-256 of every output row's (N, T) plane)
and `<name>/probes` (the tensor at `probe_positions(T)`), `meta` (a JSON string: the cases, their
shapes and the seed of each input) and `summed_run_to_run`.

The file under tests/golden was written ONCE, on an MI355X, by a checkout of the commit BEFORE the
three node bodies of walk_fused.h (fnode, fnode_shaped, fwalk_static) became one: it is what that
commit computed.  Running this on a later commit records that commit, which proves nothing about
it - do so only to pin a deliberate change of the arithmetic.

Every case runs twice.  The two runs must agree bit for bit in the thresholds, in every column the
test compares exactly and in the lean tensors; the largest relative difference they show in the
band-sum columns (wave partials that meet in LDS in arrival order) is `summed_run_to_run`, which
the test prints beside its own.

A case that fails is reported and the others still run; the file is written only when all did."""
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def record(fr, tn, case, out):
    name = case["name"]
    if case["form"] == "lean":
        got = tn.run_lean(fr, case, os.environ.__setitem__)
        again = tn.run_lean(fr, case, os.environ.__setitem__)
        np.testing.assert_array_equal(got, again, err_msg=name)
        out[name + "/digests"] = tn.row_digests(got)
        out[name + "/probes"] = got[:, :, tn.probe_positions(case["T"])]
        print(f"{name}: tensor {got.shape}", flush=True)
        return 0.0
    th, feats, labels = tn.run_features(fr, case, os.environ.__setitem__)
    th2, again, _ = tn.run_features(fr, case, os.environ.__setitem__)
    np.testing.assert_array_equal(th, th2, err_msg=name)
    summed = tn.summed_columns(labels)
    np.testing.assert_array_equal(feats[:, ~summed], again[:, ~summed], err_msg=name)
    assert 2 * int((~summed).sum()) >= len(labels) and summed.any(), (name, int(summed.sum()), len(labels))
    here = tn.largest_relative(feats[:, summed], again[:, summed])
    out[name + "/thresholds"], out[name + "/features"] = th, feats
    print(f"{name}: features {feats.shape}, {int(summed.sum())} summed, {th.size} thresholds, "
          f"two runs differ by {here:.3g}", flush=True)
    return here


def main(path):
    import fruits_amd as fr
    from fruits_amd import _native as nat
    import test_node_body_gpu as tn

    nat.require_device()
    out, moved, cases, failed = {}, 0.0, [], []
    for i, case in enumerate(tn.CASES):
        try:
            moved = max(moved, record(fr, tn, case, out))
        except Exception:
            traceback.print_exc()
            failed.append(case["name"])
            print(f"{case['name']}: FAILED", flush=True)
        cases.append(dict(case, shape=[case["N"], tn.DIMS, case["T"]], seed=[i, case["N"], case["T"]]))
    if failed:
        sys.exit(f"{len(failed)} cases failed, nothing written: {failed}")
    out["meta"] = np.array(json.dumps({"cases": cases}))
    out["summed_run_to_run"] = np.array(moved)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"{path}: {len(cases)} cases, {os.path.getsize(path)} bytes, summed_run_to_run {moved:.3g}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1
         else os.path.join(ROOT, "tests", "golden", "node_body_before_one_copy.npz"))
