"""`python tools/grad_bench.py [reps] [launches]` from the root of the tree: what the backward
pass of the differentiable ISS costs (fruits_amd.nn).  `of_weight(2, 3)` EXTENDED on a
standard normal (2048, 3, 1024) batch that lives on the device: the forward pass alone
(`nn.iss` under `torch.no_grad()`) and forward plus backward (`nn.iss(X).backward(G)` with a
dense upstream gradient), `launches` (default 10) calls back to back between one pair of HIP
events so that the host side of a call hides behind the work in front of it, the two interleaved
over `reps` rounds (default 15) after one warm-up round; the medians per call and their ratio
as one JSON line."""
import json
import statistics
import sys

import fruits_amd as fr
from fruits_amd import _native as nat
from fruits_amd import nn

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
t = nat.torch()
nat.require_device()
N, D, T = 2048, 3, 1024
words = fr.words.of_weight(2, dim=3)
layer = nn.ISSLayer(words, fr.ISSMode.EXTENDED)
X = t.randn((N, D, T), dtype=t.float64, device="cuda").requires_grad_(True)
K = fr.ISS(words, mode=fr.ISSMode.EXTENDED).n_iterated_sums()
G = t.randn((N, K, T), dtype=t.float64, device="cuda")


def forward():
    with t.no_grad():
        layer(X)


def both():
    X.grad = None
    layer(X).backward(G)


def timed(fn):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


tf, tb = [], []
for r in range(reps + 1):
    f, b = timed(forward), timed(both)
    if r:                      # (round 0 uploads the tables and warms both up)
        tf.append(f)
        tb.append(b)
f, b = statistics.median(tf), statistics.median(tb)
print(json.dumps({"shape": [N, D, T], "words": "of_weight(2, 3) EXTENDED", "rows": K, "reps": reps,
                  "launches": launches,
                  "forward_ms": round(f, 4), "forward_backward_ms": round(b, 4),
                  "ratio": round(b / f, 3)}))
