"""`python tools/grad_bench.py [reps] [launches] [--semiring=reals|arctic|bayesian]
[--weighting=indices[,total]]` from the root of the tree: what the backward pass of the
differentiable ISS costs (fruits_amd.nn).  `of_weight(2, 3)` EXTENDED on a (2048, 3, 1024) batch that lives on the device - standard
normal, uniform in [0.25, 1] for Bayesian -: the forward pass alone (under `torch.no_grad()`) and
forward plus backward (`layer(X).backward(G)` with a dense upstream gradient), `launches`
(default 10) calls back to back between one pair of HIP events so that the host side of a call
hides behind the work in front of it, interleaved over `reps` rounds (default 15) after one
warm-up round; the medians per call, the smallest and largest round of forward plus backward and
the ratio of the medians as one JSON line.  With a max semiring, or with `--weighting` (the
weighted Reals sums of `nn.WeightedISSLayer`, `Indices()` with the words' default alphas, total or
not), the unweighted Reals pair (`nn.ISSLayer`) runs interleaved in the same rounds, for
comparison."""
import json
import statistics
import sys

import fruits_amd as fr
from fruits_amd import _native as nat
from fruits_amd import nn

args = [a for a in sys.argv[1:] if not a.startswith("--")]
semiring, weighting = "reals", ""
for a in sys.argv[1:]:
    if a.startswith("--semiring="):
        semiring = a.split("=", 1)[1].lower()
    if a.startswith("--weighting="):
        weighting = a.split("=", 1)[1].lower()
if semiring not in ("reals", "arctic", "bayesian"):
    sys.exit("--semiring: reals, arctic or bayesian")
if weighting not in ("", "indices", "indices,total") or (weighting and semiring != "reals"):
    sys.exit("--weighting: indices or indices,total, with the Reals semiring")
reps = int(args[0]) if len(args) > 0 else 15
launches = int(args[1]) if len(args) > 1 else 10
t = nat.torch()
nat.require_device()
N, D, T = 2048, 3, 1024
words = fr.words.of_weight(2, dim=3)
K = fr.ISS(words, mode=fr.ISSMode.EXTENDED).n_iterated_sums()
G = t.randn((N, K, T), dtype=t.float64, device="cuda")


def pair(layer, X):
    def forward():
        with t.no_grad():
            layer(X)

    def both():
        X.grad = None
        layer(X).backward(G)

    return forward, both


X = t.randn((N, D, T), dtype=t.float64, device="cuda").requires_grad_(True)
fns = {"": pair(nn.ISSLayer(words, fr.ISSMode.EXTENDED), X)}
if semiring != "reals":
    sr = fr.semiring.Arctic() if semiring == "arctic" else fr.semiring.Bayesian()
    Xm = X.detach().clone()
    if semiring == "bayesian":
        Xm = 0.25 + 0.75 * t.rand((N, D, T), dtype=t.float64, device="cuda")
    fns = {"": pair(nn.MaxISSLayer(words, fr.ISSMode.EXTENDED, semiring=sr), Xm.requires_grad_(True)),
           "reals_": fns[""]}
if weighting:
    w = fr.iss.weighting.Indices(total=weighting.endswith(",total"))
    fns = {"": pair(nn.WeightedISSLayer(words, fr.ISSMode.EXTENDED, weighting=w),
                    X.detach().clone().requires_grad_(True)),
           "reals_": fns[""]}


def timed(fn):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


times = {(k, i): [] for k in fns for i in (0, 1)}
for r in range(reps + 1):
    for k, fs in fns.items():
        for i in (0, 1):
            ms = timed(fs[i])
            if r:                      # (round 0 uploads the tables and warms everything up)
                times[k, i].append(ms)
out = {"shape": [N, D, T], "words": "of_weight(2, 3) EXTENDED", "rows": K, "reps": reps,
       "launches": launches, "semiring": semiring, "weighting": weighting or None}
for k in fns:
    f, b = statistics.median(times[k, 0]), statistics.median(times[k, 1])
    out.update({k + "forward_ms": round(f, 4), k + "forward_backward_ms": round(b, 4),
                k + "forward_backward_minmax_ms": [round(min(times[k, 1]), 4), round(max(times[k, 1]), 4)],
                k + "ratio": round(b / f, 3)})
print(json.dumps(out))
