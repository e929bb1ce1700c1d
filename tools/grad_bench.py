"""`python tools/grad_bench.py [reps] [launches] [--semiring=reals|arctic|bayesian]
[--weighting=indices[,total]|l1[,total]] [--lengths] [--coswiss] [--features] [--band-features]` from the root of the tree: what the backward pass of the
differentiable ISS costs (fruits_amd.nn).  `of_weight(2, 3)` EXTENDED on a (2048, 3, 1024) batch that lives on the device - standard
normal, uniform in [0.25, 1] for Bayesian -: the forward pass alone (under `torch.no_grad()`) and
forward plus backward (`layer(X).backward(G)` with a dense upstream gradient), `launches`
(default 10) calls back to back between one pair of HIP events so that the host side of a call
hides behind the work in front of it, interleaved over `reps` rounds (default 15) after one
warm-up round; the medians per call, the smallest and largest round of forward plus backward and
the ratio of the medians as one JSON line.  With a max semiring, or with `--weighting` (the
weighted Reals sums of `nn.WeightedISSLayer`, `Indices()` with the words' default alphas, total or
not), the unweighted Reals pair (`nn.ISSLayer`) runs interleaved in the same rounds, for
comparison.  `--weighting=l1[,total]` measures the path-length weighting whose gradient flows
through the lookup too (`nn.PathLengthISSLayer`, `L1()`); its yardstick, interleaved
in the same rounds, is the `Indices` pair of the same body (the keys `indices_...`).

`--features[=dense|picked]` measures a training step on FEATURES instead: the
last value and the maximum of every iterated sum, forward plus backward with an `(N, 2 K)`
upstream gradient.  `picked` is `nn.FeatureLayer` with `[END([-1]), MAX([-1])]`; `dense` is the
same loss through the rows - `nn.ISSLayer`, then `Y[..., -1]` and `Y.amax(-1)` by torch - which
needs nothing of this option's own code and so also runs on a tree without `nn.FeatureLayer`.
Without a value both run interleaved.  The JSON line carries the medians, the smallest and largest
round and `torch.cuda.max_memory_allocated()` of each route, measured over a step of its own.

`--band-features[=dense|banded]` is the same for the band heads: the mean
increment and the last value of every iterated sum.  `banded` is `nn.BandFeatureLayer` with
`[MPI([-1], inc=1), END([-1])]`; `dense` composes the two from torch ops on the rows of
`nn.ISSLayer` - `torch.diff` with the first step prepended, `mean(-1)`, `Y[..., -1]` - and runs on
a tree without `nn.BandFeatureLayer`.

`--lengths` makes the batch ragged: per-series lengths uniform on [T / 2, T]
(seeded), passed as `lengths=` to every layer call - the same padded batch, so the line compares
with the dense call of a run without the option.  `picked` takes them too; the `dense` feature
route has no ragged form and stays dense.

`--coswiss` measures the cosine weighted sums instead (`nn.CosWISSLayer`): the
first CosWISS of the reference's experiments/fruit_reduced.py - `of_weight(1 ... 3, 2)`, the
frequencies 0.05 ... 0.45, exponent 1, total weighting - on a (2048, 2, 1024) batch, forward alone
and forward plus backward as above, and the number of series blocks the device budget
(`FRUITS_AMD_ISS_GIB`) forced on a backward call."""
import json
import statistics
import sys

import numpy as np

import fruits_amd as fr
from fruits_amd import _native as nat
from fruits_amd import nn

args = [a for a in sys.argv[1:] if not a.startswith("--")]
semiring, weighting, features, band = "reals", "", None, False
for a in sys.argv[1:]:
    if a == "--features" or a.startswith("--features="):
        features = a.split("=", 1)[1].lower().split(",") if "=" in a else ["dense", "picked"]
    if a == "--band-features" or a.startswith("--band-features="):
        features, band = a.split("=", 1)[1].lower().split(",") if "=" in a else ["dense", "banded"], True
    if a.startswith("--semiring="):
        semiring = a.split("=", 1)[1].lower()
    if a.startswith("--weighting="):
        weighting = a.split("=", 1)[1].lower()
if semiring not in ("reals", "arctic", "bayesian"):
    sys.exit("--semiring: reals, arctic or bayesian")
if weighting not in ("", "indices", "indices,total", "l1", "l1,total") or (weighting and semiring != "reals"):
    sys.exit("--weighting: indices, indices,total, l1 or l1,total, with the Reals semiring")
if weighting.startswith("l1") and "--lengths" in sys.argv[1:]:
    sys.exit("--weighting=l1: the path-length weighting takes no lengths")
if features is not None and (semiring != "reals" or weighting
                             or set(features) - {"dense", "banded" if band else "picked"}):
    sys.exit("--features: dense, picked or both, --band-features: dense, banded or both, with the unweighted "
             "Reals semiring")
if band and "--lengths" in sys.argv[1:]:
    sys.exit("--band-features: the dense route has no ragged form; on its own")
coswiss = "--coswiss" in sys.argv[1:]
if coswiss and (semiring != "reals" or weighting or features is not None or "--lengths" in sys.argv[1:]):
    sys.exit("--coswiss: on its own")
reps = int(args[0]) if len(args) > 0 else 15
launches = int(args[1]) if len(args) > 1 else 10
t = nat.torch()
nat.require_device()
N, D, T = 2048, 3, 1024
words = fr.words.of_weight(2, dim=3)
K = fr.ISS(words, mode=fr.ISSMode.EXTENDED).n_iterated_sums()
ragged = "--lengths" in sys.argv[1:]
lengths = np.random.default_rng(0).integers(T // 2, T + 1, N) if ragged else None
kw = {"lengths": lengths} if ragged else {}


def timed(fn):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def feature_routes():
    """{route: one training step on the 2 K features of a batch}"""
    X = t.randn((N, D, T), dtype=t.float64, device="cuda").requires_grad_(True)
    g = t.randn((N, 2 * K), dtype=t.float64, device="cuda")
    rows = nn.ISSLayer(words, fr.ISSMode.EXTENDED)

    def dense():
        X.grad = None
        Y = rows(X)                                                       # (N, K, T)
        t.stack((Y[..., -1], Y.amax(-1)), dim=-1).reshape(N, 2 * K).backward(g)

    routes = {"dense": dense}
    if "picked" in features:
        layer = nn.FeatureLayer(words, fr.ISSMode.EXTENDED, [fr.sieving.END([-1]), fr.sieving.MAX([-1])])

        def picked():
            X.grad = None
            layer(X, **kw).backward(g)

        routes["picked"] = picked
    if band:
        def dense_band():
            X.grad = None
            Y = rows(X)                                                       # (N, K, T)
            D1 = t.diff(Y, dim=-1, prepend=Y[..., :1])                        # (the first increment is 0)
            t.stack((D1.mean(-1), Y[..., -1]), dim=-1).reshape(N, 2 * K).backward(g)

        routes["dense"] = dense_band
        if "banded" in features:
            layer = nn.BandFeatureLayer(words, fr.ISSMode.EXTENDED,
                                        [fr.sieving.MPI([-1], inc=1), fr.sieving.END([-1])])

            def banded():
                X.grad = None
                layer(X).backward(g)

            routes["banded"] = banded
    return {k: routes[k] for k in features}


if features is not None:
    routes = feature_routes()
    times, peak = {k: [] for k in routes}, {}
    for r in range(reps + 1):
        for k, fn in routes.items():
            ms = timed(fn)
            if r:                      # (round 0 uploads the tables and warms everything up)
                times[k].append(ms)
    for k, fn in routes.items():
        t.cuda.synchronize()
        t.cuda.reset_peak_memory_stats()
        base = t.cuda.memory_allocated()
        fn()
        t.cuda.synchronize()
        peak[k] = [t.cuda.max_memory_allocated() - base, t.cuda.max_memory_allocated()]
    out = {"shape": [N, D, T], "words": "of_weight(2, 3) EXTENDED", "rows": K, "reps": reps,
           "launches": launches, "features": "MPI([-1], inc=1), END([-1])" if band else "END([-1]), MAX([-1])"}
    if ragged:
        out["lengths"] = [T // 2, T, round(float(lengths.mean()), 1)]
    for k in routes:
        out.update({k + "_step_ms": round(statistics.median(times[k]), 4),
                    k + "_step_minmax_ms": [round(min(times[k]), 4), round(max(times[k]), 4)],
                    k + "_peak_bytes_above_start": peak[k][0], k + "_max_memory_allocated": peak[k][1]})
    if len(routes) == 2:
        new = "banded" if band else "picked"
        out[new + "_over_dense"] = round(out[new + "_step_ms"] / out["dense_step_ms"], 3)
    print(json.dumps(out))
    sys.exit(0)

if coswiss:
    D = 2
    words = fr.words.of_weight(1, 2) + fr.words.of_weight(2, 2) + fr.words.of_weight(3, 2)
    freqs = [i / 20 for i in range(1, 11, 2)]
    layer = nn.CosWISSLayer(words, freqs, exponent=1, total_weighting=True)
    K = layer.op.n_iterated_sums()
    X = t.randn((N, D, T), dtype=t.float64, device="cuda").requires_grad_(True)
    G = t.randn((N, K, T), dtype=t.float64, device="cuda")

    def forward():
        with t.no_grad():
            layer(X)

    def both():
        X.grad = None
        layer(X).backward(G)

    times = {0: [], 1: []}
    for r in range(reps + 1):
        for i, fn in enumerate((forward, both)):
            ms = timed(fn)
            if r:                      # (round 0 uploads the tables and warms everything up)
                times[i].append(ms)
    plan = layer.op._plan(0, len(words))
    block = nn._cos_series_block(plan, N, T)
    f, b = statistics.median(times[0]), statistics.median(times[1])
    print(json.dumps({"shape": [N, D, T], "words": "of_weight(1 ... 3, 2)", "freqs": freqs, "exponent": 1,
                      "total_weighting": True, "rows": K, "reps": reps, "launches": launches,
                      "scratch_rows": list(nat.coswiss_grad_rows(plan)), "series_blocks": -(-N // block),
                      "forward_ms": round(f, 4), "forward_backward_ms": round(b, 4),
                      "forward_backward_minmax_ms": [round(min(times[1]), 4), round(max(times[1]), 4)],
                      "ratio": round(b / f, 3)}))
    sys.exit(0)

G = t.randn((N, K, T), dtype=t.float64, device="cuda")


def pair(layer, X):
    def forward():
        with t.no_grad():
            layer(X, **kw)

    def both():
        X.grad = None
        layer(X, **kw).backward(G)

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
    indices = pair(nn.WeightedISSLayer(words, fr.ISSMode.EXTENDED, weighting=w),
                   X.detach().clone().requires_grad_(True))
    fns = {"": indices, "reals_": fns[""]}
    if weighting.startswith("l1"):
        w = fr.iss.weighting.L1(total=weighting.endswith(",total"))
        fns = {"": pair(nn.PathLengthISSLayer(words, fr.ISSMode.EXTENDED, weighting=w),
                        X.detach().clone().requires_grad_(True)),
               "indices_": indices}


times = {(k, i): [] for k in fns for i in (0, 1)}
for r in range(reps + 1):
    for k, fs in fns.items():
        for i in (0, 1):
            ms = timed(fs[i])
            if r:                      # (round 0 uploads the tables and warms everything up)
                times[k, i].append(ms)
out = {"shape": [N, D, T], "words": "of_weight(2, 3) EXTENDED", "rows": K, "reps": reps,
       "launches": launches, "semiring": semiring, "weighting": weighting or None}
if ragged:
    out["lengths"] = [T // 2, T, round(float(lengths.mean()), 1)]      # [low, high, mean]
for k in fns:
    f, b = statistics.median(times[k, 0]), statistics.median(times[k, 1])
    out.update({k + "forward_ms": round(f, 4), k + "forward_backward_ms": round(b, 4),
                k + "forward_backward_minmax_ms": [round(min(times[k, 1]), 4), round(max(times[k, 1]), 4)],
                k + "ratio": round(b / f, 3)})
print(json.dumps(out))
