"""`python tools/prep_bench.py [reps] [launches]`: the four preparateur entries (fr_prep_fir,
fr_prep_project, fr_prep_normalize, fr_prep_leadlag) at (2048, 3, 1024) and (8192, 6, 4096),
HIP-event timed, next to a `torch.Tensor.copy_` that reads + writes the same number of bytes in
the same process (the yardstick of docs/history.md 4.1c).  Every candidate runs the ENTRY on
device tables and an output allocated beforehand, `launches` (default 10) back to back between
one event pair, so the host side of a call hides behind the launch in front of it; the candidates
of a shape are interleaved over `reps` rounds (default 15) and the median per launch is printed
as one markdown table row: entry, shape, us, MB read + written, us of the copy, ratio."""
import statistics
import sys

import numpy as np

import fruits_amd  # noqa: F401
from fruits_amd import _native as nat
from fruits_amd import preparation as P

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
t = nat.torch()
nat.require_device()


def fitted(p, shape, seed=1):
    np.random.seed(seed)
    p.fit(np.broadcast_to(0.0, shape))
    return p


def entry_call(p, Xd):
    """(closure that enqueues the entry once into a fixed output, that output)"""
    kind = type(p).__name__
    out = p._transform_device(Xd)          # (warm-up; the shape of the output)
    if kind == "RIN":
        kd, nd, dd = p._device_tables(Xd, p._kernel, p._ndim_per_kernel, p._dims_per_kernel, ints=2)
        w = p._kernel.shape[1]
        return lambda: nat.prep_fir(Xd, kd, w, nd, dd, p._ndim_per_kernel, p._dims_per_kernel,
                                    False, out=out), out
    if kind == "MAV":
        return lambda: nat.prep_moving_average(Xd, p._w, out=out), out
    if kind == "JLD":
        kd, bd, nd, dd = p._device_tables(Xd, p._kernel, p._bias_weights, p._ndim_per_kernel,
                                          p._dims_per_kernel, ints=2)
        return lambda: nat.prep_project(Xd, kd, bd, nd, dd, p._ndim_per_kernel, p._dims_per_kernel,
                                        out=out), out
    if kind == "FFN":
        W1, b, W2 = p._device_tables(Xd, p._weights1, p._biases, p._weights2)
        return lambda: nat.prep_ffn(Xd, W1, b, W2, p._center, p._relu_out, out=out), out
    if kind == "NRM":
        return lambda: nat.prep_normalize(Xd, p._scale_dim, out=out), out
    return lambda: nat.prep_leadlag(Xd, out=out), out


def timed(fn):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


print("| entry | shape | us | MB moved | copy us | ratio |")
print("|---|---|---|---|---|---|")
for shape in ((2048, 3, 1024), (8192, 6, 4096)):
    N, D, T = shape
    Xd = t.randn(shape, dtype=t.float64, device="cuda")
    half = 2 if D == 3 else D // 2
    cands = [(f"RIN w={w}", fitted(P.RIN(w), shape)) for w in (1, 4, 32)]
    cands += [(f"MAV w={w}", fitted(P.MAV(w), shape)) for w in (5, 102)]
    cands += [(f"JLD {D}->{half}", fitted(P.JLD(half), shape)), ("FFN default", fitted(P.FFN(), shape)),
              ("NRM", P.NRM()), ("LAG", P.LAG())]
    jobs = []
    for name, p in cands:
        fn, out = entry_call(p, Xd)
        moved = Xd.numel() * 8 + out.numel() * 8
        src = t.empty(moved // 16, dtype=t.float64, device="cuda").normal_()
        dst = t.empty_like(src)
        jobs.append((name, fn, (lambda d=dst, s_=src: d.copy_(s_)), moved, out, [], []))
    t.cuda.synchronize()
    for r in range(reps + 1):
        for name, fn, cp, moved, out, tk, tc in jobs:
            a, b = timed(fn), timed(cp)
            if r:                      # (round 0 warms both up)
                tk.append(a)
                tc.append(b)
    for name, fn, cp, moved, out, tk, tc in jobs:
        k, c = statistics.median(tk), statistics.median(tc)
        print(f"| {name} | {N}x{D}x{T} | {k:.1f} | {moved / 1e6:.1f} | {c:.1f} | {k / c:.2f} |", flush=True)
    del jobs, Xd
    t.cuda.empty_cache()
