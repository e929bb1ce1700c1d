"""`python tools/prep_bench.py [reps] [launches]`: the six preparateur entries (fr_prep_fir,
fr_prep_project, fr_prep_normalize, fr_prep_leadlag, fr_prep_mask, fr_prep_pointwise) at
(2048, 3, 1024) and (8192, 6, 4096) - RPE on the first two dimensions -
HIP-event timed, next to a `torch.Tensor.copy_` that reads + writes the same number of bytes in
the same process (the yardstick of docs/history.md 4.1c).  Every candidate runs the ENTRY on
device tables and an output allocated beforehand, `launches` (default 10) back to back between
one event pair, so the host side of a call hides behind the launch in front of it; the candidates
of a shape are interleaved over `reps` rounds (default 15) and the median per launch is printed
as one markdown table row: entry, shape, us, MB read + written, us of the copy, ratio.  MB is the
compulsory traffic: every output element written, every input element read once - of a masked
input only the kept elements (the row names the kept share), of a table its own bytes."""
import statistics
import sys

import numpy as np

import fruits_amd  # noqa: F401
from fruits_amd import _native as nat
from fruits_amd import preparation as P
from fruits_amd.cache import CacheType, SharedSeedCache

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
launches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
t = nat.torch()
nat.require_device()


def fitted(p, shape, seed=1):
    np.random.seed(seed)
    p.fit(np.broadcast_to(0.0, shape))
    return p


def derived(p, Xd):
    """The device tables the warm-up transform of ``p`` left behind (_derived_tables)."""
    return p._programs[("derived", str(Xd.device))][1]


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
    if kind == "LAG":
        return lambda: nat.prep_leadlag(Xd, out=out), out
    T = int(Xd.shape[2])
    if kind in ("DOT", "PDD", "DIL"):
        md, = derived(p, Xd)
        return lambda: nat.prep_mask(Xd, md, out=out), out
    if kind == "WIN":
        cs = p._cache.get_device(CacheType.COQUANTILE, f"{p._start}:L2")
        ce = p._cache.get_device(CacheType.COQUANTILE, f"{p._end}:L2")
        return lambda: nat.prep_mask(Xd, None, cs, ce, out=out), out
    if kind == "SPE" and p._step_transform is None:
        wd, = derived(p, Xd)
        return lambda: nat.prep_pointwise(nat.FR_PW_MUL, Xd, wd, out=out), out
    if kind == "SPE":
        path = p._cache.get_device(CacheType.ISS, p._step_transform)
        phase = (path / path[:, -1:] ** p._freq).contiguous()
        return lambda: nat.prep_pointwise(nat.FR_PW_MUL, Xd, phase, flags=nat.FR_PW_FLAG_SIN,
                                          out=out), out
    if kind == "RPE":
        cd, sd = derived(p, Xd)
        return lambda: nat.prep_pointwise(nat.FR_PW_ROTATE, Xd, cd, sd, out=out), out
    if kind == "RDW":
        wd, = p._device_tables(Xd, p._weights)
        return lambda: nat.prep_pointwise(nat.FR_PW_POW, Xd, wd, out=out), out
    if kind == "CTS":
        return lambda: nat.prep_pointwise(nat.FR_PW_SHIFT, Xd, shift=p._steps(T), out=out), out
    q = float(p._quantile)
    return lambda: nat.prep_pointwise(nat.FR_PW_CLIP, Xd, q=q, v=q, out=out), out


def kept_share(p, out, Xd):
    """The share of the input a mask keeps (what fr_prep_mask has to read), else 1."""
    kind = type(p).__name__
    if kind in ("DOT", "PDD", "DIL", "WIN"):
        return float((out != 0).double().mean())       # (a standard-normal input has no zeros)
    return 1.0


def streaming(shape, Xd):
    """(name, preparateur, input) of the fr_prep_mask / fr_prep_pointwise candidates."""
    cache = SharedSeedCache()
    cache.adopt_device_input(Xd)
    win, spe = P.WIN(0.25, 0.75), P.SPE(0.5, step_transform="L1")
    win._cache = spe._cache = cache
    qtc = P.QTC(0.7)
    qtc._quantile = 0.5
    X2 = Xd[:, :2, :].contiguous()
    return [("mask DOT n=2", fitted(P.DOT(2), shape), Xd),
            ("mask PDD 0.8/0.5", fitted(P.PDD(0.8, 0.5), shape), Xd),
            ("mask WIN 0.25-0.75", win, Xd), ("SPE table", P.SPE(0.5), Xd), ("SPE L1 device sin", spe, Xd),
            ("RPE (2 dims)", P.RPE(0.5), X2), ("RDW pow", fitted(P.RDW("uniform"), shape), Xd.abs()),
            ("CTS s=3", P.CTS(3), Xd), ("QTC", qtc, Xd)]


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
    cands = [(name, p, Xd) for name, p in cands] + streaming(shape, Xd)
    jobs = []
    for name, p, Xin in cands:
        fn, out = entry_call(p, Xin)
        share = kept_share(p, out, Xin)
        if share < 1.0:
            name += f" (keeps {share:.2f})"
        moved = int(Xin.numel() * 8 * share) + out.numel() * 8
        if type(p).__name__ in ("SPE", "RPE"):       # the wave (per series with a step transform)
            moved += (Xin.shape[0] if p.__dict__.get("_step_transform") else 2) * Xin.shape[2] * 8
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
