"""Runs a device call on a side stream behind an unfinished producer, so that a launch, copy or
table upload that went to another stream - or that ran before or after its place in the stream -
gives a WRONG NUMBER, deterministically, and never touches invalid memory
(tests/test_streams_gpu.py, tests/test_preparation_gpu.py).

Not a conftest: the modules that need it import it by name.  torch is imported when a function
runs, not when the module is.

The protocol of ``behind_producer(call, true_inputs, wrong_inputs)``; ``call(*tensors)`` takes device
tensors and returns a device tensor or a tuple of them, every input pair has one shape and two
different sets of finite random values:

1. ``call(true)`` twice on the default stream, synchronised and downloaded: the expected result
   (and every compilation and table upload the call makes the first time).  Where the comparison
   is to be exact the two runs must agree bit for bit.
2. ``call(wrong)`` on the default stream and under the side stream, synchronising after each: every
   workspace or intermediate block the caching allocator hands out again now holds values of the
   WRONG input - a kernel that ran too early would otherwise read the previous identical call's
   correct intermediates.  The second of them is timed on the host without a synchronisation:
   ``host_ms``, what the warm call takes to return.
3. The input buffers of the real run are allocated and filled with the WRONG values; the device is
   synchronised.
4. Under the side stream (``torch.cuda.Stream()``: non-blocking; one for the session,
   ``side_streams``): a delay of
   ``max(20 ms, 10 host_ms)`` of device time (the factor ten covers interpreter and allocator
   jitter), the copy of the TRUE values into the buffers, an event ``produced``, the call - noting
   whether ``produced.query()`` is still False when it returns - clones of its outputs, and the
   WRONG values into the buffers again (a launch deferred past its place reads those).
5. ``side.synchronize()``; the clones against the expected result: ``assert_array_equal``, except
   the columns the caller names as band sums (``loose``: MPI, CUR, AVG, STD - wave partials that
   meet in arrival order; rtol 1e-12, the carve-out of tests/test_epilogue_gpu.py and
   tests/test_hip_parity.py for exactly those columns).

An enqueue-only call must return while the producer still runs.  If it did not, the run is repeated
with the delay doubled, at most twice more and never beyond ``CAP_MS`` of device time; after that
the check FAILS.  ``synchronising=True`` (the entries that return host arrays) skips that check
alone.

The delay is ``torch.cuda._sleep``, calibrated with events as torch's own tests do
(``cycles_per_ms``); no length is fixed, the calibration and the delay used are in the ``Report``,
the assertion messages and, through ``note``, in the test's ``record_property``.
"""
import dataclasses
import time

import numpy as np

FLOOR_MS = 20.0
MARGIN = 10.0
CAP_MS = 500.0
LOOSE_RTOL = 1e-12      # (band sums: arrival order, tests/test_epilogue_gpu.py, tests/test_hip_parity.py)

_CYCLES_PER_MS = None
REPORTS = []            # every Report of the session, for the summary a module prints at its end


def torch():
    import torch as t
    return t


def cycles_per_ms():
    """Spin cycles of ``torch.cuda._sleep`` per millisecond of device time: the median of five
    event-timed spins of 10^6 cycles (as torch.testing._internal.common_utils.get_cycles_per_ms)."""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        t = torch()
        t.cuda._sleep(1_000_000)        # (the first launch loads the kernel)
        t.cuda.synchronize()
        rates = []
        for _ in range(5):
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            t.cuda._sleep(1_000_000)
            b.record()
            b.synchronize()
            rates.append(1_000_000 / a.elapsed_time(b))
        _CYCLES_PER_MS = float(np.median(rates))
    return _CYCLES_PER_MS


def delay(ms):
    """Queues ``ms`` (at most CAP_MS) of device time on the current stream."""
    assert 0 < ms <= CAP_MS, ms
    torch().cuda._sleep(int(ms * cycles_per_ms()))


_SIDE = []


def side_streams(n=1):
    """The session's ``n`` side streams (``torch.cuda.Stream()``: non-blocking), made once and used by
    every run: with the default stream and ``_native.to_device``'s upload stream at most four streams
    in the process, one per hardware queue of the runtime's default four.

    The runtime maps streams onto its hardware queues, and two streams on one queue run in order:
    an upload on ``to_device``'s private stream then waits behind the delay of a side stream it has
    nothing to do with, and the host with it.  That is the queue map, not the library, so a stream
    is taken only if it was SEEN to leave the others alone: while a delay holds it, an upload
    through ``to_device``, a kernel on the default stream and one on every side stream chosen before
    must finish.  At most eight of torch's pool streams are tried; none free is a failure."""
    from fruits_amd import _native as nat
    t = torch()
    while len(_SIDE) < n:
        for _ in range(8):
            c = t.cuda.Stream()
            t.cuda.synchronize()
            with t.cuda.stream(c):
                delay(FLOOR_MS)
                busy = t.cuda.Event()
                busy.record()
            nat.to_device(np.zeros(8)).add_(1.0)
            t.cuda.default_stream().synchronize()
            for o in _SIDE:
                with t.cuda.stream(o):
                    t.zeros(8, device="cuda").add_(1.0)
                o.synchronize()
            free = not busy.query()
            c.synchronize()
            if free:
                _SIDE.append(c)
                break
        else:
            raise AssertionError("no torch stream leaves the default stream, the upload stream and "
                                 f"the {len(_SIDE)} side stream(s) before it alone: fewer hardware "
                                 "queues than streams")
    return _SIDE[:n]


@dataclasses.dataclass
class Report:
    what: str
    host_ms: float          # wall time in which the warm call returned under the side stream
    delay_ms: float         # the delay of the run that was judged
    attempts: int           # runs behind a producer (1: the first delay was long enough)
    pending: bool           # produced.query() was False when the call returned
    cycles_per_ms: float

    def __str__(self):
        return (f"[{self.what}: host_ms={self.host_ms:.3f} delay_ms={self.delay_ms:.1f} "
                f"attempts={self.attempts} producer pending at return={self.pending} "
                f"cycles/ms={self.cycles_per_ms:.0f}]")


def note(record_property, report):
    for k in ("host_ms", "delay_ms", "attempts", "pending", "cycles_per_ms"):
        record_property(f"{report.what} {k}", getattr(report, k))


def _tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def _device(arrays):
    """Device copies of host arrays, of their own dtype, on the current stream (synchronous)."""
    t = torch()
    return [t.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _download(outs):
    return [o.detach().cpu().numpy().copy() for o in _tuple(outs)]


def compare(got, want, loose=None, what=""):
    """``got`` against ``want``, lists of host arrays: exact, except the columns ``loose`` (a
    boolean mask over the last axis of the FIRST array) to LOOSE_RTOL."""
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape)
        if i == 0 and loose is not None and np.any(loose):
            loose = np.asarray(loose, dtype=bool)
            np.testing.assert_array_equal(g[..., ~loose], w[..., ~loose], err_msg=f"{what} output {i}")
            np.testing.assert_allclose(g[..., loose], w[..., loose], rtol=LOOSE_RTOL, atol=0,
                                       err_msg=f"{what} output {i} (summed columns)")
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{what} output {i}")


def expected(call, true_inputs, loose=None, what=""):
    """Step 1: the default-stream result of ``call`` on the true inputs (a list of host arrays);
    two runs must agree (bit for bit outside ``loose``)."""
    t = torch()
    ins = _device(true_inputs)
    t.cuda.synchronize()
    first = _download(call(*ins))
    t.cuda.synchronize()
    second = _download(call(*ins))
    compare(second, first, loose, f"{what}: two default-stream runs")
    return first


def _poison(call, wrong_d, side):
    """Step 2; returns host_ms."""
    t = torch()
    call(*[w.clone() for w in wrong_d])
    t.cuda.synchronize()
    bufs = [w.clone() for w in wrong_d]
    t.cuda.synchronize()
    with t.cuda.stream(side):
        t0 = time.perf_counter()
        call(*bufs)
        host_ms = (time.perf_counter() - t0) * 1e3
    side.synchronize()
    t.cuda.synchronize()
    return host_ms


def _once(call, true_d, wrong_d, side, delay_ms, after=None):
    """Steps 3 to 5 for one delay: (outputs as host arrays, pending at return, result of
    ``after``).  ``after(bufs)``: called under the side stream behind the call's clones, before the
    buffers are overwritten (section 3 of tests/test_streams_gpu.py: the call that follows)."""
    t = torch()
    bufs = [w.clone() for w in wrong_d]
    t.cuda.synchronize()
    with t.cuda.stream(side):
        delay(delay_ms)
        for b, v in zip(bufs, true_d):
            b.copy_(v)
        produced = t.cuda.Event()
        produced.record()
        outs = _tuple(call(*bufs))
        pending = not produced.query()
        clones = [o.detach().clone() for o in outs]
        kept = [b.clone() for b in bufs]
        extra = after(bufs) if after is not None else None
        for b, w in zip(bufs, wrong_d):
            b.copy_(w)
    side.synchronize()
    got = [c.cpu().numpy() for c in clones]
    # (the call's own inputs: as the producer left them)
    for k, v in zip(kept, true_d):
        np.testing.assert_array_equal(k.cpu().numpy(), v.cpu().numpy(), err_msg="the call changed its input")
    t.cuda.synchronize()
    return got, pending, extra


def _check_inputs(true_inputs, wrong_inputs, what, finite=True):
    assert len(true_inputs) == len(wrong_inputs)
    for a, b in zip(true_inputs, wrong_inputs):
        assert a.shape == b.shape and a.dtype == b.dtype and not np.array_equal(a, b), what
        # (no NaN sentinels: the max-plus semirings drop them and would hide a stale read)
        assert np.isfinite(b).all() and (np.isfinite(a).all() or not finite), what


def behind_producer(call, true_inputs, wrong_inputs, *, what, loose=None, synchronising=False,
                    want=None, after=None, side=None, finite=True):
    """The whole protocol (module docstring).  Returns ``(expected outputs, Report)``, with the
    result of ``after`` as a third element when one is given.  ``want``: the expected outputs, if
    the caller has them from ``expected`` already.  ``finite=False``: the TRUE input may hold NaNs
    and infinities (the data of fr_nan_to_num), the wrong one never."""
    t = torch()
    _check_inputs(true_inputs, wrong_inputs, what, finite)
    if want is None:
        want = expected(call, true_inputs, loose, what)
    true_d, wrong_d = _device(true_inputs), _device(wrong_inputs)
    t.cuda.synchronize()
    side = side_streams(1)[0] if side is None else side
    host_ms = _poison(call, wrong_d, side)
    delay_ms = min(max(FLOOR_MS, MARGIN * host_ms), CAP_MS)
    attempts = 0
    while True:
        attempts += 1
        got, pending, extra = _once(call, true_d, wrong_d, side, delay_ms, after)
        report = Report(what, host_ms, delay_ms, attempts, pending, cycles_per_ms())
        # (the numbers are judged on every attempt: a run whose producer had finished is still a
        # run on the side stream)
        compare(got, want, loose, f"{what} on the side stream {report}")
        if pending or synchronising or attempts == 3 or delay_ms >= CAP_MS:
            break
        delay_ms = min(2.0 * delay_ms, CAP_MS)
    REPORTS.append(report)
    if not synchronising:
        assert pending, (f"{what}: the call returned only after its producer had finished - it "
                         f"waits for the stream, or the delay is too short {report}")
    return (want, report) if after is None else (want, report, extra)


def replaced_in_flight(run, set_old, set_new, true_inputs, wrong_inputs, *, what, loose=None,
                       distinct=True):
    """A device table of a live object replaced from the host while a launch that reads it waits
    behind its producer.  ``set_old()`` / ``set_new()`` put the two tables in place (host calls that
    take no stream), ``run(*tensors)`` enqueues the launch on the current stream.

    Expected, on the default stream: ``run`` under the old table and under the new one
    (``distinct``: they must differ, or the case shows nothing).  Then, with the old table in place
    and the reused memory poisoned as in ``behind_producer``: under the side stream the delay, the
    true inputs, ``run`` - the producer must still be running when it returns - a clone of its
    result, ``set_new()`` from the host while the delay runs, ``run`` again and a clone.  The first
    clone must be the OLD table's result, the second the new one's.  A setter may get there by
    synchronising; nothing here requires the first run still to be queued afterwards."""
    t = torch()
    _check_inputs(true_inputs, wrong_inputs, what)
    true_d, wrong_d = _device(true_inputs), _device(wrong_inputs)
    t.cuda.synchronize()
    set_old()
    want_old = _download(run(*true_d))
    t.cuda.synchronize()
    set_new()
    want_new = _download(run(*true_d))
    t.cuda.synchronize()
    if distinct:
        assert not all(np.array_equal(a, b) for a, b in zip(want_old, want_new)), \
            f"{what}: the two tables give one result"
    set_old()
    compare(_download(run(*true_d)), want_old, loose, f"{what}: the old table again")
    side = side_streams(1)[0]
    host_ms = _poison(run, wrong_d, side)
    delay_ms = min(max(FLOOR_MS, MARGIN * host_ms), CAP_MS)
    attempts = 0
    while True:
        attempts += 1
        set_old()
        bufs = [w.clone() for w in wrong_d]
        t.cuda.synchronize()
        with t.cuda.stream(side):
            delay(delay_ms)
            for b, v in zip(bufs, true_d):
                b.copy_(v)
            produced = t.cuda.Event()
            produced.record()
            first = [o.detach().clone() for o in _tuple(run(*bufs))]
            pending = not produced.query()
            set_new()                       # (from the host, while the delay runs)
            second = [o.detach().clone() for o in _tuple(run(*bufs))]
            for b, w in zip(bufs, wrong_d):
                b.copy_(w)
        side.synchronize()
        got_old, got_new = [c.cpu().numpy() for c in first], [c.cpu().numpy() for c in second]
        t.cuda.synchronize()
        report = Report(what, host_ms, delay_ms, attempts, pending, cycles_per_ms())
        compare(got_old, want_old, loose, f"{what}: the run queued BEFORE the table was replaced {report}")
        compare(got_new, want_new, loose, f"{what}: the run queued AFTER the table was replaced {report}")
        if pending or attempts == 3 or delay_ms >= CAP_MS:
            break
        delay_ms = min(2.0 * delay_ms, CAP_MS)
    REPORTS.append(report)
    assert pending, f"{what}: the run returned only after its producer had finished {report}"
    return report


def two_streams(call, inputs_a, inputs_b, wrong_inputs, *, what, loose=None):
    """One object, two streams: ``call`` on ``inputs_a`` under one side stream and on ``inputs_b``
    under another, each behind its own delayed producer, enqueued alternately without a
    synchronisation in between; each result must be that input's own serial result.  Returns the
    two expected results and a Report (``pending``: both producers were running when the last
    call returned)."""
    t = torch()
    want_a = expected(call, inputs_a, loose, f"{what} (a)")
    want_b = expected(call, inputs_b, loose, f"{what} (b)")
    a_d, b_d, wrong_d = _device(inputs_a), _device(inputs_b), _device(wrong_inputs)
    t.cuda.synchronize()
    s1, s2 = side_streams(2)
    host_ms = max(_poison(call, wrong_d, s1), _poison(call, wrong_d, s2))
    delay_ms = min(max(FLOOR_MS, 2 * MARGIN * host_ms), CAP_MS)      # (two calls behind each delay)
    attempts = 0
    while True:
        attempts += 1
        bufs1, bufs2 = [w.clone() for w in wrong_d], [w.clone() for w in wrong_d]
        t.cuda.synchronize()
        events = []
        for s, bufs, true_d in ((s1, bufs1, a_d), (s2, bufs2, b_d)):
            with t.cuda.stream(s):
                delay(delay_ms)
                for b, v in zip(bufs, true_d):
                    b.copy_(v)
                ev = t.cuda.Event()
                ev.record()
                events.append(ev)
        with t.cuda.stream(s1):
            o1 = _tuple(call(*bufs1))
        with t.cuda.stream(s2):
            o2 = _tuple(call(*bufs2))
        pending = not events[0].query() and not events[1].query()
        clones = []
        for s, outs, bufs in ((s1, o1, bufs1), (s2, o2, bufs2)):
            with t.cuda.stream(s):
                clones.append([o.detach().clone() for o in outs])
                for b, w in zip(bufs, wrong_d):
                    b.copy_(w)
        s1.synchronize()
        s2.synchronize()
        got = [[c.cpu().numpy() for c in cl] for cl in clones]
        t.cuda.synchronize()
        report = Report(what, host_ms, delay_ms, attempts, pending, cycles_per_ms())
        compare(got[0], want_a, loose, f"{what}: first stream {report}")
        compare(got[1], want_b, loose, f"{what}: second stream {report}")
        if pending or attempts == 3 or delay_ms >= CAP_MS:
            break
        delay_ms = min(2.0 * delay_ms, CAP_MS)
    REPORTS.append(report)
    assert pending, f"{what}: a producer had finished before both calls were enqueued {report}"
    return want_a, want_b, report
