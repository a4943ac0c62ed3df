"""The stream gate (helper, no test): makes a defect in the stream contract of include/mtd_abi.h deterministic.

Every entry point "enqueues work on an explicit HIP stream".  On the NULL stream, where the rest of the suite runs, every call is ordered
with everything else on the device, so a launch on the wrong stream, a read-back that waits for the wrong stream or a lazily built table
whose first use is not ordered with the caller's stream all go unseen.  The gate runs a call sequence on a non-blocking stream S of its
own (torch.cuda.Stream()) in a way in which such a defect changes the result:

  1. every device input sits in a buffer that holds snapshot A: a different but legal input (positions inside the box, list rows with
     valid indices and counts, finite forces), so that work which runs too early reads valid memory and gives A's answer;
  2. snapshot B, the input the calls are meant for, is staged in a second device tensor;
  3. on S: a delay kernel, an event, the device-to-device copies B -> buffers, then the library calls with stream = S;
  4. directly after the last call returned the event behind the delay must still be pending: the host ran ahead of the device, every
     call was queued while the buffers still held A.  If it is not, the case proved nothing and FAILS (no skip, no retry);
  5. the outputs are read on S and must be, bit for bit, what the same calls return for B on the NULL stream after a full synchronise;
     A's answer on the NULL stream must differ from B's in every compared output, or staleness could pass.

Calls that are documented to synchronise (mtd_metad_get_state, mtd_nlist_build, ...) are the opposite case: the runner reports them
with synced(), the event must then be COMPLETE (the call waited for S, so also for the delay), and what they returned must be B's.

A runner is a function run(..., gate=None) that owns one call sequence and talks to the gate in four places:

    gate = gate or stream_gate.Plain()
    d_x = gate.inp(x)                # every device INPUT (numpy array): uploaded by the gate, which owns the buffer
    stream = gate.arm()              # after every upload and allocation, before the first library call: the stream to pass
    ...library calls with `stream`...   gate.synced() right after a call that is documented to synchronise,
                                        gate.queued() after the last enqueue-only call in front of such a call
    return gate.done(read)           # read(): downloads the outputs (.cpu()) and returns a flat dict / tuple of numpy values

Plain is the NULL stream with torch.cuda.synchronize() before the read, what the runners did before they had a gate; it also records
the arrays and times the host side of the calls.  The delay of a case is ten times that host time (the factor covers the jitter of
the enqueue time on a shared machine), not less than 20 ms and not more than 500 ms.

The delay kernel is torch.cuda._sleep, calibrated once per process with two events; without that private function, a chain of
element-wise operations on a large tensor, timed the same way.
"""
import gc
import time

import numpy as np

MIN_MS, MAX_MS, FACTOR = 20.0, 500.0, 10.0
PROBE_MS = 5.0                                                           # the delay side_by_side_streams() asks two streams to overlap


# ---- the pure parts (tests/test_stream_gate.py checks them without a GPU) -----------------------------------------------------------

def delay_ms(host_ms):
    """FACTOR times the host time of the calls, inside [MIN_MS, MAX_MS]"""
    if not np.isfinite(host_ms) or host_ms < 0:
        raise ValueError("host time %r" % (host_ms,))
    return float(min(MAX_MS, max(MIN_MS, FACTOR * host_ms)))


def delay_units(ms, units_per_ms):
    """the argument of the delay kernel for `ms` milliseconds at the calibrated rate: at least 1"""
    if not units_per_ms > 0:
        raise ValueError("calibrated rate %r" % (units_per_ms,))
    return max(1, int(np.ceil(ms * units_per_ms)))


def pad_to(a, n):
    """a 1-d array continued with zeros to n entries (0 is a valid particle index, count and offset); longer arrays are refused"""
    a = np.ascontiguousarray(a)
    if a.ndim != 1 or len(a) > n:
        raise ValueError("cannot pad shape %s to %d" % (a.shape, n))
    out = np.zeros(n, dtype=a.dtype)
    out[:len(a)] = a
    return out


def common_shape(a, b):
    """(a', b'): snapshots A and B of one input in buffers of one size; 1-d arrays (the nlist array of two different lists) are padded"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype:
        raise ValueError("snapshots of one input differ in dtype: %s, %s" % (a.dtype, b.dtype))
    if a.shape == b.shape:
        return a, b
    if a.ndim != 1 or b.ndim != 1:
        raise ValueError("snapshots of one input differ in shape: %s, %s" % (a.shape, b.shape))
    n = max(len(a), len(b))
    return pad_to(a, n), pad_to(b, n)


def flat(result):
    """key -> bytes of every entry of a runner's result (dict, tuple or list of arrays, scalars and None; None is left out)"""
    items = result.items() if isinstance(result, dict) else enumerate(result)
    return {key: np.ascontiguousarray(x).tobytes() for key, x in items if x is not None}


def differing_keys(x, y, keys=None):
    """the keys (all of x, or `keys`) at which two results differ in any bit"""
    fx, fy = flat(x), flat(y)
    return [k for k in (fx if keys is None else keys) if fx[k] != fy[k]]


def assert_same_bits(got, want, what, keys=None):
    bad = differing_keys(want, got, keys)
    assert not bad, "%s: %s differ from the NULL-stream result" % (what, bad)


def assert_all_differ(a, b, what, keys=None):
    fa = flat(a)
    same = [k for k in (fa if keys is None else keys) if k not in differing_keys(a, b, keys)]
    assert not same, "%s: snapshots A and B give the same %s: a stale input could pass" % (what, same)


# ---- the delay ----------------------------------------------------------------------------------------------------------------------

_rate = None
_spin = None


def _delay(units):
    import torch
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
    else:
        for _ in range(int(units)):
            _spin.mul_(1.0)


def rate():
    """delay units per millisecond on the current device (cycles of torch.cuda._sleep, or operations of the fallback chain): measured
    once per process between two events on a stream of its own, printed"""
    global _rate, _spin
    if _rate is None:
        import torch
        have = hasattr(torch.cuda, "_sleep")
        if not have:
            _spin = torch.ones(1 << 24, dtype=torch.float32, device="cuda")
        units = 20_000_000 if have else 200
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            _delay(max(1, units // 100))                                 # the first launch loads the kernel
            e0.record(s)
            _delay(units)
            e1.record(s)
        s.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0
        _rate = units / ms
        print("\nstream gate: %s, %.4g units per ms (%d units took %.2f ms)" % ("torch.cuda._sleep" if have else "element-wise chain", _rate, units, ms))
    return _rate


# ---- the gates ----------------------------------------------------------------------------------------------------------------------

class Plain:
    """the NULL stream, a full synchronise before the read; keeps the uploaded arrays and the host time of the calls"""

    def __init__(self):
        self.arrays = []
        self.host_ms = None
        self._t0 = None

    def inp(self, a):
        import torch
        a = np.ascontiguousarray(a)
        self.arrays.append(a.copy())
        return torch.from_numpy(a).cuda()

    def arm(self):
        self._t0 = time.perf_counter()
        return None

    def synced(self):
        pass

    def queued(self):
        pass

    def done(self, read):
        import torch
        self.host_ms = 1e3 * (time.perf_counter() - self._t0)
        torch.cuda.synchronize()
        return read()


class Deferred:
    """the read of a gated run that has not happened yet (two streams: both sequences are queued before either is read)"""

    def __init__(self, gate, read):
        self.gate, self.read = gate, read

    def finish(self):
        return self.gate._read(self.read)


class Gated:
    """the gate itself.  a, b: the arrays two Plain runs of the same runner recorded for snapshots A and B (gate.arrays); ms: the delay.
    misuse = "null_stream": arm() hands out the NULL stream although B arrives on S (negative control: the caller's mistake).
    defer: done() returns a Deferred instead of reading.  before_arm(), after_queued(): called at the head of arm() and when the
    last call has returned (check_pair orders two runners with them); stream: the torch stream to use instead of a new one."""

    def __init__(self, a, b, ms, misuse=None, defer=False, before_arm=None, after_queued=None, stream=None):
        import torch
        assert len(a) == len(b), "the two snapshots upload a different number of inputs"
        self.pairs = [common_shape(x, y) for x, y in zip(a, b)]
        self.expect_b = b
        self.ms, self.misuse, self.defer = ms, misuse, defer
        self.before_arm, self.after_queued = before_arm, after_queued
        self.S = torch.cuda.Stream() if stream is None else stream
        self.ev = torch.cuda.Event()
        self.bufs, self.staged = [], []
        self.t_marks = []
        self.marks = []                                                  # event still pending at each queued(): the calls before it were only queued
        self.sync_complete = []                                          # event complete after each synchronising call
        self.host_ms = None

    def inp(self, a):
        import torch
        i = len(self.bufs)
        a = np.ascontiguousarray(a)
        assert a.tobytes() == self.expect_b[i].tobytes(), "input %d of the gated run is not snapshot B's" % i
        snap_a, snap_b = self.pairs[i]
        self.bufs.append(torch.from_numpy(snap_a).cuda())
        self.staged.append(torch.from_numpy(snap_b).cuda())
        return self.bufs[-1]

    def arm(self):
        import torch
        assert len(self.bufs) == len(self.pairs), "the gated run uploaded fewer inputs than the plain one"
        if self.before_arm is not None:
            self.before_arm()
        self.t_arm0 = time.perf_counter()
        self._gc = gc.isenabled()
        gc.disable()                                                     # a collection of a large heap can outlast the delay
        units = delay_units(self.ms, rate())
        self.S.synchronize()                                             # the runner's fills ran on S (run_gated); uploads are blocking copies
        with torch.cuda.stream(self.S):
            _delay(units)
            self.ev.record(self.S)
            for buf, staged in zip(self.bufs, self.staged):
                buf.copy_(staged, non_blocking=True)
        self._t0 = time.perf_counter()
        return None if self.misuse == "null_stream" else self.S.cuda_stream

    def synced(self):
        self.sync_complete.append(bool(self.ev.query()))

    def queued(self):
        self.marks.append(not self.ev.query())
        self.t_marks.append(time.perf_counter())

    @property
    def pending(self):
        return bool(self.marks) and all(self.marks)

    def done(self, read):
        if not self.sync_complete:
            self.queued()
        self.host_ms = 1e3 * (time.perf_counter() - self._t0)
        if self._gc:
            gc.enable()
        if self.after_queued is not None:
            self.after_queued()
        return Deferred(self, read) if self.defer else self._read(read)

    def _read(self, read):
        import torch
        with torch.cuda.stream(self.S):                                  # .cpu() inside read() copies on S and waits for S alone
            out = read()
        self.S.synchronize()
        return out

    def line(self, name, sized_from_ms):
        return "stream gate: %-44s delay %6.1f ms (host time %7.3f ms, gated %7.3f ms)  event pending: %s%s" % (
            name, self.ms, sized_from_ms, self.host_ms, "yes" if self.pending else ("NO" if self.marks else "-"),
            "" if not self.sync_complete else "  complete after sync calls: %s" % ("yes" if all(self.sync_complete) else "NO"))


def run_gated(run, gate, kw):
    """run(gate=gate, **kw) with the gate's stream current, so that the runner's own torch work (fills of its output arrays, .cpu()) is
    on S too"""
    import torch
    with torch.cuda.stream(gate.S):
        return run(gate=gate, **kw)


def expected(run, a_kw, b_kw, what, keys=None):
    """(B's result, A's result, B's arrays, A's arrays, host ms of B's run): the NULL-stream runs of a case; B first, it is the warm-up
    that builds the lazy tables and the run whose host time sizes the delay"""
    pb, pa = Plain(), Plain()
    want = run(gate=pb, **b_kw)
    stale = run(gate=pa, **a_kw)
    assert_all_differ(stale, want, what, keys)
    return want, stale, pb.arrays, pa.arrays, pb.host_ms


def check(name, run, a_kw, b_kw, keys=None, synchronising=False, close=None):
    """one case through the gate.  The event behind the delay must be pending at every queued() of the runner (done() is one unless a
    synchronising call came before it) and complete at every synced(); synchronising: the sequence must hold such a call.
    close(got, want): replaces the bitwise comparison for the paths that add with floating-point atomics.  Returns (got, want, gate)."""
    want, stale, arr_b, arr_a, host_ms = expected(run, a_kw, b_kw, name, keys)
    gate = Gated(arr_a, arr_b, delay_ms(host_ms))
    got = run_gated(run, gate, b_kw)
    print(gate.line(name, host_ms))
    assert bool(gate.sync_complete) == bool(synchronising), "%s: synchronising calls reported: %d" % (name, len(gate.sync_complete))
    assert all(gate.sync_complete), "%s: a call documented to synchronise returned before the stream had passed the delay" % name
    assert gate.marks or gate.sync_complete, "%s: the runner never reached the gate" % name
    assert not gate.marks or gate.pending, ("%s: the delay of %.1f ms was over before the calls were queued (%.3f ms on the host): the case "
                                            "proved nothing" % (name, gate.ms, gate.host_ms))
    if close is None:
        assert_same_bits(got, want, name, keys)
    else:
        close(got, want)
    return got, want, gate


def side_by_side_streams(tries=32):
    """two torch streams on which this process can queue work while the other one is busy.  A process has few hardware queues
    (GPU_MAX_HW_QUEUES) and the runtime spreads its streams over them: for two streams that share one, the first host call on the
    second (observed: 60 ms inside arm(), the length of the first stream's delay) waits until the first stream has drained, and such a
    pair can never hold two sequences behind two delays at once.  That is a property of the pair of streams, not of the library under
    test, so it is asked of the streams alone, with the delay kernel and a copy, before any library call: torch hands out its pool of
    streams in turn, and the first partner that does not wait for the first stream's delay is taken."""
    import torch
    s1 = torch.cuda.Stream()
    units = delay_units(PROBE_MS, rate())
    a = torch.zeros(16, device="cuda")
    b = torch.ones(16, device="cuda")
    for _ in range(tries):
        s2 = torch.cuda.Stream()
        if s2.cuda_stream == s1.cuda_stream:
            continue
        ev = torch.cuda.Event()
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            _delay(units)
            ev.record(s1)
        with torch.cuda.stream(s2):                                      # what Gated.arm() does on the second stream
            s2.synchronize()
            _delay(1)
            a.copy_(b, non_blocking=True)
        s2.synchronize()
        free = not ev.query()
        torch.cuda.synchronize()
        if free:
            return s1, s2
    raise AssertionError("the two-stream cases cannot be set up in this process: of %d torch streams none runs beside the first (one hardware "
                         "queue, GPU_MAX_HW_QUEUES=1?); nothing was asked of the library" % tries)


def check_pair(name, run1, a1, b1, run2, a2, b2, keys1=None, keys2=None):
    """two independent problems on two streams at once: both sequences are queued, each behind a delay of its own length, before either
    is read; each result must be its solo NULL-stream result bit for bit.  The first delay is longer by the host time of the first
    sequence, so that the two streams pass their delays at about the same time and their kernels run side by side.
    The two streams come from side_by_side_streams().
    Creating a handle (mtd_metad_create, mtd_mesh_create) synchronises the device, so both runners must have made theirs before either
    delay is queued: the second runner works in a thread of its own up to its arm(), waits there until the first sequence is queued
    whole, and queues its own then.  The library is never called from two threads at once."""
    import threading
    want1, _, arr_b1, arr_a1, h1 = expected(run1, a1, b1, name + " [1]", keys1)
    want2, _, arr_b2, arr_a2, h2 = expected(run2, a2, b2, name + " [2]", keys2)
    ms = delay_ms(h1 + h2)
    s1, s2 = side_by_side_streams()
    ready2, queued1 = threading.Event(), threading.Event()
    limit = 60.0                                                         # never reached in a sound run: a runner that raised never signals

    def wait(ev, what):
        if not ev.wait(limit):
            raise RuntimeError("%s: %s" % (name, what))

    def second_at_arm():
        ready2.set()
        wait(queued1, "the first sequence was never queued")

    g1 = Gated(arr_a1, arr_b1, ms + h1, defer=True, after_queued=queued1.set, stream=s1)
    g2 = Gated(arr_a2, arr_b2, ms, defer=True, before_arm=second_at_arm, stream=s2)
    box = {}

    def second():
        try:
            box["r2"] = run_gated(run2, g2, b2)
        except BaseException as e:                                       # handed to the main thread below
            box["error"] = e
            ready2.set()

    t = threading.Thread(target=second)
    t.start()
    try:
        wait(ready2, "the second runner never reached its gate")        # its uploads and handles are done; it waits at arm()
        r1 = run_gated(run1, g1, b1)
    finally:
        queued1.set()
        t.join()
    if "error" in box:
        raise box["error"]
    p1, p2 = not g1.ev.query(), not g2.ev.query()
    t_query = time.perf_counter()
    both_pending = "r2" in box and p1 and p2
    r2 = box["r2"]
    got1, got2 = r1.finish(), r2.finish()
    print(g1.line(name + " [1]", h1))
    print(g2.line(name + " [2]", h2))
    ms_since = lambda t: 1e3 * (t - g1.t_arm0)
    when = "ms after the first arm(): delay 1 queued %.3f, sequence 1 queued %.3f, second arm() %.3f, delay 2 queued %.3f, sequence 2 queued %.3f, " \
           "both events asked %.3f (pending: %s, %s); streams %#x, %#x" % (ms_since(g1._t0), ms_since(g1.t_marks[-1]), ms_since(g2.t_arm0), ms_since(g2._t0),
                                                                          ms_since(g2.t_marks[-1]), ms_since(t_query), p1, p2, g1.S.cuda_stream, g2.S.cuda_stream)
    assert g1.pending and g2.pending and both_pending, ("%s: a delay was over before both sequences were queued: the case proved nothing (%s)"
                                                        % (name, when))
    assert_same_bits(got1, want1, name + " [1]", keys1)
    assert_same_bits(got2, want2, name + " [2]", keys2)
    return got1, got2
