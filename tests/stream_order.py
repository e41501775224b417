"""The late-input harness of tests/test_gpu_stream_order.py: proves that a device entry point follows the stream it was given.

The caller's stream S is made late on purpose.  Every device buffer handed to the library starts with a DECOY (a valid
input of the same geometry); the REAL contents arrive on S behind a delay.  On S, in order: delay, real over decoy, the
library call (no host wait), a snapshot of every output, a scribble (decoy back over the inputs, a sentinel over the
outputs).  After one final synchronise the snapshot must equal the expected bytes: work that ran ahead of S saw the decoy
(or was overwritten by the late pre-fill of its output), work that finished behind S's order saw the scribble or missed the
snapshot.  Witness copies on the null stream and on a third stream W, enqueued just before the call, must hold the decoy:
they show that the window was open and that those streams run beside S.  A case whose witness sees the real data fails as
"window closed"; it never passes unproven.

Plain torch only; the library is reached through the case's own closure."""
import time

import numpy as np
import torch

MIN_WINDOW_MS = 20.0
MAX_WINDOW_MS = 500.0
SENTINEL = 0xEE

RESULTS = []                # one dict per check_late run: row, checks, blocking, call_ms, window_ms (DESIGN.md's table)
_cal = {}


class StreamOrderError(AssertionError):
    pass


def _chain_buffers(dev):
    if "chain" not in _cal:
        _cal["chain"] = torch.zeros(1 << 20, dtype=torch.float32, device=dev)
    return _cal["chain"]


def _spin(units, dev):
    """`units` of delay on the current stream: torch.cuda._sleep cycles, or (without it) that many passes of a torch op."""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
    else:
        buf = _chain_buffers(dev)
        for _ in range(int(units)):
            buf.add_(1.0)


def units_per_ms(dev="cuda:0"):
    """Delay units (cycles of torch.cuda._sleep, or passes of the fall-back chain) per millisecond, measured once per process
    with a pair of events on an idle stream."""
    if "upm" in _cal:
        return _cal["upm"]
    st = torch.cuda.Stream(dev)
    units = 2_000_000 if hasattr(torch.cuda, "_sleep") else 200
    ms = 0.0
    with torch.cuda.stream(st):
        _spin(units // 10, dev)                                    # load the kernel outside the timed pair
        st.synchronize()
        for _ in range(8):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            _spin(units, dev)
            e1.record(st)
            st.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0:
                break
            units *= 4
    if ms < 5.0:
        raise StreamOrderError(f"delay calibration: {units} units took only {ms:.3f} ms")
    _cal["upm"] = units / ms
    _cal["calibration"] = {"units": units, "ms": ms, "units_per_ms": units / ms,
                           "source": "torch.cuda._sleep" if hasattr(torch.cuda, "_sleep") else "torch op chain"}
    return _cal["upm"]


def calibration():
    units_per_ms()
    return dict(_cal["calibration"])


def delay(S, ms):
    """Keeps stream S busy for about `ms` milliseconds (asynchronous)."""
    dev = S.device
    with torch.cuda.stream(S):
        _spin(max(1, int(ms * units_per_ms(dev))), dev)


def choose_streams(dev="cuda:0", candidates=8):
    """(S, W): two torch streams that run beside each other -- a process opens few hardware queues and two torch streams may
    share one.  Probe, torch ops only: a sleep on S, a copy on W, then W.query() true while S.query() is false."""
    units_per_ms(dev)
    streams = [torch.cuda.Stream(dev) for _ in range(candidates)]
    a = torch.arange(4096, dtype=torch.int32, device=dev)
    b = torch.zeros_like(a)
    torch.cuda.synchronize()
    for S in streams:
        for W in streams:
            if W is S:
                continue
            delay(S, 40.0)
            with torch.cuda.stream(W):
                b.copy_(a, non_blocking=True)
            W.synchronize()
            ok = W.query() and not S.query()
            S.synchronize()
            if ok:
                return S, W
    raise StreamOrderError(f"no pair of {candidates} torch streams runs side by side: a copy on W never finished while S slept")


class Buf:
    """One device buffer of a case.  `real` is what the library must see (its inputs) or find (the pre-fill of its outputs);
    `decoy` is the valid stand-in that sits there until S delivers `real`; `expected` (None for a pure input that the call
    leaves alone -- then `real` is expected) is the whole buffer after the call, guard regions and row padding included.
    `mask` (bool per byte) names the bytes that are compared, for outputs whose other bytes the entry point leaves unspecified."""

    def __init__(self, name, t, real, decoy, expected=None, output=None, mask=None):
        assert t.is_cuda and t.is_contiguous(), name
        self.name, self.t = name, t
        flat = t.view(-1).view(torch.uint8)
        self.flat = flat
        self.real = _staged(real, flat)
        self.decoy = _staged(decoy, flat)
        self.output = (expected is not None) if output is None else output
        self.expected = _host_bytes(expected if expected is not None else real, flat.numel())
        self.mask = None if mask is None else np.ascontiguousarray(mask, bool).reshape(-1)
        assert self.mask is None or self.mask.size == flat.numel(), name
        self.snap = torch.empty_like(flat)
        self.sentinel = torch.full_like(flat, SENTINEL)
        self.witness = [torch.empty_like(flat) for _ in range(3)]
        self.late = not torch.equal(self.real, self.decoy)


def _host_bytes(x, nbytes):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().numpy()
    a = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    assert a.size == nbytes, (a.size, nbytes)
    return a.copy()


def _staged(x, like):
    return torch.from_numpy(_host_bytes(x, like.numel())).to(like.device)


def differences(got, expected, name, mask=None):
    """The one comparison of this module: '' when the (masked) bytes agree, else a sentence."""
    got = np.asarray(got).reshape(-1).view(np.uint8)
    wrong = got != expected if mask is None else (got != expected) & mask
    if not wrong.any():
        return ""
    bad = np.flatnonzero(wrong)
    return f"{name}: {bad.size} of {expected.size} bytes differ, first at {bad[0]}: got {got[bad[0]]} expected {expected[bad[0]]}"


def plain_run(row, bufs, call):
    """The call on the default stream with everything in place: must give the expected bytes (this separates 'wrong' from
    'wrong only when late').  Runs twice; returns the host time of the second call in ms."""
    ms = 0.0
    for _ in range(2):
        for b in bufs:
            b.flat.copy_(b.real)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        msgs = [m for m in (differences(b.flat.cpu().numpy(), b.expected, b.name, b.mask) for b in bufs) if m]
        if msgs:
            raise StreamOrderError(f"{row}: the plain run on the default stream is wrong -- " + "; ".join(msgs))
    return ms


def check_late(row, bufs, call, S, W, call_ms=None):
    """Runs `call` (a closure that enqueues on the CURRENT stream) on the delayed stream S and checks (a) late input, (b) early
    overwrite, (c) guards, and the witnesses.  `call` may return a callable: work the callee deferred, which the harness runs
    after the scribble (only the stand-ins of the self-test do).  Raises StreamOrderError; returns the results-table entry."""
    dev = S.device
    null = torch.cuda.default_stream(dev)
    if call_ms is None:
        call_ms = plain_run(row, bufs, call)
    window = max(MIN_WINDOW_MS, 10.0 * call_ms)
    if window > MAX_WINDOW_MS:
        raise StreamOrderError(f"{row}: the call takes {call_ms:.1f} ms on the host; a window of {window:.0f} ms exceeds the cap "
                               f"of {MAX_WINDOW_MS:.0f} ms, so the case cannot be proven")
    late = [b for b in bufs if b.late]
    assert late, f"{row}: no buffer differs between decoy and real"
    wb = ([b for b in late if not b.output] or late)[0]                       # the witnesses' buffer: an input the call only reads, if any
    for b in bufs:
        b.flat.copy_(b.decoy)
        b.snap.zero_()
    torch.cuda.synchronize()

    delay(S, window)
    opened = torch.cuda.Event()                                               # completes when the delay is over: the window closes
    opened.record(S)
    with torch.cuda.stream(S):
        for b in bufs:
            b.flat.copy_(b.real, non_blocking=True)
    with torch.cuda.stream(null):
        wb.witness[0].copy_(wb.flat, non_blocking=True)
    with torch.cuda.stream(W):
        wb.witness[1].copy_(wb.flat, non_blocking=True)
    with torch.cuda.stream(S):
        deferred = call()
    # A call that waits for S on the host (an upload it sends ahead, a status word it reads back) returns with the window
    # closed: it gets only the first witnesses.  Otherwise a second witness on W, which must have run to its end with the
    # window still open.
    blocking = opened.query()
    closed_under_witness = False
    if not blocking:
        with torch.cuda.stream(W):
            wb.witness[2].copy_(wb.flat, non_blocking=True)
        W.synchronize()
        closed_under_witness = opened.query()
    with torch.cuda.stream(S):
        for b in bufs:
            b.snap.copy_(b.flat, non_blocking=True)
        for b in bufs:
            b.flat.copy_(b.sentinel if (b.output and not b.late) else b.decoy, non_blocking=True)
        if callable(deferred):
            deferred()
    torch.cuda.synchronize()

    if closed_under_witness:
        raise StreamOrderError(f"{row}: window closed -- the call returned with the window open, but S was through its delay before "
                               f"the witness behind the call had run")
    decoy = wb.decoy.cpu().numpy()
    for k, who in ((0, "the null stream"), (1, "stream W"), (2, "stream W after the call")):
        if k == 2 and blocking:
            continue
        if differences(wb.witness[k].cpu().numpy(), decoy, wb.name):
            raise StreamOrderError(f"{row}: window closed -- the witness on {who} did not see the decoy of {wb.name}"
                                   + (": S delivered early, or the call wrote there ahead of S" if wb.output else ""))
    msgs = [m for m in (differences(b.snap.cpu().numpy(), b.expected, b.name, b.mask) for b in bufs) if m]
    entry = {"row": row, "checks": "a b c" if not msgs else "FAILED", "blocking": bool(blocking),
             "witnesses": 2 if blocking else 3, "call_ms": round(call_ms, 3), "window_ms": round(window, 1)}
    RESULTS.append(entry)
    if msgs:
        raise StreamOrderError(f"{row}: wrong only when late (window {window:.0f} ms, the call "
                               f"{'blocked' if blocking else 'returned at once'}) -- the call read before S delivered its inputs, "
                               f"or finished behind S's order -- " + "; ".join(msgs))
    return entry


def check_two_streams(row, bufs_a, call_a, bufs_b, call_b, S, W, stats, trim):
    """The block cache's cross-stream rule, by its own counters: a block released behind stream S goes to S again at once and
    to another stream only after its event.  `stats()` gives the library's cache counters as a dict, `trim()` empties the cache.

    With the cache emptied: call A on the delayed S (its scratch comes from the driver and is parked behind S), then at once call
    B -- the same entry point, other inputs of the same size class -- on the undelayed W, then A's call once more on S, all while
    S is still held up.  B must get nothing of what A parked (as many driver allocations as A made, no more hits than A had),
    A's second call must get everything from the cache.  A cache that hands a parked block to whoever asks serves B from the
    cache and fails here; the scratch of these calls is written before it is read, so their pixels could not show it.  The
    answers of A and B are compared all the same, and the window must still be open behind A's second call."""
    keys = ("device_driver_allocs", "device_hits", "device_bytes_cached")
    window = max(MIN_WINDOW_MS, 10.0 * (2.0 * plain_run(row + " (A)", bufs_a, call_a) + plain_run(row + " (B)", bufs_b, call_b)))
    if window > MAX_WINDOW_MS:
        raise StreamOrderError(f"{row}: a window of {window:.0f} ms exceeds the cap of {MAX_WINDOW_MS:.0f} ms")
    for b in bufs_a:
        b.flat.copy_(b.decoy)
    for b in bufs_b:
        b.flat.copy_(b.real)
    torch.cuda.synchronize()
    trim()
    s0 = stats()
    if s0["device_bytes_cached"] != 0:
        raise StreamOrderError(f"{row}: the cache still holds {s0['device_bytes_cached']} bytes after a trim")
    delay(S, window)
    opened = torch.cuda.Event()
    opened.record(S)
    with torch.cuda.stream(S):
        for b in bufs_a:
            b.flat.copy_(b.real, non_blocking=True)
        call_a()
        for b in bufs_a:
            b.snap.copy_(b.flat, non_blocking=True)
    s1 = stats()
    with torch.cuda.stream(W):
        call_b()
        for b in bufs_b:
            b.snap.copy_(b.flat, non_blocking=True)
    s2 = stats()
    with torch.cuda.stream(S):
        call_a()
    s3 = stats()
    still_open = not opened.query()
    torch.cuda.synchronize()
    if not still_open:
        raise StreamOrderError(f"{row}: window closed -- stream S was through its delay before the three calls were queued")
    a, b, a2 = ({k: y[k] - x[k] for k in keys} for x, y in ((s0, s1), (s1, s2), (s2, s3)))
    counters = f"counters of A on S, B on W, A again on S: {a}, {b}, {a2}"
    if a["device_driver_allocs"] < 1 or a["device_bytes_cached"] <= 0:
        raise StreamOrderError(f"{row}: the call parked no scratch behind its stream -- {counters}")
    if b["device_driver_allocs"] != a["device_driver_allocs"] or b["device_hits"] > a["device_hits"]:
        raise StreamOrderError(f"{row}: a block parked behind the held-up stream S was handed to stream W -- {counters}")
    if a2["device_driver_allocs"] != 0 or a2["device_hits"] != a["device_driver_allocs"] + a["device_hits"]:
        raise StreamOrderError(f"{row}: the blocks parked behind S did not go to the next call on S at once -- {counters}")
    msgs = [m for m in (differences(x.snap.cpu().numpy(), x.expected, "A: " + x.name, x.mask) for x in bufs_a) if m]
    msgs += [m for m in (differences(x.snap.cpu().numpy(), x.expected, "B: " + x.name, x.mask) for x in bufs_b) if m]
    if msgs:
        raise StreamOrderError(f"{row}: wrong when two streams share the block cache (window {window:.0f} ms) -- " + "; ".join(msgs))
    return {"row": row, "window_ms": round(window, 1), "A": a, "B": b, "A again": a2}
