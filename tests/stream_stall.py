"""Test-side tools that turn a missing cross-stream wait into a wrong number every time (tests/test_stream_order_gpu.py).

* `stall(stream, ms)` queues a bounded busy kernel on `stream`: whatever is queued behind it on that stream is late by `ms`, so work
  on another stream that should have waited for it, and does not, runs first and reads what is not there yet;
* `poison_free_blocks()` overwrites every block the caching allocator considers free with 0xFF bytes (four of them are an fp32 NaN):
  dropped, the blocks go back to the cache full of NaN and a read-before-write of a `torch.empty` workspace shows as NaN; kept alive,
  they are what the allocator would have handed out next, so a block that was released while a kernel still reads it is destroyed;
* `run_stalled(...)` sizes a stall from the host-side duration of the call under test and holds the validity condition: the stall is
  still running when the call returns (otherwise the call merely waited for it and nothing was exercised).

Nothing here may fault: the busy kernel touches no memory, the poison is written into tensors this module allocated itself."""
import time

import torch

MAX_STALL_MS = 1000.0  # no single stall is longer than this
MIN_STALL_MS = 50.0
_SMALL_REQUEST = 1 << 20  # the caching allocator's largest request that goes to its small segments

_calibration = {}  # device index -> ("sleep", cycles per ms) or ("mm", matrix, products per ms)


class StallEvent(torch.cuda.Event):
    """The event recorded right behind a stall; `.start` was recorded right in front of it (both with timing)."""


def _calibrate(device: int):
    if device in _calibration:
        return _calibration[device]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1_000_000)  # (first launch: module load)
        torch.cuda.synchronize()
        cycles = 20_000_000
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        torch.cuda.synchronize()
        _calibration[device] = ("sleep", cycles / max(e0.elapsed_time(e1), 1e-3))
    else:
        a = torch.ones((1024, 1024), device=f"cuda:{device}")
        for _ in range(3):
            torch.mm(a, a)
        torch.cuda.synchronize()
        n = 50
        e0.record()
        for _ in range(n):
            torch.mm(a, a)
        e1.record()
        torch.cuda.synchronize()
        _calibration[device] = ("mm", a, n / max(e0.elapsed_time(e1), 1e-3))
    return _calibration[device]


def stall(stream, ms: float) -> StallEvent:
    """Queue a busy kernel of about `ms` milliseconds (at most MAX_STALL_MS) on `stream`.  -> the event recorded right behind it:
    `not event.query()` = the stall is still running; after a synchronize, `realised_ms(event)` is how long it really took."""
    ms = float(min(ms, MAX_STALL_MS))
    cal = _calibrate(torch.cuda.current_device())
    ev = StallEvent(enable_timing=True)
    ev.start = torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        ev.start.record(stream)
        if cal[0] == "sleep":
            torch.cuda._sleep(max(1, int(cal[1] * ms)))
        else:
            for _ in range(max(1, int(cal[2] * ms))):
                torch.mm(cal[1], cal[1])
        ev.record(stream)
    return ev


def realised_ms(ev: StallEvent) -> float:
    return float(ev.start.elapsed_time(ev))


def poison_free_blocks():
    """Every inactive cached block of the current device, allocated again (exactly its size, on the stream whose pool owns it) and
    filled with 0xFF.  -> the tensors: drop them to re-cache the blocks full of NaN, keep them to deny the blocks to everybody else."""
    dev = torch.cuda.current_device()
    wanted = []  # (size, raw stream handle)
    for seg in torch.cuda.memory_snapshot():
        if seg["device"] != dev:
            continue
        for b in seg["blocks"]:
            if b["state"] != "inactive":
                continue
            size, handle = int(b["size"]), int(seg.get("stream", 0))
            if seg.get("segment_type") == "small":
                # requests above 1 MiB are served from the pool of large segments: a (merged) free block of a small segment
                # that is larger than that is taken in pieces of 1 MiB and a rest, which split it exactly
                wanted.extend([(_SMALL_REQUEST, handle)] * (size // _SMALL_REQUEST))
                size %= _SMALL_REQUEST
            if size:
                wanted.append((size, handle))
    # largest first: the free blocks of a pool and the requests to it are then the same multiset of sizes at every step, so every
    # request finds a block of exactly its size (best fit) and nothing new is allocated
    wanted.sort(reverse=True)
    out = []
    for size, handle in wanted:
        st = torch.cuda.default_stream(dev) if handle == 0 else torch.cuda.ExternalStream(handle, device=dev)
        with torch.cuda.stream(st):
            t = torch.empty((size,), dtype=torch.uint8, device=f"cuda:{dev}")
            t.fill_(0xFF)
        out.append(t)
    return out


def holds(tensors, ptr: int) -> bool:
    """Whether the device address `ptr` lies inside one of `tensors`."""
    return any(t.data_ptr() <= ptr < t.data_ptr() + t.numel() * t.element_size() for t in tensors)


class StalledRun:
    def __init__(self, value, event, requested_ms, host_s, unstalled_host_s):
        self.value, self.event, self.requested_ms = value, event, requested_ms
        self.host_s, self.unstalled_host_s = host_s, unstalled_host_s  # host time of the call: behind the stall / without one

    @property
    def realised_ms(self):
        return realised_ms(self.event)


def run_stalled(stream_of, prepare, call, finish, unstalled_host_s=None, behind=None):
    """The call under test with `stream_of()` stalled right in front of it.

    prepare() -> state (everything up to the call; poisons);  call(state) = the host call under test;  finish(state, stalled) ->
    value runs right after the validity check and must end with the device idle (`torch.cuda.synchronize()`);  behind(state), if
    given, queues work right behind the stall (and, for an equal host-side duration, at the same place of the unstalled run).
    The stall is 10 x the host-side duration of one unstalled run of the same call (measured here unless given), 50 ms at least;
    it must still be running when `call` returns -- if not it is doubled once, and if it is over again the test FAILS.
    -> (StalledRun of the stalled run, value of the unstalled run or None when `unstalled_host_s` was given)."""
    plain = None
    if unstalled_host_s is None:
        state = prepare()
        if behind is not None:
            behind(state)
        t0 = time.perf_counter()
        call(state)
        unstalled_host_s = time.perf_counter() - t0
        plain = finish(state, False)
    ms = max(MIN_STALL_MS, 10.0 * 1e3 * unstalled_host_s)
    for _ in range(2):
        state = prepare()
        ev = stall(stream_of(), ms)
        if behind is not None:
            behind(state)
        t0 = time.perf_counter()
        call(state)
        running = not ev.query()
        host_s = time.perf_counter() - t0
        value = finish(state, True)
        if running:
            return StalledRun(value, ev, min(ms, MAX_STALL_MS), host_s, unstalled_host_s), plain
        ms *= 2.0
    raise AssertionError(f"the stall ({min(ms / 2.0, MAX_STALL_MS):.0f} ms requested, {realised_ms(ev):.1f} ms realised) was over when the call "
                         f"under test returned after {host_s * 1e3:.1f} ms of host time: the call waited for it, or the stall is too short")
