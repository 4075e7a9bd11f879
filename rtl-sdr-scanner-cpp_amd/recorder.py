"""ctypes view of include/specscan_record_feed.h — the recorder bound to the pipelined feed (``Feed.record``) — and the host
logic that turns a batch's per-frame tracker lists into the sample ranges it records: ``RangePlanner``, the reference's
SdrDevice::updateRecordings (sources/radio/sdr_device.cpp:82-144) walked frame by frame, i.e. host/recorder_bank.h restated in
Python. Test and tooling plumbing; the compute is csrc/channelizer.hip."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import SpecscanError
from .channelizer import SC_MAX_CHANNELS, SC_MAX_RANGES, ScRange, _ranges

SRF_ABI_VERSION = 2
SRF_EXPORTS = ("srf_create", "srf_destroy", "srf_last_error", "srf_record", "srf_release")


class SrfConfig(C.Structure):  # srf_config
    _fields_ = [("abi_version", C.c_uint32), ("bandwidth", C.c_int32), ("threshold", C.c_int32), ("channels", C.c_int32),
                ("pack_scale", C.c_float), ("want_cf32", C.c_int32)]


class SrfResult(C.Structure):  # srf_result
    _fields_ = [("nsamples", C.c_int32), ("cap", C.c_int32), ("counts", C.POINTER(C.c_int32)), ("range_counts", C.POINTER(C.c_int32)),
                ("out_i8", C.POINTER(C.c_int8)), ("out_cf32", C.POINTER(C.c_float)), ("h2d_bytes", C.c_uint64)]


def bind_record_feed(lib: C.CDLL) -> C.CDLL:
    lib.srf_create.argtypes = [C.c_void_p, C.POINTER(SrfConfig), C.POINTER(C.c_void_p)]
    lib.srf_create.restype = C.c_int
    lib.srf_destroy.argtypes = [C.c_void_p]
    lib.srf_destroy.restype = None
    lib.srf_last_error.argtypes = [C.c_void_p]
    lib.srf_last_error.restype = C.c_char_p
    lib.srf_record.argtypes = [C.c_void_p, C.POINTER(ScRange), C.c_int32, C.POINTER(SrfResult)]
    lib.srf_record.restype = C.c_int
    lib.srf_release.argtypes = [C.c_void_p]
    lib.srf_release.restype = C.c_int
    return lib


class RecordedFeed:
    """One srf_ctx bound to a Feed (``Feed.record``): of an engine with decim 1, or an items feed (``engine.feed(items=True)``) of
    any engine. From now on every collect of the feed (its own, or a TrackedFeed's) leaves the batch held: ``record(ranges)``
    channelises sample ranges of it and lets it go, ``release()`` lets it go unrecorded. With decim 1 the samples are the upload
    that is still on the device; on an items feed of a decimated engine they are the batch's whole items in the slot's pinned
    memory, of which only the union of the ranges is uploaded (``last_h2d_bytes``). ``RangePlanner(channels, N * decim)`` is the
    planner for an items feed: a frame of the tracker's lists stands for one item of the stream. The feed and its engine must
    outlive the object."""

    def __init__(self, feed, bandwidth: int, channels: int = 4, threshold: int = 125, pack_scale: float = 127.0, want_cf32: bool = False):
        self._feed = feed
        self._lib = bind_record_feed(feed._lib)
        self.cfg = SrfConfig(SRF_ABI_VERSION, int(bandwidth), int(threshold), int(channels), float(pack_scale), int(bool(want_cf32)))
        h = C.c_void_p()
        st = self._lib.srf_create(feed._h, C.byref(self.cfg), C.byref(h))
        if st != 0:
            raise SpecscanError(st, (self._lib.srf_last_error(None) or b"").decode())
        self._h = h
        self.last_h2d_bytes = 0  # srf_result.h2d_bytes of the last record()

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._feed._e, "_h", None):  # (an engine closed first took its lock with it)
                self._lib.srf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise SpecscanError(st, (self._lib.srf_last_error(self._h) or b"").decode())

    def release(self):
        self._check(self._lib.srf_release(self._h))

    def record(self, ranges):
        """ranges: [(channel, shift_hz, begin, end), ...] in samples of the held batch's stream: frame f is f * N .. (f + 1) * N, or
        on an items feed f * N * decim .. f * N * decim + N with the rest of its item behind it. Returns
        ({channel: (int8 [m, 2], complex64 [m] or None)} for every channel with a range, range_counts), numpy copies;
        ``last_h2d_bytes`` is what the call uploaded."""
        arr, n = _ranges(ranges)
        r = SrfResult()
        self._check(self._lib.srf_record(self._h, arr, n, C.byref(r)))
        self.last_h2d_bytes = int(r.h2d_bytes)
        nch, cap = self.cfg.channels, r.cap
        counts = np.ctypeslib.as_array(r.counts, shape=(nch,)).copy()
        rc = np.ctypeslib.as_array(r.range_counts, shape=(max(n, 1),))[:n].copy()
        out = {}
        for ch in sorted({int(arr[i].channel) for i in range(n)}):
            m = int(min(counts[ch], cap))
            i8 = np.ctypeslib.as_array(r.out_i8, shape=(nch, cap, 2))[ch, :m].copy() if m else np.zeros((0, 2), np.int8)
            cf = None
            if r.out_cf32:
                cf = np.ctypeslib.as_array(r.out_cf32, shape=(nch, cap, 2))[ch, :m].copy().view(np.complex64).reshape(-1) if m else np.zeros(0, np.complex64)
            out[ch] = (i8, cf)
        return out, rc


IDLE = 2**31 - 1  # Recorder::getShift while idle


class RangePlanner:
    """SdrDevice::updateRecordings (sdr_device.cpp:82-144) over the per-frame lists of one batch after another. Per frame, in the
    reference's order: recorders whose shift is no longer wanted stop; then for every (shift, flush) of the frame's list the
    recorder on that shift flushes if asked, or the first idle recorder starts on it, or — none idle — the shift is ignored.
    Then the frame's samples go to every recording slot. The slots' state carries from batch to batch.

    ``plan(frames)`` -> (ranges, ends, flushes): sc_range tuples (channel, shift_hz, begin, end) in samples of the batch, frame f
    being f * n .. (f + 1) * n, merged while a slot keeps recording on its shift (the tracker asks a running recording to flush in
    almost every frame: a flush cuts nothing), in the order they end. ends[i] says what closed ranges[i]: "stop" (the recording
    ended; the reference drops what was not flushed) or "batch" (the batch ended, the recording goes on at sample 0 of the next).
    flushes[i]: the range ends with a flush — the tracker asked the slot to flush in the range's last frame, so the host may
    publish everything the slot has gathered up to the end of this range. A batch seldom needs more than a few ranges;
    more than SC_MAX_RANGES do not fit one srf_record: plan fewer frames at a time."""

    def __init__(self, channels: int, n: int):
        if not 1 <= channels <= SC_MAX_CHANNELS:
            raise ValueError("channels")
        self.n = int(n)
        self.slots = [{"rec": False, "shift": IDLE} for _ in range(channels)]
        self.ignored = set()

    def plan(self, frames):
        ranges, ends, flushes = [], [], []
        begin = {k: 0 for k, s in enumerate(self.slots) if s["rec"]}  # a recording that spans batches goes on at sample 0
        flush_frame = {}  # slot -> the last frame whose list asked it to flush

        def close(k, at, why):
            ranges.append((k, self.slots[k]["shift"], begin.pop(k), at))
            ends.append(why)
            flushes.append(at > 0 and flush_frame.get(k) == at // self.n - 1)

        nframes = 0
        for f, want in enumerate(frames):
            nframes = f + 1
            at = f * self.n
            shifts = [int(s) for s, _ in want]
            for k, s in enumerate(self.slots):  # sdr_device.cpp:103-111
                if s["rec"] and s["shift"] not in shifts:
                    close(k, at, "stop")
                    s.update(rec=False, shift=IDLE)
                    flush_frame.pop(k, None)
            for shift, flush in want:  # sdr_device.cpp:113-136
                hit = [k for k, s in enumerate(self.slots) if s["shift"] == int(shift)]
                if hit:
                    if flush:
                        flush_frame[hit[0]] = f
                else:
                    free = [k for k, s in enumerate(self.slots) if not s["rec"]]
                    if free:
                        self.slots[free[0]].update(rec=True, shift=int(shift))
                        begin[free[0]] = at
                    else:
                        self.ignored.add(int(shift))  # "no recorders available"
            self.ignored = {s for s in self.ignored if s in shifts}
        for k in sorted(begin):
            close(k, nframes * self.n, "batch")
        return ranges, ends, flushes


SRP_EXPORTS = ("srp_create", "srp_destroy", "srp_last_error", "srp_plan", "srp_slots", "srp_ignored")
SRS_EXPORTS = ("srs_create", "srs_destroy", "srs_item_samples", "srs_feed", "srs_finish", "srs_published", "srs_dropped", "srs_pending_samples",
               "srs_held_items")
_PUBLISH_FN = C.CFUNCTYPE(None, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_int32, C.c_void_p)  # srs_publish_fn
_FRAME_TIME_FN = C.CFUNCTYPE(C.c_int64, C.c_int64, C.c_void_p)  # srs_frame_time_fn
_ENDS = ("stop", "batch")  # specscan::RangeEnd


def bind_recording_host(lib: C.CDLL) -> C.CDLL:
    """srp_* and srs_* of host/libspecscan_host.so (host/recording_host.cpp): the C++ RangePlanner and RecordingStore."""
    if getattr(lib, "_srp_bound", False):
        return lib
    i32p = C.POINTER(C.c_int32)
    lib.srp_create.argtypes = [C.c_int32, C.c_int64]
    lib.srp_create.restype = C.c_void_p
    lib.srp_destroy.argtypes = [C.c_void_p]
    lib.srp_destroy.restype = None
    lib.srp_last_error.argtypes = [C.c_void_p]
    lib.srp_last_error.restype = C.c_char_p
    lib.srp_plan.argtypes = [C.c_void_p, C.c_int32, i32p, i32p, C.POINTER(C.c_uint8), C.POINTER(ScRange), i32p, i32p]
    lib.srp_plan.restype = C.c_int32
    lib.srp_slots.argtypes = [C.c_void_p, i32p, i32p]
    lib.srp_slots.restype = C.c_int32
    lib.srp_ignored.argtypes = [C.c_void_p, i32p, C.c_int32]
    lib.srp_ignored.restype = C.c_int32
    lib.srs_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, _PUBLISH_FN, C.c_void_p]
    lib.srs_create.restype = C.c_void_p
    lib.srs_destroy.argtypes = [C.c_void_p]
    lib.srs_destroy.restype = None
    lib.srs_item_samples.argtypes = [C.c_void_p]
    lib.srs_item_samples.restype = C.c_int32
    lib.srs_feed.argtypes = [C.c_void_p, C.POINTER(ScRange), C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, _FRAME_TIME_FN, C.c_void_p]
    lib.srs_feed.restype = C.c_int32
    lib.srs_finish.argtypes = [C.c_void_p]
    lib.srs_finish.restype = None
    for name in ("srs_published", "srs_dropped"):
        getattr(lib, name).argtypes = [C.c_void_p]
        getattr(lib, name).restype = C.c_uint64
    for name in ("srs_pending_samples", "srs_held_items"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int32]
        getattr(lib, name).restype = C.c_int32
    lib._srp_bound = True
    return lib


def _host_lib() -> C.CDLL:
    from .tracker import load_host_library
    return bind_recording_host(load_host_library())


class HostRangePlanner:
    """specscan::RangePlanner (host/range_planner.h) through srp_*: RangePlanner above restated in C++, the planner
    ``specscan_replay --record-out`` runs. Same ``plan`` and the same state; a plan of more than SC_MAX_RANGES ranges raises
    ValueError and changes nothing (the Python class returns it: one srf_record would refuse it)."""

    def __init__(self, channels: int, n: int):
        self._lib = _host_lib()
        self._h = self._lib.srp_create(int(channels), int(n))
        if not self._h:
            raise ValueError("channels")
        self.n = int(n)
        self.channels = int(channels)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def plan(self, frames):
        frames = [list(f) for f in frames]
        off = np.zeros(len(frames) + 1, np.int32)
        off[1:] = np.cumsum([len(f) for f in frames])
        shifts = np.array([int(s) for f in frames for s, _ in f] + [0], np.int32)  # (+ one: never an empty array's pointer)
        flush = np.array([bool(x) for f in frames for _, x in f] + [0], np.uint8)
        ranges, ends, flushes = (ScRange * SC_MAX_RANGES)(), (C.c_int32 * SC_MAX_RANGES)(), (C.c_int32 * SC_MAX_RANGES)()
        n = self._lib.srp_plan(self._h, len(frames), off.ctypes.data_as(C.POINTER(C.c_int32)), shifts.ctypes.data_as(C.POINTER(C.c_int32)),
                               flush.ctypes.data_as(C.POINTER(C.c_uint8)), ranges, ends, flushes)
        if n < 0:
            raise ValueError((self._lib.srp_last_error(self._h) or b"").decode())
        return ([(ranges[i].channel, ranges[i].shift_hz, ranges[i].begin, ranges[i].end) for i in range(n)], [_ENDS[ends[i]] for i in range(n)],
                [bool(flushes[i]) for i in range(n)])

    @property
    def slots(self):
        """[{"rec": bool, "shift": int}, ...] as RangePlanner.slots."""
        sh, rec = (C.c_int32 * self.channels)(), (C.c_int32 * self.channels)()
        self._lib.srp_slots(self._h, sh, rec)
        return [{"rec": bool(rec[k]), "shift": int(sh[k])} for k in range(self.channels)]

    @property
    def ignored(self):
        n = self._lib.srp_ignored(self._h, None, 0)
        out = (C.c_int32 * max(n, 1))()
        self._lib.srp_ignored(self._h, out, n)
        return {int(out[i]) for i in range(n)}


class HostRecordingStore:
    """specscan::RecordingStore (host/recording_store.h) through srs_*: the 100 ms items of every slot, gathered from the outputs of
    planned ranges. ``published`` collects (time_ms, frequency, sample_rate, bytes of the int8 (re,im) samples) in publishing
    order; ``frame_time`` maps an absolute frame index to ms."""

    def __init__(self, channels: int, center_frequency: int, bandwidth: int, stride: int, frame_time):
        self._lib = _host_lib()
        self.published = []
        self._frame_time = frame_time
        self._publish_cb = _PUBLISH_FN(lambda t, f, rate, iq, n, _u: self.published.append((int(t), int(f), int(rate), C.string_at(iq, 2 * n))))
        self._time_cb = _FRAME_TIME_FN(lambda frame, _u: int(self._frame_time(int(frame))))
        self._h = self._lib.srs_create(int(channels), int(center_frequency), int(bandwidth), int(stride), self._publish_cb, None)
        if not self._h:
            raise ValueError("channels, bandwidth or stride")
        self.item_samples = int(self._lib.srs_item_samples(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.srs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, rng, end: str, flush: bool, iq_i8: np.ndarray, first_frame: int):
        """rng: (channel, shift_hz, begin, end); iq_i8: the range's outputs, int8 [count, 2]."""
        a = np.ascontiguousarray(iq_i8, np.int8).reshape(-1, 2)
        r = ScRange(*(int(v) for v in rng))
        if self._lib.srs_feed(self._h, C.byref(r), _ENDS.index(end), int(bool(flush)), a.ctypes.data if len(a) else None, len(a), int(first_frame),
                              self._time_cb, None) != 0:
            raise ValueError("srs_feed")

    def finish(self):
        self._lib.srs_finish(self._h)

    @property
    def dropped(self) -> int:
        return int(self._lib.srs_dropped(self._h))

    @property
    def published_items(self) -> int:
        return int(self._lib.srs_published(self._h))

    def pending_samples(self, slot: int) -> int:
        return int(self._lib.srs_pending_samples(self._h, int(slot)))

    def held_items(self, slot: int) -> int:
        return int(self._lib.srs_held_items(self._h, int(slot)))


__all__ = ["RecordedFeed", "RangePlanner", "HostRangePlanner", "HostRecordingStore", "SRF_EXPORTS", "SRF_ABI_VERSION", "SRP_EXPORTS", "SRS_EXPORTS",
           "SC_MAX_RANGES", "bind_record_feed", "bind_recording_host"]
