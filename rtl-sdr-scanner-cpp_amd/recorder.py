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


__all__ = ["RecordedFeed", "RangePlanner", "SRF_EXPORTS", "SRF_ABI_VERSION", "SC_MAX_RANGES", "bind_record_feed"]
