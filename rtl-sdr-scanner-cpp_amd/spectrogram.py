"""ctypes view of include/specscan_spectrogram_feed.h — the spectrogram rows delivered through the pipelined feed
(``Feed.spectrogram``): the reference's per-frame send gate (Spectrogram::work / send, sources/radio/blocks/spectrogram.cpp:29-75)
behind every submitted batch. Test and tooling plumbing; the compute is csrc/spectrogram_rows.h, the gate csrc/spectrogram_gate.h."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from .abi import SpecscanError

SGF_ABI_VERSION = 1
SGF_MAX_ROWS = 64
SGF_EXPORTS = ("sgf_create", "sgf_destroy", "sgf_gate_plan", "sgf_last_error", "sgf_rows")
SGF_RING_EXPORTS = ("sgf_batch_db_rows", "sgf_create_ring")  # include/specscan_spectrogram_feed_ring.h


class SgfConfig(C.Structure):  # sgf_config
    _fields_ = [("abi_version", C.c_uint32), ("max_rows", C.c_int32), ("want_mean", C.c_int32)]


class SgfResult(C.Structure):  # sgf_result
    _fields_ = [("nrows", C.c_int32), ("size", C.c_int32), ("frequency", C.c_int32), ("sample_rate", C.c_int32), ("open_count", C.c_int32),
                ("time_ms", C.POINTER(C.c_int64)), ("frame", C.POINTER(C.c_int32)), ("count", C.POINTER(C.c_int32)),
                ("rows", C.POINTER(C.c_int8)), ("mean", C.POINTER(C.c_float))]


def bind_spectrogram_feed(lib: C.CDLL) -> C.CDLL:
    lib.sgf_create.argtypes = [C.c_void_p, C.POINTER(SgfConfig), C.POINTER(C.c_void_p)]
    lib.sgf_create.restype = C.c_int
    lib.sgf_destroy.argtypes = [C.c_void_p]
    lib.sgf_destroy.restype = None
    lib.sgf_last_error.argtypes = [C.c_void_p]
    lib.sgf_last_error.restype = C.c_char_p
    lib.sgf_rows.argtypes = [C.c_void_p, C.POINTER(SgfResult)]
    lib.sgf_rows.restype = C.c_int
    lib.sgf_gate_plan.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    lib.sgf_gate_plan.restype = C.c_int32
    return lib


def bind_spectrogram_feed_ring(lib: C.CDLL) -> C.CDLL:
    """include/specscan_spectrogram_feed_ring.h on top of bind_spectrogram_feed."""
    bind_spectrogram_feed(lib)
    lib.sgf_create_ring.argtypes = [C.c_void_p, C.POINTER(SgfConfig), C.POINTER(C.c_void_p)]
    lib.sgf_create_ring.restype = C.c_int
    lib.sgf_batch_db_rows.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float)]
    lib.sgf_batch_db_rows.restype = C.c_int
    return lib


class Gate:
    """sgf_gate_plan with its state: the reference's send gate of ONE centre frequency's container (host only, no GPU).
    ``plan(t_ms, cap)`` -> (rows closed, the first min(rows, cap) closing frames)."""

    def __init__(self, lib: C.CDLL | None = None):
        if lib is None:
            from .engine import load_library
            lib = load_library()
        self._lib = bind_spectrogram_feed(lib)
        self.last_send, self.have_last = C.c_int64(0), C.c_int32(0)

    def plan(self, t_ms, cap: int = SGF_MAX_ROWS):
        t = np.ascontiguousarray(t_ms, dtype=np.int64).reshape(-1)
        cut = np.zeros(max(int(cap), 1), np.int32)
        n = self._lib.sgf_gate_plan(C.byref(self.last_send), C.byref(self.have_last), t.ctypes.data_as(C.POINTER(C.c_int64)), t.size,
                                    cut.ctypes.data_as(C.POINTER(C.c_int32)), int(cap))
        if n < 0:
            raise SpecscanError(n, "sgf_gate_plan: bad argument")
        return n, cut[:min(n, int(cap))].copy()


def frame_payloads(payloads) -> bytes:
    """The file form of ``replay_file(spectrogram=...)`` and ``specscan_replay --spectrogram-out``: every payload behind its
    length as a little-endian uint32."""
    return b"".join(struct.pack("<I", len(p)) + p for p in payloads)


class SpectrogramFeed:
    """One sgf_ctx bound to a Feed of an engine with ``flags=SS_FLAG_SPECTROGRAM`` (``Feed.spectrogram``). From now on every
    ``submit`` needs ``t_ms``, and ``rows()`` after a collect (the feed's own, or a TrackedFeed's; also while a RecordedFeed holds
    the batch) gives the rows that batch closed. The feed and its engine must outlive the object.
    ``ring=True`` (include/specscan_spectrogram_feed_ring.h, sgf_create_ring): the engine has NO SS_FLAG_SPECTROGRAM; from 65536
    points up the batches then go through the feed as ``process_device`` makes its calls, and the rows of a batch that kept no dB
    plane are formed from the rows it left in the averager ring's buffer."""

    def __init__(self, feed, max_rows: int = 8, want_mean: bool = False, ring: bool = False):
        self._feed = feed
        self._lib = bind_spectrogram_feed_ring(feed._lib)
        self.ring = bool(ring)
        self.cfg = SgfConfig(SGF_ABI_VERSION, int(max_rows), int(bool(want_mean)))
        h = C.c_void_p()
        create = self._lib.sgf_create_ring if self.ring else self._lib.sgf_create
        st = create(feed._h, C.byref(self.cfg), C.byref(h))
        if st != 0:
            raise SpecscanError(st, (self._lib.sgf_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._feed._e, "_h", None):  # (an engine closed first took its lock with it)
                self._lib.sgf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self) -> dict:
        """The batch collected last: nrows, size, frequency, sample_rate, open_count; time_ms / frame / count [nrows]; rows
        [nrows, size] int8; mean [nrows, size] float32 (want_mean) — numpy views of the slot's pinned memory, valid until the slot
        is acquired again — and ``payloads()``, one DataController::pushSpectrogram payload (engine.spectrogram_payload) per row."""
        r = SgfResult()
        st = self._lib.sgf_rows(self._h, C.byref(r))
        if st != 0:
            raise SpecscanError(st, (self._lib.sgf_last_error(self._h) or b"").decode())
        k, size = r.nrows, r.size

        def view(p, shape):
            return np.ctypeslib.as_array(p, shape=tuple(max(d, 1) for d in shape))[tuple(slice(0, d) for d in shape)]

        out = {"nrows": k, "size": size, "frequency": r.frequency, "sample_rate": r.sample_rate, "open_count": r.open_count,
               "time_ms": view(r.time_ms, (k,)), "frame": view(r.frame, (k,)), "count": view(r.count, (k,)), "rows": view(r.rows, (k, size))}
        if r.mean:
            out["mean"] = view(r.mean, (k, size))

        def payloads():
            from .engine import spectrogram_payload
            return [spectrogram_payload(int(out["time_ms"][i]), out["frequency"], out["sample_rate"], out["rows"][i]) for i in range(k)]

        out["payloads"] = payloads
        return out

    def batch_db_rows(self, frame0: int = 0, nframes: int | None = None) -> np.ndarray:
        """sgf_batch_db_rows: the dB rows [frame0, frame0 + nframes) of the batch SUBMITTED last, [nframes, N] float32 in bin order
        (a copy), from the plane or from the ring's buffer, wherever the batch left them. ``nframes=None``: up to the batch's end."""
        if nframes is None:
            nframes = self._feed.last_submitted - int(frame0)
        out = np.empty((int(nframes), self._feed._e.n), np.float32)
        st = self._lib.sgf_batch_db_rows(self._h, int(frame0), int(nframes), out.ctypes.data_as(C.POINTER(C.c_float)))
        if st != 0:
            raise SpecscanError(st, (self._lib.sgf_last_error(self._h) or b"").decode())
        return out

    def payloads(self) -> list:
        """``rows()["payloads"]()``: the payloads of the batch collected last."""
        return self.rows()["payloads"]()


__all__ = ["SpectrogramFeed", "Gate", "SGF_EXPORTS", "SGF_RING_EXPORTS", "SGF_ABI_VERSION", "SGF_MAX_ROWS", "bind_spectrogram_feed", "bind_spectrogram_feed_ring",
           "frame_payloads"]
