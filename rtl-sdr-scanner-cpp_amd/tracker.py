"""ctypes binding of host/libspecscan_host.so — the host-side signal tracker (host/signal_tracker.h), the part of
the reference's Transmission block that turns per-frame candidates into the Scanner's (shift Hz, flush) list — and of the
st_* entry points of libspecscan.so (include/specscan_track.h), the device-side digest that tracker can run on instead of
the rel and avg planes, with its form for engines that keep no planes
(include/specscan_track_digest_sparse.h) — and of the stf_* entry points (include/specscan_track_feed.h), the same digest behind the pipelined feed, with
its form for engines that keep no planes (include/specscan_track_sparse.h)."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from .build import HOST_LIB, build_host_lib

_lib = None
c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)


def load_host_library() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB):
            build_host_lib()
        lib = C.CDLL(HOST_LIB)
        lib.sst_create.argtypes = [C.c_int, C.c_int32, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int32]
        lib.sst_create.restype = C.c_void_p
        lib.sst_destroy.argtypes = [C.c_void_p]
        lib.sst_reset.argtypes = [C.c_void_p]
        lib.sst_process_frame.argtypes = [C.c_void_p, C.c_int64, c_float_p, c_float_p, c_int32_p, C.c_int, c_int32_p, C.c_int, c_int32_p,
                                          C.c_int, C.POINTER(C.c_int)]
        lib.sst_process_frame.restype = C.c_int
        lib.sst_process_frame_digest.argtypes = [C.c_void_p, C.c_int64, c_int32_p, c_float_p, c_int32_p, C.c_int, c_int32_p, C.c_int, c_int32_p,
                                                 c_float_p, c_int32_p, C.c_int, c_int32_p, C.c_int, C.POINTER(C.c_int)]
        lib.sst_process_frame_digest.restype = C.c_int
        _lib = lib
    return _lib


def index_step(bandwidth_hz: int, sample_rate: int, fft_size: int) -> int:
    """indexStep of SdrDevice::setupChains (reference sources/radio/sdr_device.cpp:151)."""
    return int(math.ceil(bandwidth_hz / (sample_rate / fft_size)))


class SignalTracker:
    def __init__(self, fft_size, sample_rate, start_level=8.0, stop_level=5.0, group_size=None, grouping_y=21, min_time_ms=2000,
                 timeout_ms=2000, tuning_step=2500, bandwidth=32000):
        self._lib = load_host_library()
        if group_size is None:
            group_size = index_step(bandwidth, sample_rate, fft_size)
        self.n = fft_size
        self._h = self._lib.sst_create(fft_size, sample_rate, start_level, stop_level, group_size, grouping_y, min_time_ms, timeout_ms, tuning_step)
        if not self._h:
            raise ValueError("bad tracker configuration")
        self._tx = np.empty(2 * fft_size, np.int32)
        self._sig = np.empty(fft_size, np.int32)
        self.group_size = group_size
        self.start_level = start_level
        self.keys = np.zeros(0, np.int32)  # the tracked keys after the last frame: what the next st_digest must watch

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sst_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._lib.sst_reset(self._h)
        self.keys = np.zeros(0, np.int32)

    def process_frame(self, now_ms: int, avg_row: np.ndarray, rel_row: np.ndarray, candidates: np.ndarray):
        """Returns (transmissions [k, 2] = (shift Hz, flush), tracked signal keys)."""
        a = np.ascontiguousarray(avg_row, np.float32)
        r = np.ascontiguousarray(rel_row, np.float32)
        c = np.ascontiguousarray(candidates, np.int32)
        nsig = C.c_int()
        ntx = self._lib.sst_process_frame(self._h, int(now_ms), a.ctypes.data_as(c_float_p), r.ctypes.data_as(c_float_p),
                                          c.ctypes.data_as(c_int32_p), c.size, self._tx.ctypes.data_as(c_int32_p), self.n,
                                          self._sig.ctypes.data_as(c_int32_p), self.n, C.byref(nsig))
        self.keys = self._sig[:nsig.value].copy()
        return self._tx[:2 * ntx].reshape(-1, 2).copy(), self.keys

    def process_frame_digest(self, now_ms: int, cand_idx, cand_avg, cand_best, watch, peak_idx_row, peak_avg_row):
        """One frame of a digest (include/specscan_track.h): the frame's slices of the candidate lists, the watch list and the
        frame's rows of the peaks. Same return as process_frame; ValueError when a tracked key is missing from ``watch``."""
        ci = np.ascontiguousarray(cand_idx, np.int32)
        ca = np.ascontiguousarray(cand_avg, np.float32)
        cb = np.ascontiguousarray(cand_best, np.int32)
        w = np.ascontiguousarray(watch, np.int32)
        pi = np.ascontiguousarray(peak_idx_row, np.int32)
        pa = np.ascontiguousarray(peak_avg_row, np.float32)
        if not (ci.size == ca.size == cb.size) or not (w.size == pi.size == pa.size):
            raise ValueError("digest arrays of different lengths")
        nsig = C.c_int()
        ntx = self._lib.sst_process_frame_digest(self._h, int(now_ms), ci.ctypes.data_as(c_int32_p), ca.ctypes.data_as(c_float_p),
                                                 cb.ctypes.data_as(c_int32_p), ci.size, w.ctypes.data_as(c_int32_p), w.size,
                                                 pi.ctypes.data_as(c_int32_p), pa.ctypes.data_as(c_float_p), self._tx.ctypes.data_as(c_int32_p),
                                                 self.n, self._sig.ctypes.data_as(c_int32_p), self.n, C.byref(nsig))
        if ntx < 0:
            raise ValueError("a tracked key is missing from the digest's watch list")
        self.keys = self._sig[:nsig.value].copy()
        return self._tx[:2 * ntx].reshape(-1, 2).copy(), self.keys

    def process_batch_digest(self, t_ms, result):
        """A whole batch from ``TrackDigest.digest`` (or any dict with the same arrays): what process_batch returns on the planes."""
        off, watch = result["cand_off"], result["watch"]
        out = []
        for f in range(len(off) - 1):
            a, b = int(off[f]), int(off[f + 1])
            out.append(self.process_frame_digest(t_ms[f], result["cand_idx"][a:b], result["cand_avg"][a:b], result["cand_best"][a:b], watch,
                                                 result["peak_idx"][f], result["peak_avg"][f]))
        return out

    def process_batch(self, t_ms, avg, rel, cand_off, cand_idx):
        out = []
        for f in range(avg.shape[0]):
            out.append(self.process_frame(t_ms[f], avg[f], rel[f], cand_idx[cand_off[f]:cand_off[f + 1]]))
        return out


class StConfig(C.Structure):  # st_config, include/specscan_track.h
    _fields_ = [("abi_version", C.c_uint32), ("group_size", C.c_int32), ("start_level", C.c_float), ("max_watch", C.c_int32), ("cand_cap", C.c_int32)]


class StResult(C.Structure):  # st_result
    _fields_ = [("nframes", C.c_int32), ("ncand", C.c_int32), ("nwatch", C.c_int32), ("cand_best", c_int32_p), ("cand_avg", c_float_p),
                ("watch", c_int32_p), ("peak_idx", c_int32_p), ("peak_avg", c_float_p), ("d2h_bytes", C.c_uint64)]


ST_ABI_VERSION = 1


def bind_track(lib: C.CDLL) -> None:
    lib.st_create.argtypes = [C.c_void_p, C.POINTER(StConfig), C.POINTER(C.c_void_p)]
    lib.st_create.restype = C.c_int
    lib.st_destroy.argtypes = [C.c_void_p]
    lib.st_destroy.restype = None
    lib.st_last_error.argtypes = [C.c_void_p]
    lib.st_last_error.restype = C.c_char_p
    lib.st_reset.argtypes = [C.c_void_p]
    lib.st_reset.restype = C.c_int
    lib.st_digest.argtypes = [C.c_void_p, c_int32_p, c_int32_p, c_int32_p, C.c_int32, C.POINTER(StResult)]
    lib.st_digest.restype = C.c_int


ST_SPARSE_EXPORTS = ("st_create_sparse", "st_sparse_stats")  # include/specscan_track_digest_sparse.h


def bind_track_digest_sparse(lib: C.CDLL) -> None:
    lib.st_create_sparse.argtypes = [C.c_void_p, C.POINTER(StConfig), C.POINTER(C.c_void_p)]
    lib.st_create_sparse.restype = C.c_int
    lib.st_sparse_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.st_sparse_stats.restype = C.c_int


class TrackDigest:
    """One st_ctx bound to a SpectrumEngine created with SS_FLAG_KEEP_PLANES (SpectrumEngine.track_digest). Call ``digest`` once
    after every batch, ``reset`` with the engine's ``reset``.
    ``sparse=True``: st_create_sparse — the engine may lack SS_FLAG_KEEP_PLANES (fused back end, any size)."""

    def __init__(self, engine, group_size: int, start_level: float = 8.0, max_watch: int = 1024, cand_cap: int = 1 << 20, sparse: bool = False):
        from .abi import SpecscanError
        self._err = SpecscanError
        self._engine = engine  # (the scan context must outlive the digest object)
        self._lib = engine._lib
        bind_track(self._lib)
        cfg = StConfig(ST_ABI_VERSION, int(group_size), float(start_level), int(max_watch), int(cand_cap))
        h = C.c_void_p()
        if sparse:
            bind_track_digest_sparse(self._lib)
        st = (self._lib.st_create_sparse if sparse else self._lib.st_create)(engine._h, C.byref(cfg), C.byref(h))
        if st != 0:
            raise SpecscanError(st, (self._lib.st_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._engine, "_h", None):  # (an engine closed first took its stream with it; the object is only freed)
                self._lib.st_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise self._err(st, (self._lib.st_last_error(self._h) or b"").decode())

    def reset(self):
        self._check(self._lib.st_reset(self._h))

    def sparse_stats(self) -> dict:
        """{"tiles_evaluated", "tiles_in_batches"} since the object was made or reset: the tiles the replay inside ``digest`` ran, out
        of the tiles the digested batches have. SpecscanError on an object whose engine keeps its planes (nothing is replayed there)."""
        bind_track_digest_sparse(self._lib)
        ev, tot = C.c_uint64(), C.c_uint64()
        self._check(self._lib.st_sparse_stats(self._h, C.byref(ev), C.byref(tot)))
        return {"tiles_evaluated": int(ev.value), "tiles_in_batches": int(tot.value)}

    def digest(self, cand_off, cand_idx, keys) -> dict:
        """The digest of the engine's last batch as numpy copies: cand_off (clipped to the lists), cand_idx, cand_best, cand_avg,
        watch, peak_idx / peak_avg [nframes, nwatch], d2h_bytes."""
        off = np.ascontiguousarray(cand_off, np.int32)
        idx = np.ascontiguousarray(cand_idx, np.int32)
        k = np.ascontiguousarray(keys, np.int32).reshape(-1)
        r = StResult()
        self._check(self._lib.st_digest(self._h, off.ctypes.data_as(c_int32_p), idx.ctypes.data_as(c_int32_p), k.ctypes.data_as(c_int32_p), k.size,
                                        C.byref(r)))
        take = lambda p, count, dt: np.ctypeslib.as_array(p, shape=(count,)).astype(dt, copy=True) if count else np.zeros(0, dt)  # noqa: E731
        nf, nc, nw = r.nframes, r.ncand, r.nwatch
        return {"nframes": nf, "cand_off": np.minimum(off[:nf + 1], nc).astype(np.int32), "cand_idx": idx[:nc].copy(),
                "cand_best": take(r.cand_best, nc, np.int32), "cand_avg": take(r.cand_avg, nc, np.float32), "watch": take(r.watch, nw, np.int32),
                "peak_idx": take(r.peak_idx, nf * nw, np.int32).reshape(nf, nw), "peak_avg": take(r.peak_avg, nf * nw, np.float32).reshape(nf, nw),
                "d2h_bytes": int(r.d2h_bytes)}


class StfConfig(C.Structure):  # stf_config, include/specscan_track_feed.h
    _fields_ = [("abi_version", C.c_uint32), ("group_size", C.c_int32), ("start_level", C.c_float), ("max_watch", C.c_int32)]


_stf_result = None


def _stf_result_type():
    """stf_result, defined once: every binding of the library and every TrackedFeed share the one ctypes class."""
    global _stf_result
    if _stf_result is not None:
        return _stf_result
    from .abi import SsFeedResult

    class StfResult(C.Structure):  # stf_result
        _fields_ = [("batch", SsFeedResult), ("seq", C.c_uint64), ("keys_seq", C.c_uint64), ("status", C.c_int32), ("ncand", C.c_int32), ("nwatch", C.c_int32),
                    ("cand_best", c_int32_p), ("cand_avg", c_float_p), ("watch", c_int32_p), ("peak_idx", c_int32_p), ("peak_avg", c_float_p),
                    ("d2h_bytes", C.c_uint64)]
    _stf_result = StfResult
    return StfResult


STF_ABI_VERSION = 1
STF_EXPORTS = ("stf_create", "stf_destroy", "stf_last_error", "stf_post_keys", "stf_collect", "stf_reset")


def bind_track_feed(lib: C.CDLL):
    result = _stf_result_type()
    lib.stf_create.argtypes = [C.c_void_p, C.POINTER(StfConfig), C.POINTER(C.c_void_p)]
    lib.stf_create.restype = C.c_int
    lib.stf_destroy.argtypes = [C.c_void_p]
    lib.stf_destroy.restype = None
    lib.stf_last_error.argtypes = [C.c_void_p]
    lib.stf_last_error.restype = C.c_char_p
    lib.stf_post_keys.argtypes = [C.c_void_p, C.c_uint64, c_int32_p, C.c_int32]
    lib.stf_post_keys.restype = C.c_int
    lib.stf_collect.argtypes = [C.c_void_p, C.POINTER(result)]
    lib.stf_collect.restype = C.c_int
    lib.stf_reset.argtypes = [C.c_void_p]
    lib.stf_reset.restype = C.c_int
    return result


STF_SPARSE_EXPORTS = ("stf_create_sparse", "stf_sparse_stats")  # include/specscan_track_sparse.h


def bind_track_sparse(lib: C.CDLL) -> None:
    lib.stf_create_sparse.argtypes = [C.c_void_p, C.POINTER(StfConfig), C.POINTER(C.c_void_p)]
    lib.stf_create_sparse.restype = C.c_int
    lib.stf_sparse_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.stf_sparse_stats.restype = C.c_int


class TrackedFeed:
    """One stf_ctx bound to a Feed of an engine created with SS_FLAG_KEEP_PLANES (Feed.track): every batch submitted through the
    feed is digested in the stream behind its chain. ``collect`` replaces the feed's own; ``post_keys(seq, tracker.keys)`` after
    every collect keeps the watch lists short; ``reset`` goes with the engine's ``reset`` (feed drained first).
    ``sparse=True``: stf_create_sparse — the engine may lack SS_FLAG_KEEP_PLANES (fused back end, up to 32768 points).
    ``sparse=True, ring=True``: stf_create_ring (include/specscan_track_feed_ring.h) — ... at any size: from 65536 points up the
    feed's batches take the forms that keep no dB plane, and are digested from the rows they leave in the averager ring's buffer."""

    def __init__(self, feed, group_size: int, start_level: float = 8.0, max_watch: int = 1024, sparse: bool = False, ring: bool = False):
        from .abi import SpecscanError
        self._err = SpecscanError
        self._feed = feed  # (the feed and its engine must outlive the object; a feed closed first leaves it only close())
        self._lib = feed._lib
        self._result = bind_track_feed(self._lib)
        cfg = StfConfig(STF_ABI_VERSION, int(group_size), float(start_level), int(max_watch))
        h = C.c_void_p()
        if ring and not sparse:
            raise ValueError("ring=True goes with sparse=True (stf_create_ring is stf_create_sparse at every size)")
        if sparse:
            bind_track_sparse(self._lib)
        if ring:
            from .abi import bind_track_feed_ring
            bind_track_feed_ring(self._lib)
        create = self._lib.stf_create_ring if ring else self._lib.stf_create_sparse if sparse else self._lib.stf_create
        st = create(feed._h, C.byref(cfg), C.byref(h))
        if st != 0:
            raise SpecscanError(st, (self._lib.stf_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self._feed._e, "_h", None):  # (an engine closed first took its stream and its lock with it)
                self._lib.stf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise self._err(st, (self._lib.stf_last_error(self._h) or b"").decode())

    def reset(self):
        self._check(self._lib.stf_reset(self._h))

    def sparse_stats(self) -> dict:
        """{"tiles_evaluated", "tiles_in_batches"} since the object was made or reset: the tiles the replay behind the batches ran, out
        of the tiles those batches have. SpecscanError on an object whose engine keeps its planes (nothing is replayed there)."""
        bind_track_sparse(self._lib)
        ev, tot = C.c_uint64(), C.c_uint64()
        self._check(self._lib.stf_sparse_stats(self._h, C.byref(ev), C.byref(tot)))
        return {"tiles_evaluated": int(ev.value), "tiles_in_batches": int(tot.value)}

    def post_keys(self, seq: int, keys):
        """The tracker's keys after it has processed batch ``seq`` (SignalTracker.keys): batches submitted from now on watch them."""
        k = np.ascontiguousarray(keys, np.int32).reshape(-1)
        self._check(self._lib.stf_post_keys(self._h, int(seq), k.ctypes.data_as(c_int32_p), k.size))

    def collect(self) -> dict:
        """The oldest pending batch with its digest, as numpy copies: the feed's nframes / status / tag (/ psd), seq, keys_seq,
        digest_status (0, or SS_ERR_INVALID: more than max_watch watch keys — watch and peaks are empty then, nwatch is the true count)
        and the arrays of ``TrackDigest.digest``: cand_off (clipped to the lists; cand_total is what the batch found), cand_idx, cand_best,
        cand_avg (gathered from the avg plane; feed_cand_avg is the feed's own list), watch, peak_idx / peak_avg [nframes, nwatch]."""
        r = self._result()
        self._check(self._lib.stf_collect(self._h, C.byref(r)))
        take = lambda p, count, dt: np.ctypeslib.as_array(p, shape=(count,)).astype(dt, copy=True) if count else np.zeros(0, dt)  # noqa: E731
        nf, nc = r.batch.nframes, r.ncand
        nw = r.nwatch if r.status == 0 else 0
        off = take(r.batch.cand_off, nf + 1, np.int32)
        out = {"nframes": nf, "status": r.batch.status, "tag": r.batch.user_tag, "seq": int(r.seq), "keys_seq": int(r.keys_seq), "digest_status": r.status,
               "nwatch": r.nwatch, "cand_total": int(off[nf]), "cand_off": np.minimum(off, nc).astype(np.int32), "cand_idx": take(r.batch.cand_idx, nc, np.int32),
               "feed_cand_avg": take(r.batch.cand_avg, nc, np.float32), "cand_best": take(r.cand_best, nc, np.int32), "cand_avg": take(r.cand_avg, nc, np.float32),
               "watch": take(r.watch, nw, np.int32), "peak_idx": take(r.peak_idx, nf * nw, np.int32).reshape(nf, nw),
               "peak_avg": take(r.peak_avg, nf * nw, np.float32).reshape(nf, nw), "d2h_bytes": int(r.d2h_bytes)}
        if r.batch.psd_db:
            out["psd"] = np.ctypeslib.as_array(r.batch.psd_db, shape=(nf, self._feed._e.n)).copy()
        return out
