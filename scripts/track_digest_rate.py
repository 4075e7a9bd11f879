"""Transmissions per batch, three routes, one process, the same synthetic stream (synth.SyntheticBand):

  (a) planes:  ss_process with rel_db and avg_db, then sst_process_frame per frame          — what enableTracker does
  (b) digest:  ss_process without them (SS_FLAG_KEEP_PLANES), st_digest, then
               sst_process_frame_digest per frame                                           — what enableDeviceTracker does
  (c) tracked feed: ss_feed_acquire / ss_feed_submit with an stf_ctx on the feed (depth 3), stf_collect of the
               batch submitted two turns earlier, sst_process_frame_digest per frame, stf_post_keys — what specscan_replay --track does
  (d) tracked feed, sparse: route (c) on an engine WITHOUT SS_FLAG_KEEP_PLANES, stf_create_sparse (include/specscan_track_sparse.h)
               — what specscan_replay --track-sparse does
  (s) digest, sparse: route (b) on an engine WITHOUT SS_FLAG_KEEP_PLANES, st_create_sparse (include/specscan_track_digest_sparse.h)
               — what enableSparseDeviceTracker does; reports st_sparse_stats (tiles_evaluated / tiles_in_batches) as well
  (u) untracked feed: route (c)'s turns with no tracker at all (ss_feed_collect, no per-frame loop): the scan alone, the floor of c and d

at 8192 points in 1024-frame batches and at 2^20 points in 16-frame batches; --shapes 65536 is 65536 points in 128-frame batches, where
routes (b) and (s) are DEVICE routes on CS8 input: ss_process cannot take a form that writes no dB plane (it runs its batch with no
overlap allowed), so there the frames are resident on the device before the clock starts, the call is ss_process_device with no plane
pointer at all and device candidate lists, then ss_sync, the lists' copy to the host, st_digest and the tracker's frames. Route (s) then
takes the radix-8 fold, and the script checks it after every batch but the learning one, outside the clock: ss_read_window(SS_PLANE_PSD)
must refuse on (s) and serve on (b), whose context keeps planes and so runs the four-step form. The other routes get CF32 frames from
host memory at that shape as at the others. Wall clock around the whole batch (the call, the digest, the tracker's frames), median of
--reps repetitions after a warm-up; routes (b) and (s) also report the call and st_digest on their own (*_scan_ms_median,
*_st_digest_ms_median). All routes go through the C ABI with buffers allocated once, and the per-frame loop is the
same Python loop in all. Route (c)'s turn is: fill a pinned slot, submit it, and — from the third turn on — collect, track and post the oldest batch, so its time per turn is its time per batch with two batches in flight (what it
leaves in flight when its turn ends is a millisecond or two of device work that finishes while its own tracker loop still runs).
Routes on a feed also report what their scan culled (ss_get_stats: tiles_culled / tiles_tested) and, route (d), what its replay ran
(stf_sparse_stats: tiles_evaluated / tiles_in_batches); `d_minus_c_ms_median` is the median of the turn-by-turn differences of the two
interleaved routes. Prints one JSON line per shape. With --route b (or c) only that route runs: the form to put behind
`rocprofv3 --kernel-trace --stats --` for the device times of the digest's kernels.

    python scripts/track_digest_rate.py [--reps 7] [--warm 3] [--route abc|ab|a|b|s|bs|c|d|ucd|...] [--shapes 8192,1048576] [--group G]

--group G replaces the shapes' group_size (128 and 547). --level L: start_level of the engines and of the trackers (default: the
reference's 8 dB; the script's streams learn their ceiling from 7 frames, which leaves the noise tiles' culling bounds above 8 dB —
nothing is culled there on any route —, at 15 dB the noise tiles are).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtl_sdr_scanner_cpp_amd as pkg  # noqa: E402
from rtl_sdr_scanner_cpp_amd import abi, tracker  # noqa: E402

f32p, i32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def at(a, offset_elems, typ):
    return C.cast(a.ctypes.data + offset_elems * a.itemsize, typ)


class Route:
    def __init__(self, n, fs, batch, g, digest: bool, level=8.0, sparse=False, in_format=abi.SS_FMT_CF32, device=False):
        self.n, self.batch, self.digest, self.sparse, self.device, self.in_format = n, batch, digest, sparse, device, in_format
        # (learn_frames: device calls carry no clocks; seven frames either way)
        self.eng = pkg.SpectrumEngine(fs, 145_000_000, fft_size=n, decim=1, max_batch=batch, learn_ms=280, learn_frames=7, start_level=level, in_format=in_format,
                                      flags=abi.SS_FLAG_KEEP_PLANES if digest and not sparse else 0)
        self.trk = tracker.SignalTracker(n, fs, group_size=g, start_level=level, min_time_ms=200, timeout_ms=400)
        self.cap = batch * 1024
        self.psd = None if device else np.empty((batch, n), np.float32)
        self.rel = None if digest else np.empty((batch, n), np.float32)
        self.avg = None if digest else np.empty((batch, n), np.float32)
        self.off = np.zeros(batch + 1, np.int32)
        self.idx = np.empty(self.cap, np.int32)
        self.cav = np.empty(self.cap, np.float32)
        self.tx = np.empty(2 * n, np.int32)
        self.sig = np.empty(n, np.int32)
        self.nsig = C.c_int()
        self.dig = self.eng.track_digest(g, max_watch=4096, cand_cap=self.cap, sparse=sparse) if digest else None
        self.res = tracker.StResult()
        self.keys = np.zeros(n, np.int32)
        self.nkeys = 0
        self.d2h = 0
        self.calls = 0
        self.parts = []  # per batch: (seconds of the scan call, seconds of st_digest) — the rest of a batch's time is the tracker's loop
        if device:
            import torch
            assert digest, "the device routes are the digest's"
            dev = torch.device("cuda", 0)
            self.d_off = torch.zeros(batch + 1, dtype=torch.int32, device=dev)
            self.d_idx = torch.empty(self.cap, dtype=torch.int32, device=dev)
            self.d_cav = torch.empty(self.cap, dtype=torch.float32, device=dev)
            self.h_off, self.h_idx = torch.from_numpy(self.off), torch.from_numpy(self.idx)
            torch.cuda.synchronize()  # (torch's fills run on torch's stream, the library writes from its own)

    def check_form(self):
        """A device route, outside the clock: the sparse route's call left no dB plane (a no-plane form ran), the planes route's did."""
        self.calls += 1
        if not self.device or self.calls == 1:  # (the first batch holds the learning frames: the four-step form on every route)
            return
        if self.sparse:
            try:
                self.eng.read_window(abi.SS_PLANE_PSD, 0, 0, 64)
            except abi.SpecscanError as e:
                assert e.status == abi.SS_ERR_INVALID, e
            else:
                raise AssertionError("route (s): the call left a dB plane, so no no-plane form ran")
        else:
            self.eng.read_window(abi.SS_PLANE_PSD, 0, 0, 64)

    def run(self, iq, t):
        """One batch; returns (seconds, transmissions). iq: a numpy array, or for a device route a tensor on the device."""
        lib, hl, n, nf = self.eng._lib, self.trk._lib, self.n, self.batch
        seen = 0
        t0 = time.perf_counter()
        if self.device:
            self.eng.process_device(iq, nf, cand_off=self.d_off, cand_idx=self.d_idx, cand_avg=self.d_cav)
            self.eng.sync()
            self.h_off.copy_(self.d_off)
            ncand = min(int(self.off[nf]), self.cap)
            self.h_idx[:ncand].copy_(self.d_idx[:ncand])
        else:
            st = lib.ss_process(self.eng._h, iq.ctypes.data_as(C.c_void_p), nf, t.ctypes.data_as(i64p), at(self.psd, 0, f32p),
                                None if self.digest else at(self.rel, 0, f32p), None if self.digest else at(self.avg, 0, f32p), at(self.off, 0, i32p),
                                at(self.idx, 0, i32p), at(self.cav, 0, f32p), self.cap)
            assert st == 0, (st, lib.ss_last_error(self.eng._h))
        t1 = time.perf_counter()
        off = self.off.tolist()
        if self.digest:
            st = lib.st_digest(self.dig._h, at(self.off, 0, i32p), at(self.idx, 0, i32p), at(self.keys, 0, i32p), self.nkeys, C.byref(self.res))
            assert st == 0, (st, lib.st_last_error(self.dig._h))
            self.parts.append((t1 - t0, time.perf_counter() - t1))  # the call up to its lists on the host; st_digest
            r = self.res
            best, cavg, pidx, pavg = (C.addressof(p.contents) if p else 0 for p in (r.cand_best, r.cand_avg, r.peak_idx, r.peak_avg))
            nw = r.nwatch
            self.d2h = int(r.d2h_bytes)
            for f in range(nf):
                a, b = off[f], off[f + 1]
                seen += hl.sst_process_frame_digest(self.trk._h, int(t[f]), at(self.idx, a, i32p), C.cast(cavg + 4 * a, f32p), C.cast(best + 4 * a, i32p), b - a,
                                                    r.watch, nw, C.cast(pidx + 4 * f * nw, i32p), C.cast(pavg + 4 * f * nw, f32p), at(self.tx, 0, i32p), n,
                                                    at(self.sig, 0, i32p), n, C.byref(self.nsig))
            self.nkeys = self.nsig.value
            self.keys[:self.nkeys] = self.sig[:self.nkeys]
        else:
            for f in range(nf):
                a, b = off[f], off[f + 1]
                seen += hl.sst_process_frame(self.trk._h, int(t[f]), at(self.avg, f * n, f32p), at(self.rel, f * n, f32p), at(self.idx, a, i32p), b - a,
                                             at(self.tx, 0, i32p), n, at(self.sig, 0, i32p), n, C.byref(self.nsig))
        dt = time.perf_counter() - t0
        self.check_form()
        return dt, seen


class FeedRoute:
    """Routes (c), (d), (u): the feed, two batches in flight — tracked on kept planes, tracked sparse, or not tracked."""

    def __init__(self, n, fs, batch, g, sparse=False, tracked=True, level=8.0):
        self.n, self.batch, self.sparse = n, batch, sparse
        self.eng = pkg.SpectrumEngine(fs, 145_000_000, fft_size=n, decim=1, max_batch=batch, learn_ms=280, start_level=level,
                                      flags=abi.SS_FLAG_KEEP_PLANES if tracked and not sparse else 0)
        self.trk = tracker.SignalTracker(n, fs, group_size=g, start_level=level, min_time_ms=200, timeout_ms=400)
        self.feed = self.eng.feed(depth=3, cand_cap=batch * 1024)
        self.stf = self.feed.track(g, max_watch=4096, sparse=sparse) if tracked else None
        self.res = self.stf._result() if tracked else abi.SsFeedResult()
        self.tx = np.empty(2 * n, np.int32)
        self.sig = np.empty(n, np.int32)
        self.nsig = C.c_int()
        self.times = []  # t_ms of the batches in flight
        self.d2h = 0
        self.total = 0  # transmissions over every batch collected, warm-up included

    def collect(self):
        lib, hl, n = self.eng._lib, self.trk._lib, self.n
        if self.stf is None:
            st = lib.ss_feed_collect(self.feed._h, C.byref(self.res))
            assert st == 0, (st, lib.ss_last_error(self.eng._h))
            self.times.pop(0)
            return 0
        st = lib.stf_collect(self.stf._h, C.byref(self.res))
        assert st == 0, (st, lib.stf_last_error(self.stf._h))
        r, t = self.res, self.times.pop(0)
        assert r.status == 0, r.nwatch
        off = np.ctypeslib.as_array(r.batch.cand_off, shape=(r.batch.nframes + 1,)).tolist()
        idx, best, cavg, pidx, pavg = (C.addressof(p.contents) if p else 0 for p in (r.batch.cand_idx, r.cand_best, r.cand_avg, r.peak_idx, r.peak_avg))
        nw, nc, seen = r.nwatch, r.ncand, 0
        self.d2h = int(r.d2h_bytes)
        for f in range(r.batch.nframes):
            a, b = min(off[f], nc), min(off[f + 1], nc)
            seen += hl.sst_process_frame_digest(self.trk._h, int(t[f]), C.cast(idx + 4 * a, i32p), C.cast(cavg + 4 * a, f32p), C.cast(best + 4 * a, i32p), b - a,
                                                r.watch, nw, C.cast(pidx + 4 * f * nw, i32p), C.cast(pavg + 4 * f * nw, f32p), at(self.tx, 0, i32p), n,
                                                at(self.sig, 0, i32p), n, C.byref(self.nsig))
        st = lib.stf_post_keys(self.stf._h, r.seq, at(self.sig, 0, i32p), self.nsig.value)
        assert st == 0, (st, lib.stf_last_error(self.stf._h))
        self.total += seen
        return seen

    def run(self, iq, t):
        t0 = time.perf_counter()
        buf = self.feed.acquire()
        np.copyto(buf[:self.batch], iq)
        self.feed.submit(self.batch, t_ms=t)
        self.times.append(t)
        seen = self.collect() if len(self.times) > 2 else 0
        return time.perf_counter() - t0, seen

    def drain(self):
        seen = 0
        while self.times:
            seen += self.collect()
        return seen


    def tile_stats(self):
        self.eng.sync()
        s = self.eng.stats()
        out = {"tiles_total": s["tiles_total"], "tiles_tested": s["tiles_tested"], "tiles_culled": s["tiles_culled"],
               "culled_over_tested": round(s["tiles_culled"] / s["tiles_tested"], 4) if s["tiles_tested"] else None}
        if self.sparse:
            r = self.stf.sparse_stats()
            out.update(r, evaluated_over_in_batches=round(r["tiles_evaluated"] / max(1, r["tiles_in_batches"]), 4))
        return out


LABELS = {"a": "planes", "b": "digest", "s": "digest_sparse", "c": "feed", "d": "feed_sparse", "u": "feed_untracked"}


def make_route(name, n, fs, batch, g, level):
    if name in "cdu":
        return FeedRoute(n, fs, batch, g, sparse=name == "d", tracked=name != "u", level=level)
    device = n == 65536 and name in "bs"  # CS8 frames resident on the device, so that (s) takes the radix-8 fold
    return Route(n, fs, batch, g, digest=name in "bs", level=level, sparse=name == "s", in_format=abi.SS_FMT_CS8 if device else abi.SS_FMT_CF32, device=device)


def shape(n, batch, g, reps, routes, warm=3, distinct=4, level=8.0):
    fs = 2_048_000 if n == 8192 else n * 250
    out = {"fft_size": n, "batch": batch, "group_size": g, "start_level": level, "reps": reps}
    if n == 65536 and set(routes) & set("bs"):  # torch initialises its HIP context before libspecscan.so creates streams, so that both see the device
        import torch
        torch.cuda.init()
    made = {name: make_route(name, n, fs, batch, g, level) for name in routes}

    def frames_for(device):  # the same stream in the format and the place each kind of route reads it from
        band = pkg.synth.SyntheticBand(n, seed=0, on_frame=batch // 8 + 30, off_frame=5 * max(batch, 64) // 8 + 30, period=max(batch, 64) + 60)
        if not device:
            return [band.frames_cf32(batch) for _ in range(distinct)]
        import torch
        return [torch.from_numpy(band.frames_cs8(batch)).to(torch.device("cuda", 0)) for _ in range(distinct)]

    batches = {device: frames_for(device) for device in {getattr(r, "device", False) for r in made.values()}}
    if True in batches:
        import torch
        torch.cuda.synchronize()
        out["device_routes"] = sorted(name for name, r in made.items() if getattr(r, "device", False))
    times = {name: [] for name in routes}
    seen = {name: 0 for name in routes}
    for k in range(warm + reps):  # the routes alternate batch by batch: whatever else the host does meets both
        t = (1_000 + 40 * (k * batch + np.arange(batch))).astype(np.int64)
        for name, route in made.items():
            dt, tx = route.run(batches[getattr(route, "device", False)][k % distinct], t)
            if k >= warm:
                times[name].append(dt)
                seen[name] += tx
    for name, route in made.items():
        label = LABELS[name]
        out[f"{label}_ms_median"] = round(1e3 * statistics.median(times[name]), 3)
        out[f"{label}_ms_all"] = [round(1e3 * x, 3) for x in times[name]]
        out[f"{label}_transmissions"] = seen[name]
        if name == "b":
            out["digest_d2h_bytes_last"] = route.d2h
            out["planes_d2h_bytes"] = 8 * n * batch
        if name in "bs":  # the two parts of the batch's time that the routes differ in
            out[f"{label}_scan_ms_median"] = round(1e3 * statistics.median(p[0] for p in route.parts[warm:]), 3)
            out[f"{label}_st_digest_ms_median"] = round(1e3 * statistics.median(p[1] for p in route.parts[warm:]), 3)
        if name == "s":
            r = route.dig.sparse_stats()
            out["digest_sparse_tiles"] = dict(r, evaluated_over_in_batches=round(r["tiles_evaluated"] / max(1, r["tiles_in_batches"]), 4))
    for name in "cdu":  # (their transmissions lag two batches behind the other routes')
        if name in made:
            label = LABELS[name]
            out[f"{label}_d2h_bytes_last"] = made[name].d2h
            made[name].drain()
            out[f"{label}_transmissions_warm_up_included"] = made[name].total
            out[f"{label}_tiles"] = made[name].tile_stats()
    for x, y in (("d", "c"), ("c", "u"), ("d", "u")):  # paired: the routes alternate turn by turn
        if x in made and y in made:
            out[f"{x}_minus_{y}_ms_median"] = round(1e3 * statistics.median(p - q for p, q in zip(times[x], times[y])), 3)
    if "c" in made and "d" in made:
        out["same_transmission_count_c_d"] = made["c"].total == made["d"].total
        out["feed_sparse_over_feed"] = round(out["feed_sparse_ms_median"] / out["feed_ms_median"], 4)
    if "b" in made and "c" in made:
        out["feed_over_digest"] = round(out["feed_ms_median"] / out["digest_ms_median"], 4)
    if "b" in made and "s" in made:
        out["same_transmission_count_b_s"] = seen["b"] == seen["s"]
        out["digest_sparse_over_digest"] = round(out["digest_sparse_ms_median"] / out["digest_ms_median"], 4)
        out["s_minus_b_ms_median"] = round(1e3 * statistics.median(p - q for p, q in zip(times["s"], times["b"])), 3)
    if "a" in made and "b" in made:
        out["same_transmission_count"] = seen["a"] == seen["b"]  # (tests/test_gpu_track_digest.py holds the two routes to each other frame by frame)
        out["digest_over_planes"] = round(out["digest_ms_median"] / out["planes_ms_median"], 4)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--route", default="ab", help="any of a, b, s, c, d, u, in the order they are to alternate")
    ap.add_argument("--shapes", default="8192,1048576")
    ap.add_argument("--group", type=int, default=None)
    ap.add_argument("--level", type=float, default=8.0)
    args = ap.parse_args()
    for n in (int(s) for s in args.shapes.split(",")):
        g = args.group if args.group is not None else 128 if n == 8192 else 547
        if not args.route or set(args.route) - set("abscdu") or ("d" in args.route and n > 32768):
            ap.error("--route: letters of abscdu (d: up to 32768 points)")
        shape(n, 1024 if n == 8192 else 128 if n == 65536 else 16, g, args.reps, list(dict.fromkeys(args.route)), warm=args.warm, level=args.level)


if __name__ == "__main__":
    main()
