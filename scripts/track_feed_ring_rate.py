"""Batches per second through a depth-3 feed at the reference's own transform sizes, three routes, one process, the same stream:

  (u) untracked:  ss_feed_acquire / ss_feed_submit / ss_feed_collect, no tracker. A batch goes through an untracked feed as an ordinary
                  call: every batch keeps its dB plane (the four-step form at 131072 points, the two-launch chain at 262144).
  (p) planes:     stf_create on a SS_FLAG_KEEP_PLANES context: full dB and avg planes per batch, no culling, no no-plane form.
  (r) ring:       stf_create_ring (include/specscan_track_feed_ring.h) on a context without the flag: from the second batch on the
                  batches take the forms that keep no dB plane (counted outside the clock: ss_read_window(SS_PLANE_PSD) refuses behind such a
                  batch; every route's last batch is asked once more when the run is over).

at 131072 points, CS8, 128-frame batches (32 MiB of input per batch) and at 262144 points, CF32, 32-frame batches (64 MiB per batch).
A turn is scripts/track_digest_rate.py's FeedRoute turn: fill a pinned slot from one of --distinct host batches, submit it, and — from
the third turn on — collect the oldest batch, run the host tracker over its frames and post the keys: two batches in flight. The
routes alternate turn by turn, so whatever else the host does meets all three; wall clock per turn, median over --reps turns after
--warm, the whole measurement --runs times (the medians of the runs' medians are reported, and every run's). Every batch's input
comes over from host memory and the three contexts' work buffers, planes and slots together exceed the 256 MiB Infinity Cache
several times (the script prints the input bytes per turn), so nothing a turn reads is left in the cache by the turn before.

Also reported: ss_get_stats tile counters per route, the ring route's stf_sparse_stats, transmissions per route (u has none), and
`r_minus_u_ms_median` / `p_minus_r_ms_median`, the medians of the turn-by-turn differences. Prints one JSON line per shape.

    python scripts/track_feed_ring_rate.py [--reps 15] [--warm 4] [--runs 3] [--shapes 131072,262144] [--distinct 3] [--route upr]

The digest's own cost is a device figure, and the turns above cannot give it (the untracked feed runs another scan form, and a tracked
turn holds the host tracker's loop). --route r runs the ring route alone: the form to put behind `rocprofv3 --kernel-trace --stats --`,
a run of its own. --kernel-stats FILE then reads that run's *_kernel_stats.csv and prints one JSON line: the device time of the
digest's kernels (k_feed_*, k_ring_*, k_digest_tiles, k_watch_tiles, k_best_blocked, k_save_tail) and of the scan's (every other
kernel of the library) summed over the run, and the first as a share of the second — the scan being the one the same batches run
with no tracker, since the digest changes no launch of it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtl_sdr_scanner_cpp_amd as pkg  # noqa: E402
from rtl_sdr_scanner_cpp_amd import abi, tracker  # noqa: E402
from track_digest_rate import FeedRoute  # noqa: E402

SHAPES = {131072: (abi.SS_FMT_CS8, 128, "frames_cs8"), 262144: (abi.SS_FMT_CF32, 32, "frames_cf32")}
LABELS = {"u": "untracked", "p": "planes", "r": "ring"}


class RingRateRoute(FeedRoute):
    """FeedRoute (scripts/track_digest_rate.py: the turn, the tracker's loop, drain, tile_stats) on the three objects of this script."""

    def __init__(self, name, n, fs, batch, g, in_format):
        self.n, self.batch, self.name = n, batch, name
        self.sparse = name == "r"  # (FeedRoute.tile_stats: report stf_sparse_stats)
        self.eng = pkg.SpectrumEngine(fs, 145_000_000, fft_size=n, decim=1, max_batch=batch, learn_ms=280, in_format=in_format,
                                      flags=abi.SS_FLAG_KEEP_PLANES if name == "p" else 0)
        self.trk = tracker.SignalTracker(n, fs, group_size=g, start_level=8.0, min_time_ms=200, timeout_ms=400)
        self.feed = self.eng.feed(depth=3, cand_cap=batch * 1024)
        self.stf = None if name == "u" else self.feed.track(g, max_watch=4096, sparse=name == "r", ring=name == "r")
        self.res = self.stf._result() if self.stf is not None else abi.SsFeedResult()
        self.tx = np.empty(2 * n, np.int32)
        self.sig = np.empty(n, np.int32)
        import ctypes as C
        self.nsig = C.c_int()
        self.times, self.d2h, self.total = [], 0, 0
        self.turns = self.no_plane = 0

    def check_form(self):
        """Outside the clock: did the batch submitted last keep a dB plane? (ss_read_window speaks of the batch submitted last.)"""
        self.turns += 1
        try:
            self.eng.read_window(abi.SS_PLANE_PSD, 0, 0, 64)
        except abi.SpecscanError as e:
            assert e.status == abi.SS_ERR_INVALID, e
            self.no_plane += 1


DIGEST_KERNELS = ("k_feed_", "k_ring_", "k_digest_tiles", "k_digest_cols", "k_watch_tiles", "k_best_blocked", "k_save_tail")


def kernel_stats(path):
    """One JSON line from a rocprofv3 --kernel-trace --stats table (Name, Calls, TotalDurationNs, ...)."""
    import csv
    sums = {"digest": 0, "scan": 0, "other": 0}
    rows = {"digest": {}, "scan": {}, "other": {}}
    for row in csv.DictReader(open(path)):
        name, ns, calls = row["Name"], int(float(row["TotalDurationNs"])), int(row["Calls"])
        kind = "digest" if any(k in name for k in DIGEST_KERNELS) else "scan" if "ss::" in name or name.startswith("k_") or " k_" in name else "other"
        sums[kind] += ns
        short = name.split("(")[0].replace("void ", "")
        rows[kind][short] = {"calls": calls, "us": round(ns / 1e3, 1)}
    out = {"file": os.path.basename(path), "digest_us": round(sums["digest"] / 1e3, 1), "scan_us": round(sums["scan"] / 1e3, 1),
           "other_us": round(sums["other"] / 1e3, 1), "digest_over_scan": round(sums["digest"] / max(1, sums["scan"]), 4), "kernels": rows}
    print(json.dumps(out), flush=True)


def shape(n, reps, warm, runs, distinct, routes="upr"):
    in_format, batch, frames = SHAPES[n]
    fs, g = n * 250, 128
    band = pkg.synth.SyntheticBand(n, seed=0, on_frame=batch // 8 + 30, off_frame=5 * max(batch, 64) // 8 + 30, period=max(batch, 64) + 60)
    batches = [getattr(band, frames)(batch) for _ in range(distinct)]
    out = {"fft_size": n, "batch": batch, "in_format": frames[7:], "group_size": g, "reps": reps, "warm": warm, "runs": runs,
           "input_bytes_per_turn": int(batches[0].nbytes), "distinct_host_batches": distinct}
    labels = {name: LABELS[name] for name in routes}
    per_run = {name: [] for name in labels}
    diffs = {"r_minus_u": [], "p_minus_r": []} if len(labels) == 3 else {}
    for run in range(runs):
        made = {name: RingRateRoute(name, n, fs, batch, g, in_format) for name in labels}
        times = {name: [] for name in labels}
        for k in range(warm + reps):
            t = (1_000 + 40 * (k * batch + np.arange(batch))).astype(np.int64)
            for name, route in made.items():
                dt, _ = route.run(batches[k % distinct], t)
                if name == "r":  # (a refusal touches no stream; a served read waits for it, which would drain the other routes' pipelines)
                    route.check_form()
                if k >= warm:
                    times[name].append(dt)
        for name, route in made.items():
            per_run[name].append(round(1e3 * statistics.median(times[name]), 3))
            route.drain()
        if diffs:
            diffs["r_minus_u"].append(round(1e3 * statistics.median(p - q for p, q in zip(times["r"], times["u"])), 3))
            diffs["p_minus_r"].append(round(1e3 * statistics.median(p - q for p, q in zip(times["p"], times["r"])), 3))
        if run == runs - 1:
            for name, route in made.items():
                label = LABELS[name]
                out[f"{label}_tiles"] = route.tile_stats()
                if name == "r":
                    out["ring_batches_without_db_plane"] = [route.no_plane, route.turns]
                before = route.no_plane
                route.check_form()  # (drained: the last batch)
                out[f"{label}_last_batch_kept_db_plane"] = route.no_plane == before
                if name != "u":
                    out[f"{label}_transmissions"] = route.total
                    out[f"{label}_d2h_bytes_last"] = route.d2h
        for route in made.values():
            if route.stf is not None:
                route.stf.close()
            route.feed.close()
            route.eng.close()
    for name, label in labels.items():
        out[f"{label}_ms_median"] = statistics.median(per_run[name])
        out[f"{label}_ms_runs"] = per_run[name]
        out[f"{label}_batches_per_s"] = round(1e3 / out[f"{label}_ms_median"], 1)
    for key, vals in diffs.items():
        out[f"{key}_ms_median"] = statistics.median(vals)
        out[f"{key}_ms_runs"] = vals
    if diffs:
        out["ring_between_the_other_two"] = out["untracked_ms_median"] <= out["ring_ms_median"] <= out["planes_ms_median"]
        out["ring_minus_untracked_over_untracked"] = round(out["r_minus_u_ms_median"] / out["untracked_ms_median"], 4)
        out["same_transmission_count_p_r"] = out["planes_transmissions"] == out["ring_transmissions"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=3)
    ap.add_argument("--shapes", default="131072,262144")
    ap.add_argument("--route", default="upr", help="upr (all three, alternating), or one letter: that route alone")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of a --route r run: print the digest's share")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    if args.route != "upr" and args.route not in ("u", "p", "r"):
        ap.error("--route: upr, u, p or r")
    for n in (int(s) for s in args.shapes.split(",")):
        if n not in SHAPES:
            ap.error("--shapes: 131072 and / or 262144")
        shape(n, args.reps, args.warm, args.runs, args.distinct, args.route)


if __name__ == "__main__":
    main()
