"""Batches per second through a depth-3 feed that tracks AND delivers spectrogram rows, at the reference's own transform sizes: three
routes, one process, the same stream (after scripts/track_feed_ring_rate.py):

  (a) planes:  SS_FLAG_SPECTROGRAM, sgf_create, a ring tracker. The flag makes every batch keep its dB plane: the tracker digests
               planes, the rows kernel reads the plane. What a deployment that tracks and publishes the waterfall ran before
               sgf_create_ring.
  (b) ring:    no flag, sgf_create_ring (include/specscan_spectrogram_feed_ring.h), a ring tracker: from the second batch on the batches
               take the forms that keep no dB plane, and the rows are formed from the averager ring's buffer.
  (c) floor:   route (b) without the spectrogram object.

at 65536 points CS8 x 128 frames, 131072 points CS8 x 64 frames and 262144 points CF32 x 32 frames per batch. A turn fills a pinned
slot from one of --distinct host batches, submits it with the stream's own clock (1000 N / fs ms a frame: 4 ms, so a row closes every
250 frames) and — from the third turn on — collects the oldest batch, reads its rows and posts an empty key list: two batches in
flight. No host tracker runs in the turn: it would be the same work on every route. The routes alternate turn by turn; wall clock per
turn, median over --reps turns after --warm, the whole measurement --runs times. Reported: every run's median and their median per
route, the medians of the turn-by-turn differences b - a and b - c with the spread of b - a over the runs, the rows delivered, how many
of (b)'s batches kept no plane (asked outside the clock), and the tile counters. One JSON line per shape.

    python scripts/spectrogram_feed_ring_rate.py [--reps 12] [--warm 4] [--runs 8] [--shapes 65536,131072,262144] [--route abc] [--out DIR]

The rows kernel's own time is a device figure: --route b runs route (b) alone, the form to put behind `rocprofv3 --kernel-trace
--stats --` in a run of its own; --kernel-stats FILE reads that run's *_results.db (every launch) or *_kernel_stats.csv (totals) and
prints the device time of k_spec_rows / k_spec_rows_ring per launch next to the time of all kernels.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtl_sdr_scanner_cpp_amd as pkg  # noqa: E402
from rtl_sdr_scanner_cpp_amd import abi  # noqa: E402

SHAPES = {65536: (abi.SS_FMT_CS8, 128, "frames_cs8"), 131072: (abi.SS_FMT_CS8, 64, "frames_cs8"), 262144: (abi.SS_FMT_CF32, 32, "frames_cf32")}
LABELS = {"a": "planes", "b": "ring", "c": "floor"}


class Route:
    def __init__(self, name, n, fs, batch, in_format, period_ms):
        self.name, self.n, self.batch = name, n, batch
        self.eng = pkg.SpectrumEngine(fs, 145_000_000, fft_size=n, decim=1, max_batch=batch, learn_ms=int(7 * period_ms), in_format=in_format,
                                      flags=abi.SS_FLAG_SPECTROGRAM if name == "a" else 0)
        self.feed = self.eng.feed(depth=3, cand_cap=batch * 1024)
        self.stf = self.feed.track(128, max_watch=4096, sparse=True, ring=True)
        self.sgf = None if name == "c" else self.feed.spectrogram(max_rows=8, ring=name == "b")
        self.in_flight = self.rows = self.turns = self.no_plane = 0

    def collect(self):
        got = self.stf.collect()
        if self.sgf is not None:
            self.rows += self.sgf.rows()["nrows"]
        self.stf.post_keys(got["seq"], np.zeros(0, np.int32))
        self.in_flight -= 1

    def run(self, iq, t):
        t0 = time.perf_counter()
        buf = self.feed.acquire()
        buf[:len(iq)] = iq
        self.feed.submit(len(iq), t_ms=t)
        self.in_flight += 1
        if self.in_flight > 2:
            self.collect()
        return time.perf_counter() - t0

    def check_form(self):
        """Outside the clock: did the batch submitted last keep a dB plane? (A refusal touches no stream.)"""
        self.turns += 1
        try:
            self.eng.read_window(abi.SS_PLANE_PSD, 0, 0, 64)
        except abi.SpecscanError as e:
            assert e.status == abi.SS_ERR_INVALID, e
            self.no_plane += 1

    def close(self):
        while self.in_flight:
            self.collect()
        self.eng.sync()
        s = self.eng.stats()
        for obj in (self.sgf, self.stf, self.feed, self.eng):
            if obj is not None:
                obj.close()
        return {k: s[k] for k in ("tiles_total", "tiles_tested", "tiles_culled")}


def kernel_stats(path):
    """One JSON line from a rocprofv3 --kernel-trace run of --route b: the rows kernels' device time per launch, shape by shape (the
    launches are taken in order: a run makes warm + reps of them per shape). A *_kernel_stats.csv gives totals only; a *_results.db
    (rocprofv3's SQLite output, view `kernels`) gives every launch."""
    if path.endswith(".db"):
        import sqlite3
        con = sqlite3.connect(path)
        launches = con.execute("select name, grid_x, end - start from kernels where name like '%k_spec_rows%' order by start").fetchall()
        total_ns = con.execute("select sum(end - start) from kernels").fetchone()[0]
        groups = []  # consecutive launches of one kernel and grid: one shape
        for name, grid, ns in launches:
            key = (name.split("(")[0].replace("void ", ""), int(grid) // 256)
            if not groups or groups[-1][0] != key:
                groups.append((key, []))
            groups[-1][1].append(ns / 1e3)
        out = [{"kernel": k[0], "workgroups": k[1], "launches": len(v), "us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
               for k, v in groups]
        print(json.dumps({"file": os.path.basename(path), "rows_kernels": out, "rows_kernels_us": round(sum(x[2] for x in launches) / 1e3, 1),
                          "all_kernels_us": round(total_ns / 1e3, 1)}), flush=True)
        return
    import csv
    rows, scan_ns = {}, 0
    for row in csv.DictReader(open(path)):
        name, ns, calls = row["Name"], int(float(row["TotalDurationNs"])), int(row["Calls"])
        if "k_spec_rows" in name:
            rows[name.split("(")[0].replace("void ", "")] = {"calls": calls, "us_per_call": round(ns / 1e3 / max(calls, 1), 2), "us": round(ns / 1e3, 1)}
        else:
            scan_ns += ns
    print(json.dumps({"file": os.path.basename(path), "rows_kernels": rows, "every_other_kernel_us": round(scan_ns / 1e3, 1)}), flush=True)


def shape(n, reps, warm, runs, distinct, routes):
    in_format, batch, frames = SHAPES[n]
    fs = n * 250
    period_ms = 1000.0 * n / fs
    band = pkg.synth.SyntheticBand(n, seed=0, on_frame=batch // 8 + 30, off_frame=5 * max(batch, 64) // 8 + 30, period=max(batch, 64) + 60)
    batches = [getattr(band, frames)(batch) for _ in range(distinct)]
    out = {"fft_size": n, "batch": batch, "in_format": frames[7:], "reps": reps, "warm": warm, "runs": runs, "input_bytes_per_turn": int(batches[0].nbytes)}
    per_run = {name: [] for name in routes}
    diffs = {"b_minus_a": [], "b_minus_c": []} if routes == "abc" else {}
    for run in range(runs):
        made = {name: Route(name, n, fs, batch, in_format, period_ms) for name in routes}
        times = {name: [] for name in routes}
        for k in range(warm + reps):
            t = np.round((k * batch + np.arange(batch)) * period_ms).astype(np.int64)
            for name, route in made.items():
                dt = route.run(batches[k % distinct], t)
                if name == "b":
                    route.check_form()
                if k >= warm:
                    times[name].append(dt)
        for name in routes:
            per_run[name].append(round(1e3 * statistics.median(times[name]), 3))
        if diffs:
            diffs["b_minus_a"].append(round(1e3 * statistics.median(p - q for p, q in zip(times["b"], times["a"])), 3))
            diffs["b_minus_c"].append(round(1e3 * statistics.median(p - q for p, q in zip(times["b"], times["c"])), 3))
        for name, route in made.items():
            tiles = route.close()
            if run == runs - 1:
                out[f"{LABELS[name]}_tiles"] = tiles
                out[f"{LABELS[name]}_rows"] = route.rows
                if name == "b":
                    out["ring_batches_without_db_plane"] = [route.no_plane, route.turns]
    for name in routes:
        label = LABELS[name]
        out[f"{label}_ms_median"] = statistics.median(per_run[name])
        out[f"{label}_ms_runs"] = per_run[name]
        out[f"{label}_batches_per_s"] = round(1e3 / out[f"{label}_ms_median"], 1)
    for key, vals in diffs.items():
        out[f"{key}_ms_median"] = statistics.median(vals)
        out[f"{key}_ms_runs"] = vals
    if diffs:
        spread = max(diffs["b_minus_a"]) - min(diffs["b_minus_a"])
        out["b_minus_a_spread_ms"] = round(spread, 3)
        out["ring_not_slower_than_planes"] = out["b_minus_a_ms_median"] <= spread
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--distinct", type=int, default=3)
    ap.add_argument("--shapes", default="65536,131072,262144")
    ap.add_argument("--route", default="abc", help="abc (all three, alternating), or one letter: that route alone")
    ap.add_argument("--out", default=None, help="a directory: the JSON lines are also written to DIR/rate.jsonl")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_results.db or *_kernel_stats.csv of a --route b run: print the rows kernels' time")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    if args.route not in ("abc", "a", "b", "c"):
        ap.error("--route: abc, a, b or c")
    lines = []
    for n in (int(s) for s in args.shapes.split(",")):
        if n not in SHAPES:
            ap.error("--shapes: 65536, 131072 and / or 262144")
        lines.append(shape(n, args.reps, args.warm, args.runs, args.distinct, args.route))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "rate.jsonl"), "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
