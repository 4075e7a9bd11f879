"""The pipelined feed's batches per second with and without the spectrogram rows (include/specscan_spectrogram_feed.h), one process,
the same synthetic stream (synth.SyntheticBand), the same build:

  (p) plain: ss_feed_acquire / ss_feed_submit / ss_feed_collect, depth 3, SS_FLAG_SPECTROGRAM on the context
  (r) rows:  the same with an sgf_ctx on the feed, sgf_rows after every collect

at 8192 points in 1024-frame batches (2.048 MS/s: a batch is 4.1 s of signal and closes four rows). A turn fills a pinned slot,
submits it and — from the third turn on — collects the oldest batch, so the time per turn is the time per batch with two batches in
flight. The two routes alternate turn by turn; wall clock, median of --reps turns after a warm-up. Prints one JSON line.
With --route r only that route runs: the form to put behind `rocprofv3 --kernel-trace --stats --` for k_spec_rows' device time
(compare with its byte floor: the batch's dB plane, frames * N * 4 bytes, read once).

    python scripts/spectrogram_rows_rate.py [--reps 15] [--route pr|p|r] [--fft 8192] [--batch 1024]
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


class FeedRoute:
    def __init__(self, n, fs, batch, rows: bool):
        self.batch = batch
        self.eng = pkg.SpectrumEngine(fs, 145_000_000, fft_size=n, decim=1, max_batch=batch, learn_ms=280, flags=abi.SS_FLAG_SPECTROGRAM)
        self.feed = self.eng.feed(depth=3, cand_cap=batch * 1024)
        self.sgf = self.feed.spectrogram(max_rows=16) if rows else None
        self.in_flight = 0
        self.rows = 0

    def collect(self):
        self.feed.collect()
        self.in_flight -= 1
        if self.sgf:
            self.rows += self.sgf.rows()["nrows"]

    def run(self, iq, t):
        t0 = time.perf_counter()
        buf = self.feed.acquire()
        np.copyto(buf[:self.batch], iq)
        self.feed.submit(self.batch, t_ms=t)
        self.in_flight += 1
        if self.in_flight > 2:
            self.collect()
        return time.perf_counter() - t0

    def drain(self):
        while self.in_flight:
            self.collect()


LABELS = {"p": "plain", "r": "rows"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--route", default="pr", choices=("pr", "p", "r"))
    ap.add_argument("--fft", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=1024)
    args = ap.parse_args()
    n, batch, warm, distinct = args.fft, args.batch, 4, 4
    fs = 2_048_000 if n == 8192 else n * 250
    period_ms = 1000.0 * n / fs
    band = pkg.synth.SyntheticBand(n, seed=0, on_frame=batch // 8 + 30, off_frame=5 * max(batch, 64) // 8 + 30, period=max(batch, 64) + 60)
    batches = [band.frames_cf32(batch) for _ in range(distinct)]
    made = {name: FeedRoute(n, fs, batch, rows=name == "r") for name in args.route}
    times = {name: [] for name in made}
    for k in range(warm + args.reps):
        t = np.round(1_000 + period_ms * (k * batch + np.arange(batch))).astype(np.int64)
        for name, route in made.items():
            dt = route.run(batches[k % distinct], t)
            if k >= warm:
                times[name].append(dt)
    out = {"fft_size": n, "batch": batch, "reps": args.reps, "plane_bytes": 4 * n * batch}
    for name, route in made.items():
        route.drain()
        label = LABELS[name]
        med = statistics.median(times[name])
        out[f"{label}_ms_median"] = round(1e3 * med, 3)
        out[f"{label}_batches_per_s"] = round(1.0 / med, 2)
        out[f"{label}_ms_all"] = [round(1e3 * x, 3) for x in times[name]]
    if "r" in made:
        out["rows_closed"] = made["r"].rows
    if len(made) == 2:
        out["rows_over_plain"] = round(out["rows_ms_median"] / out["plain_ms_median"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
