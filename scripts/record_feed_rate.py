"""One batch recorded from the feed's own upload (srf_record) against the second-upload route (sc_process of the same samples from
pageable host memory), both synchronous and with the int8 outputs back on the host.
    python scripts/record_feed_rate.py [--fs 2048000] [--bw 32000] [--fft 8192] [--frames 1024] [--slots 4] [--format cf32 cs8]
                                       [--repeats 9]
Per format one JSON line: the medians of --repeats alternating calls, and their ratio.

    python scripts/record_feed_rate.py --items --decim 5 [--fraction 0.05 0.25 1.0] [--format cf32] ...
A decimated scan on a whole-item feed (engine.feed(items=True)): srf_record, which uploads only the union of the ranges it is
given, against the only other route to the same recording, sc_process_ranges with the whole batch of --frames items of fft * decim
samples uploaded, from the same pinned slot, alternating in one process. Every slot records the same window of --fraction of the
batch (from an odd sample in the middle of it). Per format and fraction one JSON line: medians, min - max, the uploaded bytes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtl_sdr_scanner_cpp_amd as pkg  # noqa: E402
from rtl_sdr_scanner_cpp_amd import abi as A  # noqa: E402
from rtl_sdr_scanner_cpp_amd.channelizer import Channelizer, ScRange  # noqa: E402

FORMATS = {"cf32": (A.SS_FMT_CF32, "frames_cf32"), "cs8": (A.SS_FMT_CS8, "frames_cs8"), "cu8": (A.SS_FMT_CU8, "frames_cu8"), "cs16": (A.SS_FMT_CS16, "frames_cs16")}


def items_lines(a):
    n, item = a.fft, a.fft * a.decim
    nsamples = item * a.frames
    shifts = [int((k - a.slots / 2) * 0.9 * a.fs / max(a.slots, 2)) for k in range(a.slots)]
    for f in a.format:
        fmt, frames = FORMATS[f]
        tile = getattr(pkg.synth.SyntheticBand(n, decim=a.decim, seed=1), frames)(8)
        eng = pkg.SpectrumEngine(a.fs, 145_000_000, fft_size=n, decim=a.decim, max_batch=a.frames, in_format=fmt)
        feed = eng.feed(depth=2, cand_cap=1 << 20, items=True)
        rec = feed.record(a.bw, channels=a.slots)
        ch = Channelizer(a.fs, a.bw, in_format=fmt, channels=a.slots, max_samples=nsamples)
        cap = ch.output_capacity(nsamples)
        h_i8 = np.zeros((a.slots, cap, 2), np.int8)
        counts, rcs = np.zeros(a.slots, np.int32), np.zeros(a.slots, np.int32)
        i32p = C.POINTER(C.c_int32)
        for frac in a.fraction:
            length = max(1, min(nsamples, int(round(frac * nsamples))))
            begin = min(nsamples - length, (nsamples - length) // 2 | 1) if length < nsamples else 0
            ranges = [(k, shifts[k], begin, begin + length) for k in range(a.slots)]
            arr = (ScRange * a.slots)(*(ScRange(*r) for r in ranges))
            t_feed, t_host, up, produced = [], [], 0, 0
            for it in range(a.repeats + 2):  # two warm-up rounds
                buf = feed.acquire()
                for at in range(0, a.frames, 8):
                    buf[at:at + 8] = tile[:min(8, a.frames - at)]
                feed.submit(a.frames)
                feed.collect()
                t0 = time.perf_counter()
                out, rc = rec.record(ranges)
                t1 = time.perf_counter()  # the slot is let go, and stays as it is until it is acquired again
                ch._check(ch._lib.sc_process_ranges(ch._h, buf.ctypes.data, nsamples, arr, a.slots, h_i8.ctypes.data, None, counts.ctypes.data_as(i32p),
                                                    rcs.ctypes.data_as(i32p), cap))
                t2 = time.perf_counter()
                up, produced = rec.last_h2d_bytes, int(rc.sum())
                assert list(rc) == list(rcs) and all(out[k][0].tobytes() == h_i8[k, :counts[k]].tobytes() for k in range(a.slots))
                if it >= 2:
                    t_feed.append((t1 - t0) * 1e3)
                    t_host.append((t2 - t1) * 1e3)
            mf, mh = float(np.median(t_feed)), float(np.median(t_host))
            print(json.dumps({"fs": a.fs, "bw": a.bw, "format": f, "slots": a.slots, "decim": a.decim, "items": a.frames, "samples": nsamples,
                              "fraction": frac, "batch_MB": round(nsamples * A.SS_FMT_BYTES[fmt] / 1e6, 1), "h2d_MB": round(up / 1e6, 1), "outputs": produced,
                              "srf_record_ms": round(mf, 4), "srf_record_ms_min_max": [round(min(t_feed), 4), round(max(t_feed), 4)],
                              "sc_process_ranges_ms": round(mh, 4), "sc_process_ranges_ms_min_max": [round(min(t_host), 4), round(max(t_host), 4)],
                              "ratio_whole_over_items": round(mh / mf, 2), "srf_record_ms_runs": [round(t, 4) for t in t_feed],
                              "sc_process_ranges_ms_runs": [round(t, 4) for t in t_host]}), flush=True)
        rec.close()
        feed.close()
        ch.close()
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, default=2_048_000)
    ap.add_argument("--bw", type=int, default=32_000)
    ap.add_argument("--fft", type=int, default=8192)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--format", nargs="+", default=["cf32", "cs8"], choices=list(FORMATS))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--decim", type=int, default=1)
    ap.add_argument("--items", action="store_true", help="a whole-item feed: srf_record against sc_process_ranges of the whole batch")
    ap.add_argument("--fraction", type=float, nargs="+", default=[0.05, 0.25, 1.0], help="with --items: the part of the batch every slot records")
    a = ap.parse_args()
    if a.items:
        return items_lines(a)
    if a.decim != 1:
        ap.error("--decim needs --items: an ordinary feed of a decimated scan has no stream to record from")
    n, nsamples = a.fft, a.fft * a.frames
    shifts = [int((k - a.slots / 2) * 0.9 * a.fs / max(a.slots, 2)) for k in range(a.slots)]
    whole = [(k, shifts[k], 0, nsamples) for k in range(a.slots)]
    for f in a.format:
        fmt, frames = FORMATS[f]
        tile = getattr(pkg.synth.SyntheticBand(n, seed=1), frames)(8)
        batch = np.ascontiguousarray(np.concatenate([tile] * (a.frames // 8)))
        eng = pkg.SpectrumEngine(a.fs, 145_000_000, fft_size=n, decim=1, max_batch=a.frames, in_format=fmt)
        feed = eng.feed(depth=2, cand_cap=1 << 20)
        rec = feed.record(a.bw, channels=a.slots)
        ch = Channelizer(a.fs, a.bw, in_format=fmt, channels=a.slots, max_samples=nsamples)
        for k in range(a.slots):
            ch.start(k, shifts[k])
        cap = ch.output_capacity(nsamples)
        h_i8 = np.zeros((a.slots, cap, 2), np.int8)
        counts = np.zeros(a.slots, np.int32)
        t_feed, t_host, produced = [], [], 0
        for it in range(a.repeats + 2):  # two warm-up rounds
            feed.acquire()[:] = batch
            feed.submit(a.frames)
            feed.collect()
            t0 = time.perf_counter()
            out, rc = rec.record(whole)
            t1 = time.perf_counter()
            ch._check(ch._lib.sc_process(ch._h, batch.ctypes.data, nsamples, h_i8.ctypes.data, None, counts.ctypes.data_as(C.POINTER(C.c_int32)), cap))
            t2 = time.perf_counter()
            produced = int(rc.sum())
            assert produced == int(counts.sum())
            if it >= 2:
                t_feed.append(t1 - t0)
                t_host.append(t2 - t1)
        mf, mh = float(np.median(t_feed)), float(np.median(t_host))
        print(json.dumps({"fs": a.fs, "bw": a.bw, "format": f, "slots": a.slots, "samples": nsamples, "input_MB": round(batch.nbytes / 1e6, 1),
                          "outputs": produced, "srf_record_ms": round(mf * 1e3, 4), "sc_process_ms": round(mh * 1e3, 4),
                          "ratio_host_over_feed": round(mh / mf, 2), "srf_record_ms_runs": [round(t * 1e3, 4) for t in t_feed],
                          "sc_process_ms_runs": [round(t * 1e3, 4) for t in t_host]}), flush=True)
        rec.close()
        feed.close()
        ch.close()
        eng.close()


if __name__ == "__main__":
    main()
