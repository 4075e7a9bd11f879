"""Microseconds per detect-mode ss_process_device call at 65536 and 131072 points, three routes, one process, the same stream:

  (f) CS16 flagged:    a CS16 context created with SS_FLAG_FOLD_CS16 — calls that keep no plane take the radix-8 / radix-16 fold.
  (u) CS16 unflagged:  the same context without the flag: the merged four-step chain at 65536 points, the unculled chain at 131072 —
                       byte for byte what CS16 got before the flag existed. THE BASELINE of (f).
  (8) CS8:             the int8 context (the fold by default), fed the same band at eight bits: what the fold does at half the input bytes.

Shapes: 65536 points x {16, 128, 512} frames and 131072 points x {24, 64} frames. A call hands out no plane (lists only); the learning
frames are a call of their own before the clock starts. A turn is --calls calls back to back on device-resident input — the calls go
round at least --sets device batches at distinct addresses, 512 MiB of CS16 input or more (up to 32 batches), so that nothing a call
reads is left in the 256 MiB Infinity Cache by the call before (the script prints the bytes) — ended by ss_sync: wall clock around the turn over the
calls in it. The routes alternate turn by turn; --warm turns are not counted; the median over --reps turns is a run's figure, the whole
measurement runs --runs times, and the median of the runs' medians is reported next to every run's. ss_get_stats per route says which
form ran (fold, culling) and the tile counters.

    python scripts/fold_cs16_rate.py [--out profiles/fold_cs16/rate.json] [--shapes 65536x16,65536x128,...] [--calls 200] [--reps 9] [--warm 2] [--runs 3] [--sets 6]

Prints one JSON line per shape and, with --out, writes them all to that file with a table (us per call, GS/s, flagged over unflagged).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtl_sdr_scanner_cpp_amd as pkg  # noqa: E402
from rtl_sdr_scanner_cpp_amd import abi  # noqa: E402

SHAPES = [(65536, 16), (65536, 128), (65536, 512), (131072, 24), (131072, 64)]
ROUTES = {"f": ("cs16_flagged", abi.SS_FMT_CS16, abi.SS_FLAG_FOLD_CS16, "frames_cs16"),
          "u": ("cs16_unflagged", abi.SS_FMT_CS16, 0, "frames_cs16"),
          "8": ("cs8", abi.SS_FMT_CS8, 0, "frames_cs8")}
LEARN = 21
CENTER = 145_000_000


class Route:
    def __init__(self, key, n, frames, host_sets, learn_iq, nsets):
        import torch
        self.label, in_format, flags, _ = ROUTES[key]
        self.frames, self.n = frames, n
        self.eng = pkg.SpectrumEngine(20_000_000, CENTER, fft_size=n, decim=1, max_batch=max(frames, LEARN), learn_frames=LEARN, in_format=in_format, flags=flags)
        dev = torch.device("cuda", 0)
        self.sets = [torch.from_numpy(host_sets[i % len(host_sets)]).to(dev) for i in range(nsets)]  # (distinct addresses: what the cache sees)
        cap = frames * 2048
        self.outs = [(torch.zeros(frames + 1, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.float32, device=dev))
                     for _ in range(nsets)]
        d_learn = torch.from_numpy(learn_iq).to(dev)
        off = torch.zeros(LEARN + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        self.eng.process_device(d_learn, LEARN, cand_off=off, cand_idx=self.outs[0][1], cand_avg=self.outs[0][2])
        self.eng.sync()
        self.k = 0
        self.candidates = 0

    def turn(self, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            s = self.k % len(self.sets)
            off, idx, avg = self.outs[s]
            self.eng.process_device(self.sets[s], self.frames, cand_off=off, cand_idx=idx, cand_avg=avg)
            self.k += 1
        self.eng.sync()
        dt = time.perf_counter() - t0
        self.candidates = int(self.outs[(self.k - 1) % len(self.sets)][0][-1])
        return dt / calls


def shape(n, frames, calls, reps, warm, runs, nsets, routes):
    # device sets: at least --sets, and enough of them that the CS16 input alone is twice the Infinity Cache (at most 32)
    nsets = max(nsets, min(32, -(-(512 << 20) // (frames * n * 4))))
    distinct = min(nsets, 3)
    host = {"frames_cs16": None, "frames_cs8": None}
    for kind in host:  # the same band for every format: a fresh generator with the same seed
        b = pkg.synth.SyntheticBand(n, seed=46, on_frame=LEARN + 24, off_frame=LEARN + 24 + 5 * max(frames, 64) // 8, period=max(frames, 64) + 60)
        learn = getattr(b, kind)(LEARN)
        host[kind] = (learn, [getattr(b, kind)(frames) for _ in range(distinct)])
    out = {"fft_size": n, "frames": frames, "calls_per_turn": calls, "reps": reps, "warm": warm, "runs": runs, "device_sets": nsets, "distinct_host_batches": distinct,
           "input_bytes_per_call": {ROUTES[k][0]: int(host[ROUTES[k][3]][1][0].nbytes) for k in routes}}
    per_run = {k: [] for k in routes}
    for run in range(runs):
        made = {k: Route(k, n, frames, host[ROUTES[k][3]][1], host[ROUTES[k][3]][0], nsets) for k in routes}
        times = {k: [] for k in routes}
        for rep in range(warm + reps):
            for k, route in made.items():
                dt = route.turn(calls)
                if rep >= warm:
                    times[k].append(dt)
        for k, route in made.items():
            per_run[k].append(round(1e6 * statistics.median(times[k]), 2))
            if run == runs - 1:
                st = route.eng.stats()
                out[f"{route.label}_stats"] = {key: st[key] for key in ("fold", "culling", "tiles_total", "tiles_tested", "tiles_culled")}
                out[f"{route.label}_candidates_last_call"] = route.candidates
            route.eng.close()
        del made
    for k in routes:
        label = ROUTES[k][0]
        us = statistics.median(per_run[k])
        out[f"{label}_us_per_call"] = us
        out[f"{label}_us_runs"] = per_run[k]
        out[f"{label}_gsamples_per_s"] = round(frames * n / us * 1e-3, 1)
    if "f" in routes and "u" in routes:
        out["flagged_over_unflagged"] = round(out["cs16_flagged_us_per_call"] / out["cs16_unflagged_us_per_call"], 3)
    print(json.dumps(out), flush=True)
    return out


def table(rows):
    lines = ["| points x frames | CS16 flagged us (GS/s) | CS16 unflagged us (GS/s) | CS8 us (GS/s) | flagged / unflagged |", "|---|---|---|---|---|"]
    for r in rows:
        cell = lambda label: f"{r[label + '_us_per_call']:.1f} ({r[label + '_gsamples_per_s']:.0f})" if label + "_us_per_call" in r else "-"  # noqa: E731
        lines.append(f"| {r['fft_size']} x {r['frames']} | {cell('cs16_flagged')} | {cell('cs16_unflagged')} | {cell('cs8')} | {r.get('flagged_over_unflagged', '-')} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(f"{n}x{f}" for n, f in SHAPES))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--routes", default="fu8")
    args = ap.parse_args()
    if not args.routes or any(k not in ROUTES for k in args.routes):
        ap.error("--routes: letters of f, u, 8")
    import torch
    if not torch.cuda.is_available():
        sys.exit("fold_cs16_rate: no GPU; a rate is measured on one or not at all")
    rows = []
    for item in args.shapes.split(","):
        n, frames = (int(v) for v in item.split("x"))
        if n not in (65536, 131072) or frames < 1:
            ap.error("--shapes: 65536xF or 131072xF")
        rows.append(shape(n, frames, args.calls, args.reps, args.warm, args.runs, args.sets, args.routes))
        if args.out:  # (after every shape: a run cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fp:
                json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fp, indent=1)
            with open(os.path.splitext(args.out)[0] + ".md", "w") as fp:
                fp.write(f"Detect-mode ss_process_device calls, steady state, {torch.cuda.get_device_name(0)} (scripts/fold_cs16_rate.py)\n\n" + table(rows) + "\n")


if __name__ == "__main__":
    main()
