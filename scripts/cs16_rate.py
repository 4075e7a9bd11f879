"""CS16 against CF32 on this box: the same values (CS16 frames and their exact CF32 conversion, scale 1/32768) through the same
shapes, CF32 and CS16 runs alternating in one process, medians of the repeats with their spread. Prints one JSON object.
    python scripts/cs16_rate.py [--repeats 5] [--steps 200]

  step8192      device-resident 8192 x 1024-frame steps (BASELINE config 2's shape: dB plane and candidate lists out), ss_process_device
                calls without a synchronisation in between, drained; a rotation of input sets well past the Infinity Cache
  detect65536   65536 x 128 detect-mode calls (candidate lists only), device-resident
  detect2p20    2^20 x 16 detect-mode calls, device-resident
  process2p20   ss_process at 2^20 x 16: host buffers in (pageable), candidate lists back
Per-call figures in microseconds (per step for step8192)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtl_sdr_scanner_cpp_amd as pkg  # noqa: E402

A = pkg.abi
CENTER = 145_000_000


def _frames(n, nb, seed):
    band = pkg.synth.SyntheticBand(n, seed=seed, on_frame=0, off_frame=1 << 30)
    return band.frames_cs16(nb)


def _cf32(iq16):
    return (iq16.astype(np.float32) * np.float32(1.0 / 32768)).reshape(iq16.shape[0], -1)  # [F, 2N] float32 = [F, N] complex64


class Device:
    """One shape, one format: an engine on resident input sets, timed over `calls` ss_process_device calls."""

    def __init__(self, torch, fmt, n, fs, nb, nsets, want_psd, base16):
        self.torch, self.n, self.nb = torch, n, nb
        dev = torch.device("cuda:0")
        self.eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=nb, learn_frames=8,
                                      in_format=A.SS_FMT_CS16 if fmt == "cs16" else A.SS_FMT_CF32)
        src = torch.from_numpy(base16 if fmt == "cs16" else _cf32(base16)).to(dev)
        self.sets = [src if k == 0 else torch.roll(src, shifts=37 * k, dims=0).contiguous() for k in range(nsets)]
        cap = nb * 1024
        self.outs = [dict(psd=torch.empty((nb, n), dtype=torch.float32, device=dev) if want_psd else None,
                          off=torch.zeros(nb + 1, dtype=torch.int32, device=dev), idx=torch.empty(cap, dtype=torch.int32, device=dev),
                          avg=torch.empty(cap, dtype=torch.float32, device=dev)) for _ in range(nsets)]
        self.k = 0
        torch.cuda.synchronize()
        self.calls(max(1, -(-8 // nb)) + 4)  # learning and warm-up

    def calls(self, count):
        for _ in range(count):
            o = self.outs[self.k % len(self.outs)]
            src = self.sets[self.k % len(self.sets)]
            self.eng.process_device(src, self.nb, psd=o["psd"], cand_off=o["off"], cand_idx=o["idx"], cand_avg=o["avg"])
            self.k += 1
        self.eng.sync()

    def time(self, count):
        self.calls(5)
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.calls(count)
        self.torch.cuda.synchronize()
        return (time.perf_counter() - t0) / count * 1e6


class Host:
    """ss_process with host buffers: the input copy is part of every call."""

    def __init__(self, fmt, n, fs, nb, base16):
        self.eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=nb, learn_frames=8,
                                      in_format=A.SS_FMT_CS16 if fmt == "cs16" else A.SS_FMT_CF32)
        self.iq = base16 if fmt == "cs16" else _cf32(base16).view(np.complex64)
        self.time(2)

    def time(self, count):
        t0 = time.perf_counter()
        for _ in range(count):
            self.eng.process(self.iq, want=())
        return (time.perf_counter() - t0) / count * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="calls per timed run (step8192, detect65536); detect2p20 takes half, process2p20 a tenth")
    a = ap.parse_args()
    import torch
    shapes = {  # name: (n, fs, frames per call, input sets, dB plane out, calls per run)
        "step8192": (8192, 2_048_000, 1024, 24, True, a.steps),
        "detect65536": (65536, 20_000_000, 128, 24, False, a.steps),
        "detect2p20": (1 << 20, 61_440_000, 16, 12, False, max(1, a.steps // 2)),
    }
    res = {"what": "CS16 against CF32, the same values (exact conversion), alternating runs in one process; per-call microseconds",
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, (n, fs, nb, nsets, want_psd, calls) in shapes.items():
        base16 = _frames(n, nb, seed=n % 101)
        runs = {fmt: Device(torch, fmt, n, fs, nb, nsets, want_psd, base16) for fmt in ("cf32", "cs16")}
        t = {"cf32": [], "cs16": []}
        for _ in range(a.repeats):
            for fmt in ("cf32", "cs16"):
                t[fmt].append(runs[fmt].time(calls))
        res["shapes"][name] = _summary(n, nb, calls, t)
        del runs
        torch.cuda.empty_cache()
    n, fs, nb = 1 << 20, 61_440_000, 16
    base16 = _frames(n, nb, seed=5)
    runs = {fmt: Host(fmt, n, fs, nb, base16) for fmt in ("cf32", "cs16")}
    t = {"cf32": [], "cs16": []}
    calls = max(1, a.steps // 10)
    for _ in range(a.repeats):
        for fmt in ("cf32", "cs16"):
            t[fmt].append(runs[fmt].time(calls))
    res["shapes"]["process2p20"] = _summary(n, nb, calls, t)
    print(json.dumps(res))


def _summary(n, nb, calls, t):
    med = {f: statistics.median(v) for f, v in t.items()}
    return {"fft_size": n, "frames_per_call": nb, "calls_per_run": calls,
            **{f"{f}_us_median": round(med[f], 2) for f in t}, **{f"{f}_us_runs": [round(x, 2) for x in v] for f, v in t.items()},
            **{f"{f}_gsps": round(n * nb / med[f] / 1e3, 3) for f in t}, "cf32_over_cs16": round(med["cf32"] / med["cs16"], 3)}


if __name__ == "__main__":
    main()
