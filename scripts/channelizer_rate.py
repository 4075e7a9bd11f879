"""Throughput of the recorder channeliser on HBM-resident input (sc_process_device), next to the VALU bound, per input format;
with --host also sc_process from pageable host memory (the PCIe copy of the raw stream included); with --ranges also
sc_process_ranges_device with one whole-call range per slot (a twin context: ranges and start / stop are not mixed), which must
cost what sc_process_device costs.
    python scripts/channelizer_rate.py [--fs 2048000] [--bw 32000] [--samples 8388608] [--slots 1 4 8]
                                       [--format cf32 cs8 cu8 cs16] [--host] [--ranges] [--lib PATH]
                                       [--repeats 5] [--steps 20] [--host-steps 20]
The formats are timed in alternation, --repeats rounds of --steps (device, ranges) / --host-steps (host) calls each; the medians
of the rounds are reported. --lib: another build of the library (an A/B build of an older tree, say) instead of csrc/libspecscan.so."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rtl_sdr_scanner_cpp_amd import abi as A  # noqa: E402
from rtl_sdr_scanner_cpp_amd import engine  # noqa: E402
from rtl_sdr_scanner_cpp_amd.channelizer import Channelizer  # noqa: E402

FORMATS = {"cf32": (A.SS_FMT_CF32, np.float32), "cs8": (A.SS_FMT_CS8, np.int8), "cu8": (A.SS_FMT_CU8, np.uint8), "cs16": (A.SS_FMT_CS16, np.int16)}


def _stream(samples, name, rng):
    """The same noise in every format: [samples, 2] float32 (CF32) or the format's integers at a quarter of full scale."""
    x = rng.standard_normal((samples, 2), dtype=np.float32) * np.float32(0.25)
    if name == "cf32":
        return x
    full, off = {"cs8": (127.0, 0.0), "cu8": (127.5, 127.5), "cs16": (32767.0, 0.0)}[name]
    dt = FORMATS[name][1]
    return np.clip(np.rint(x * full + off), np.iinfo(dt).min, np.iinfo(dt).max).astype(dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, default=2_048_000)
    ap.add_argument("--bw", type=int, default=32_000)
    ap.add_argument("--samples", type=int, default=1 << 23)
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--format", nargs="+", default=["cf32"], choices=list(FORMATS))
    ap.add_argument("--host", action="store_true", help="also time sc_process from pageable host memory")
    ap.add_argument("--ranges", action="store_true", help="also time sc_process_ranges_device, one whole-call range per slot")
    ap.add_argument("--lib", default=None, help="path of another build of libspecscan.so to measure")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.lib:
        engine.use_diag_library(os.path.abspath(a.lib))
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    host = {f: _stream(a.samples, f, rng) for f in a.format}
    d_iq = {f: torch.from_numpy(host[f]).to(dev) for f in a.format}
    for nslots in a.slots:
        ctx, ctx_r, d_i8, h_i8 = {}, {}, {}, {}
        shifts = [int((k - nslots / 2) * 0.9 * a.fs / max(nslots, 2)) for k in range(nslots)]
        whole = [(k, shifts[k], 0, a.samples) for k in range(nslots)]
        counts = np.zeros(nslots, np.int32)
        for f in a.format:
            ch = Channelizer(a.fs, a.bw, in_format=FORMATS[f][0], channels=nslots, max_samples=a.samples)
            for k in range(nslots):
                ch.start(k, shifts[k])
            ctx[f] = ch
            if a.ranges:
                ctx_r[f] = Channelizer(a.fs, a.bw, in_format=FORMATS[f][0], channels=nslots, max_samples=a.samples)
        cap = ctx[a.format[0]].output_capacity(a.samples)
        for f in a.format:
            d_i8[f] = torch.zeros((nslots, cap, 2), dtype=torch.int8, device=dev)
            h_i8[f] = np.zeros((nslots, cap, 2), np.int8)

        def dev_call(f):
            ctx[f].process_device(d_iq[f], a.samples, d_i8[f], None, cap)

        def ranges_call(f):
            ctx_r[f].process_ranges_device(d_iq[f], a.samples, whole, d_i8[f], None, cap)

        def host_call(f):
            ch = ctx[f]
            ch._check(ch._lib.sc_process(ch._h, host[f].ctypes.data, a.samples, h_i8[f].ctypes.data, None,
                                         counts.ctypes.data_as(C.POINTER(C.c_int32)), cap))

        def timed(f, call, steps):
            c = ctx_r[f] if call is ranges_call else ctx[f]
            c.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                call(f)
            c.sync()
            return (time.perf_counter() - t0) / steps

        kinds = [("device", dev_call, a.steps)] + ([("ranges", ranges_call, a.steps)] if a.ranges else []) + ([("host", host_call, a.host_steps)] if a.host else [])
        for f in a.format:  # warm-up: code objects, staging buffers
            for _kind, call, _steps in kinds:
                for _ in range(3):
                    call(f)
            ctx[f].sync()
            if a.ranges:
                ctx_r[f].sync()
        runs = {(f, kind): [] for f in a.format for kind, _, _ in kinds}
        for _ in range(a.repeats):  # alternating rounds
            for kind, call, steps in kinds:
                for f in a.format:
                    runs[(f, kind)].append(timed(f, call, steps))
        ch = ctx[a.format[0]]
        taps_per_in = sum(nt / d * np.prod([i2 / d2 for i2, d2, _ in ch.stages[:k]]) for k, (i, d, nt) in enumerate(ch.stages))
        flops = 4.0 * taps_per_in * a.samples * nslots  # 2 FMA per tap per input sample (real taps, complex data)
        for f in a.format:
            dt = float(np.median(runs[(f, "device")]))
            rec = {"fs": a.fs, "bw": a.bw, "stages": ch.stages, "slots": nslots, "samples": a.samples, "format": f,
                   "input_MB": round(a.samples * A.SS_FMT_BYTES[FORMATS[f][0]] / 1e6, 1), "ms_per_call": round(dt * 1e3, 4),
                   "ms_per_call_runs": [round(t * 1e3, 4) for t in runs[(f, "device")]], "input_GSps": round(a.samples / dt / 1e9, 2),
                   "slot_GSps": round(a.samples * nslots / dt / 1e9, 2), "fir_TFLOPs": round(flops / dt / 1e12, 2),
                   "taps_per_input_sample": round(float(taps_per_in), 2)}
            if a.ranges:
                rt = float(np.median(runs[(f, "ranges")]))
                rec.update(ranges_ms_per_call=round(rt * 1e3, 4), ranges_ms_per_call_runs=[round(t * 1e3, 4) for t in runs[(f, "ranges")]])
            if a.host:
                ht = float(np.median(runs[(f, "host")]))
                rec.update(host_ms_per_call=round(ht * 1e3, 4), host_ms_per_call_runs=[round(t * 1e3, 4) for t in runs[(f, "host")]])
            print(json.dumps(rec), flush=True)
        for c in list(ctx.values()) + list(ctx_r.values()):
            c.close()


if __name__ == "__main__":
    main()
