#!/usr/bin/env python3
"""How long ss_create + ss_destroy of one scan context take: the 8192-point default configuration unless told otherwise. One JSON line:
the median and the range of --pairs create / destroy pairs behind --warmup untimed ones. Needs an MI355X.

    python scripts/ctx_create_rate.py [--fft 8192] [--sample-rate 2048000] [--max-batch 1024] [--pairs 40] [--warmup 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fft", type=int, default=8192)
    ap.add_argument("--sample-rate", type=int, default=2_048_000)
    ap.add_argument("--max-batch", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import rtl_sdr_scanner_cpp_amd as pkg

    lib = pkg.load_library()
    pkg.abi.bind(lib, "ss_")
    cfg = pkg.abi.SsConfig()
    lib.ss_default_config(C.byref(cfg), args.sample_rate, 145_000_000)
    cfg.fft_size, cfg.max_batch = args.fft, args.max_batch
    ms = []
    for k in range(args.warmup + args.pairs):
        h = C.c_void_p()
        t0 = time.perf_counter()
        st = lib.ss_create(C.byref(cfg), C.byref(h))
        if st != 0:
            raise SystemExit(f"ss_create: {st} {lib.ss_last_error(None)}")
        lib.ss_destroy(h)
        if k >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"metric": "create_destroy_ms", "fft_size": args.fft, "max_batch": args.max_batch, "pairs": args.pairs,
                      "median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}))


if __name__ == "__main__":
    main()
