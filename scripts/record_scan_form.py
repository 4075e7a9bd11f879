#!/usr/bin/env python3
"""Record what ss_create decides and allocates, case by case, from a diagnostics library that prints it: the fixture
tests/golden/scan_form_parent.json, which tests/test_scan_form.py holds decide_form (csrc/scan_form.h) and alloc_ctx_buffers
(csrc/ctx_buffers.h) to.

The fixture was recorded on an MI355X from the commit before the form became a function of its own, with a patch that is not part of the
repository: in the -DSS_DIAG build every hipMalloc inside ss_create went through a wrapper that noted the expression it was given and its
byte count, and at the end of a successful ss_create, when SS_FORM_RECORD named a file, one line was appended to it:

    status=0 n=.. logn=.. fused=.. ... order_capacity=..  tw256=.. ... dif8_tab=..  sizes=<bytes>,<bytes>,...

that is the decided members of ss_ctx (FIELDS below, in this order), whether each optional table's pointer was set, and the sorted byte
counts of every allocation but the constant tables (d_win, d_tw, d_tw256, d_tw_small, d_tw_cols, d_tw_rowsR, d_tw_sub, d_tw8k, d_tw8v2,
d_win1024, d_wtab1024, d_dif8_tab). A create call that was refused is recorded with its status and text.

    python scripts/record_scan_form.py --lib path/to/libspecscan_diag.so --out tests/golden/scan_form_parent.json

Cases whose context would take more than about 8 GiB are not run and are listed in the fixture as dropped (by their index in cases()). `--list FILE` writes the case
lines only (what the host checks read), without a library or a GPU."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("status n logn fused step_path deep nq lag ncnt nbuf npsd det_lag2 merge merge_max dif8 dif_logq cull_fold_only plan_all cull cull_long x256_tile "
          "rows1024x256 rows256_step two_pass use_fft256 use_fft8192 spec_n spec_m spec_in_detect ref_nan deep_ring_safe hist_rows smax_rows order_capacity "
          "tw256 tw_small tw_cols tw_rowsR tw_sub tw8k tw8v2 win1024 wtab dif8_tab").split()
SIZES = [256, 1024, 4096, 8192, 16384, 65536, 131072, 262144, 524288, 1 << 20]
FLAGS = [0, 1, 2, 4, 8, 16, 4 | 1]  # none, each of the five alone, NO_CULL | KEEP_PLANES
# every switch of Diag::read() alone, at a value that is not the product's
SWITCHES = ["SS_BACKEND=unfused", "SS_FFT_IMPL=generic", "SS_FFT_ROWSR=0", "SS_FFT_ROWSR=1", "SS_FFT_SUB=0", "SS_FFT_SUB=1", "SS_FFT_TWOPASS=0", "SS_RING_ONLY=0",
            "SS_FFT_XCDMAP=0", "SS_SPEC_IMPL=standalone", "SS_PIPELINE=0", "SS_FFT_TW=0", "SS_FFT_SWZ=0", "SS_STEP_PRIO_FFT=1", "SS_STEP_PRIO_OTHER=1", "SS_EMIT_WIDE=0",
            "SS_STEP_LONG=0", "SS_DEEP=0", "SS_CULL=0", "SS_ABLATE_ROLES=1", "SS_CULL_65536=0", "SS_ROWS256_STEP=0", "SS_PLAN_FUSED=0", "SS_LIST_FIRST=0", "SS_HALO_MAXIMA=0",
            "SS_LIST_FIRST_FOLD=3", "SS_CHUNK_LONG=0", "SS_CHUNK_65536=0", "SS_ROWS1024X256=0", "SS_ABS_START=1000", "SS_DRAIN_TAIL_EVENT=0", "SS_PLAN_FIRST=4", "SS_DET_LAG2=0",
            "SS_DIF8=0", "SS_EMIT_ON_ROWS=1", "SS_MERGE_65536=0", "SS_MERGE_MAX=32", "SS_WIN_CALC=0", "SS_CANARY=1", "SS_QUEUES=3", "SS_QUEUES=4", "SS_HINT_MODE=1",
            "SS_WAIT_LIMIT=64", "SS_ORDER_TABLE=0", "SS_PLAN_NOZERO=1", "SS_CULL_STATS=1", "SS_STEP_ORDER=E*|D*,F*", "SS_STEP_ORDER_MERGED=E*|D*,R*,F*"]
SIZE_LIMIT = 8 << 30


def case_line(n, fmt, window, flags, grouping, max_batch, switch=None):
    """n sample_rate fmt window flags gx gy max_batch [switch]: the sample rate is the one whose default transform has n points"""
    gx, gy = grouping
    return " ".join(str(v) for v in (n, n * 250, fmt, int(window), flags, gx, gy, max_batch)) + (" " + switch if switch else "")


def cases():
    out = []
    for n in SIZES:
        batches = [16, 64] + ([1024] if n <= 8192 else [])
        for fmt in (0, 1):  # CF32, CS8
            for window in (False, True):
                for flags in FLAGS:
                    for grouping in ((21, 21), (5, 3)):
                        for mb in batches:
                            out.append(case_line(n, fmt, window, flags, grouping, mb))
        # the switches alone: on the default configuration of each size at 64 frames, both formats, and with the spectrogram the one that asks for it
        for sw in SWITCHES:
            for fmt in (0, 1):
                out.append(case_line(n, fmt, False, 0, (21, 21), 64, sw))
        out.append(case_line(n, 0, False, 2, (21, 21), 64, "SS_SPEC_IMPL=standalone"))
    return out


def upper_bound_bytes(line):
    """more than any form allocates: the ring at its largest, twelve planes' worth of rotating sets and work buffers (twenty at 8192 points and below)"""
    n, _, _, _, _, _, _, mb = (int(v) for v in line.split()[:8])
    ring = max(1024, 4 * (mb + 35)) if n >= 65536 else 64 * 35
    return 4 * n * (ring + mb * (12 if n >= 16384 else 20))


def parse(text):
    """a recorded line -> (values in FIELDS order, sizes run-length coded) or (status, text) of a refusal"""
    kv = dict(item.split("=", 1) for item in text.split(" ") if "=" in item and not item.startswith(("err=", "sizes=")))
    if int(kv["status"]) != 0:
        return [int(kv["status"]), text.split("err=", 1)[1]], None
    sizes = [int(v) for v in text.split("sizes=", 1)[1].split(",")] if "sizes=" in text else None
    return [int(kv[k]) for k in FIELDS], sizes


def run_lengths(sizes):
    out = []
    for v in sizes:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return " ".join(f"{v}*{c}" if c > 1 else str(v) for v, c in out)


def cases_digest():
    return hashlib.sha256("\n".join(cases()).encode()).hexdigest()


def write_fixture(out_path, forms, form_of_case, dropped):
    """The case lines are not stored: cases() gives them, in order, and their digest says that it still gives the ones recorded.
    form_of_case[k] is the index into forms of cases()[k] (-1: dropped); a form is a pair of indices, into values (the decided members in
    FIELDS order, or [status, text] of a refusal) and into sizes (the run-length coded byte counts, null for a refusal): many share either."""
    values, sizes = [], []
    for v, z in forms:
        if v not in values:
            values.append(v)
        if z not in sizes:
            sizes.append(z)
    head = {"about": "what ss_create decided and allocated before scan_form.h: scripts/record_scan_form.py", "fields": FIELDS, "cases_sha256": cases_digest(),
            "dropped": dropped, "form_of_case": form_of_case, "forms": [[values.index(v), sizes.index(z)] for v, z in forms]}
    rows = lambda items: ",\n".join(json.dumps(item, separators=(",", ":")) for item in items)  # noqa: E731
    with open(out_path, "w") as fp:
        fp.write(json.dumps(head, separators=(",", ":"))[:-1] + ',\n"values":[\n' + rows(values) + '\n],\n"sizes":[\n' + rows(sizes) + "\n]}\n")


def record(lib_path, out_path):
    from rtl_sdr_scanner_cpp_amd import abi

    lib = C.CDLL(lib_path)
    abi.bind(lib, "ss_")
    forms, index, form_of_case, dropped = [], {}, [], []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "form.txt")
        os.environ["SS_FORM_RECORD"] = path
        window = np.ones(1 << 20, np.float32)  # (a caller's window: any taps)
        for k, line in enumerate(cases()):
            if upper_bound_bytes(line) > SIZE_LIMIT:
                dropped.append(k)
                form_of_case.append(-1)
                continue
            words = line.split()
            n, fs, fmt, win, flags, gx, gy, mb = (int(v) for v in words[:8])
            switches = [w.split("=", 1) for w in words[8:]]
            for name, value in switches:
                os.environ[name] = value
            cfg = abi.SsConfig()
            lib.ss_default_config(C.byref(cfg), fs, 100_000_000)
            assert cfg.fft_size == n, (cfg.fft_size, n)
            cfg.in_format, cfg.flags, cfg.grouping_x, cfg.grouping_y, cfg.max_batch = fmt, flags, gx, gy, mb
            if win:
                cfg.window = window.ctypes.data_as(abi.c_float_p)
            open(path, "w").close()
            h = C.c_void_p()
            st = lib.ss_create(C.byref(cfg), C.byref(h))
            for name, _ in switches:
                del os.environ[name]
            if st == 0:
                lib.ss_destroy(h)
                text = open(path).read().strip()
            else:
                text = f"status={st} err=" + (lib.ss_last_error(None) or b"").decode()
            values, sizes = parse(text)
            key = json.dumps([values, None if sizes is None else run_lengths(sizes)])
            if key not in index:
                index[key] = len(forms)
                forms.append(json.loads(key))
            form_of_case.append(index[key])
            if k % 200 == 0:
                print(k, line, flush=True)
    write_fixture(out_path, forms, form_of_case, dropped)
    print(f"{len(form_of_case) - len(dropped)} cases, {len(forms)} forms, {len(dropped)} dropped, {os.path.getsize(out_path)} bytes")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--list")
    args = ap.parse_args()
    if args.list:
        with open(args.list, "w") as fp:
            fp.write("\n".join(cases()) + "\n")
        return
    record(args.lib, args.out)


if __name__ == "__main__":
    main()
