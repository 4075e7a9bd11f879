#!/usr/bin/env python3
"""Record what run_batch decides call by call, from a diagnostics library that prints it: the fixture
tests/golden/call_route_parent.json, which tests/test_call_route.py holds decide_call (csrc/call_route.h) to and
tests/test_gpu_call_route.py holds run_batch to.

The -DSS_DIAG library appends one line per call to the file SS_ROUTE_RECORD names (Diag::route_path, print_route of call_route.h): the
ask, then the route, as name=value in the order of FIELDS below.

The fixture was recorded on an MI355X from the commit before the decision became a function of its own, with a patch that is not part
of the repository: Diag read SS_ROUTE_RECORD as it does now, and run_batch wrote the same line from its own locals — the shape from
the branch it took (in the deep and the non-step branch every predicate 0, but, on the deep path, overlap = allow_overlap &&
diag.pipeline && n_learn == 0 && nframes >= kHistRows, run_call_deep's predicate without the two terms that are the context's state),
in the step branch keeps_no_plane, dif_call, db_call, cull_call, ring_by_rows, ring_only (as place_ring's answer gave it), overlap and
merged_call as they stood, plan_fused as computed under cull_call (0 where it was not computed), det_lag2 the context's, the chunk of
the loop that ran (nframes where none did) and the rider kinds its first two launches named.

    python scripts/record_call_route.py --lib path/to/libspecscan_diag.so --out tests/golden/call_route_parent.json

Every session runs in a child process of its own (`--session K`), under a time limit. `--list` prints the sessions; `--keep DIR` keeps every session's lines as DIR/route_K.txt."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ASK = "nframes n_learn device psd rel avg spec".split()
FIELDS = ASK + "shape keeps_no_plane dif_call db_call cull_call ring_by_rows ring_only overlap merged_call plan_fused det_lag2 chunk ride_first ride_second".split()
SHAPES = "deep frames_8192 cols_rows fold merged rows256_step rows1024x256 two_pass non_step".split()
PREDICATES = "keeps_no_plane dif_call db_call cull_call ring_by_rows ring_only overlap merged_call plan_fused".split()
CF32, CS8 = 0, 1
KEEP_PLANES, SPECTROGRAM, STREAM_ORDERED = 1, 2, 8
LEARN_FRAMES = 10  # the first call of a session, and the first after its retune, learn in part
SESSION_TIMEOUT = 120


def sessions():
    """(n, in_format, flags, max_batch, switch or None): the case line of scripts/record_scan_form.py plus what the session does"""
    out = []
    for n, fmt in ((8192, CF32), (65536, CS8), (65536, CF32), (131072, CS8), (131072, CF32), (262144, CF32), (1 << 20, CF32)):
        for flags in (0, SPECTROGRAM, KEEP_PLANES):
            out.append((n, fmt, flags, 64, None))
    out.append((262144, CF32, 0, 128, None))  # (its 64-frame chunk loop runs twice)
    for n, fmt, switch in ((65536, CS8, "SS_PIPELINE=0"), (1 << 20, CF32, "SS_RING_ONLY=0"), (65536, CF32, "SS_DET_LAG2=0"), (65536, CF32, "SS_MERGE_65536=0"),
                           (65536, CF32, "SS_MERGE_MAX=32"), (65536, CS8, "SS_DIF8=0"), (1 << 20, CF32, "SS_PLAN_FUSED=0"), (65536, CF32, "SS_EMIT_ON_ROWS=1"),
                           (65536, CF32, "SS_CHUNK_65536=32"), (1 << 20, CF32, "SS_CHUNK_LONG=0")):
        out.append((n, fmt, 0, 64, switch))
    # the shapes no session above reaches: 8192 points in order on the public stream, and a size off the step path
    out.append((8192, CF32, STREAM_ORDERED, 64, None))
    out.append((1024, CF32, 0, 64, None))
    return out


def case_line(session):
    n, fmt, flags, mb, switch = session
    return " ".join(str(v) for v in (n, n * 250, fmt, 0, flags, 21, 21, mb)) + (" " + switch if switch else "")


def sessions_digest():
    return hashlib.sha256("\n".join(case_line(s) for s in sessions()).encode()).hexdigest()


def parse(line):
    kv = dict(item.split("=", 1) for item in line.split())
    assert list(kv) == FIELDS, line
    return kv


def run_session(lib_path, k):
    """The calls of one session (this process: one context, then gone). Device memory comes from the HIP runtime directly."""
    import numpy as np
    import rtl_sdr_scanner_cpp_amd as pkg

    n, fmt, flags, mb, switch = sessions()[k]
    if switch:
        name, value = switch.split("=", 1)
        os.environ[name] = value
    pkg.engine.use_diag_library(lib_path)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def dev(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        return p

    eng = pkg.SpectrumEngine(n * 250, 500_000_000, fft_size=n, decim=1, in_format=fmt, flags=flags, max_batch=mb, learn_frames=LEARN_FRAMES)
    rng = np.random.default_rng(n + fmt)
    frame = ((rng.standard_normal((n, 2)) * 20).astype(np.int8) if fmt == CS8 else (rng.standard_normal((n, 2)) * 0.05).astype(np.float32))
    frame_bytes = frame.nbytes
    d_iq = dev(frame_bytes * mb)
    for f in range(mb):  # every frame the same noise: what a call decides does not look at the samples
        assert hip.hipMemcpy(C.c_void_p(d_iq.value + f * frame_bytes), frame.ctypes.data_as(C.c_void_p), frame_bytes, 1) == 0
    cap = 4096
    d_off, d_idx, d_avg = dev(4 * (mb + 1)), dev(4 * cap), dev(4 * cap)
    d_psd, d_avgp = dev(4 * 16 * n), dev(4 * 16 * n)
    lib, h = eng._lib, eng._h

    def call(nframes, psd=None, avg=None):
        eng._check(lib.ss_process_device(h, d_iq, nframes, psd, None, avg, d_off, d_idx, d_avg, cap))

    for nframes in (16, 7, 35, 36, mb):
        call(nframes)
    call(16, d_psd, d_avgp)
    host = np.ascontiguousarray(np.broadcast_to(frame, (16,) + frame.shape))
    eng.process(host if fmt == CS8 else host.view(np.complex64)[..., 0], want=(), cand_cap=cap)
    eng.set_frequency_range(501_000_000 - n * 125, 501_000_000 + n * 125)  # a retune between two calls: a new ceiling to learn
    for nframes in (36, 16, mb):
        call(nframes)
    eng.sync()
    eng.close()
    for p in (d_iq, d_off, d_idx, d_avg, d_psd, d_avgp):
        hip.hipFree(p)


def record_sessions(lib_path, which=None, keep=None):
    """{session index: its lines}, each session in a child process under its own time limit"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        if keep:
            os.makedirs(keep, exist_ok=True)
        for k in (range(len(sessions())) if which is None else which):
            path = os.path.join(keep or tmp, f"route_{k}.txt")
            open(path, "w").close()
            env = {name: v for name, v in os.environ.items() if not name.startswith("SS_")}
            env["SS_ROUTE_RECORD"] = path
            subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib_path, "--session", str(k)], check=True, timeout=SESSION_TIMEOUT, env=env)
            with open(path) as fp:
                out[k] = fp.read().strip().splitlines()
    return out


def complete(lines):
    """what never occurs among the lines: shapes of the enum, values of a predicate"""
    rows = [parse(line) for line in lines]
    missing = [s for s in SHAPES if not any(r["shape"] == s for r in rows)]
    missing += [f"{p}={v}" for p in PREDICATES for v in "01" if not any(r[p] == v for r in rows)]
    return missing


def write_fixture(out_path, by_session):
    """the session lines are not stored (sessions() gives them, their digest says it still gives the ones recorded); `lines` holds every
    recorded line once, `calls[k]` the indices of session k's lines in call order"""
    lines = sorted({line for k in by_session for line in by_session[k]})
    missing = complete(lines)
    if missing:
        raise SystemExit(f"the sessions never reach: {missing}")
    head = {"about": "what run_batch decided call by call before call_route.h: scripts/record_call_route.py", "fields": FIELDS, "sessions_sha256": sessions_digest(),
            "calls": [[lines.index(line) for line in by_session[k]] for k in range(len(sessions()))]}
    with open(out_path, "w") as fp:
        fp.write(json.dumps(head, separators=(",", ":"))[:-1] + ',\n"lines":[\n' + ",\n".join(json.dumps(line) for line in lines) + "\n]}\n")
    print(f"{len(by_session)} sessions, {sum(len(v) for v in by_session.values())} calls, {len(lines)} different lines, {os.path.getsize(out_path)} bytes")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--session", type=int)
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--keep")
    args = ap.parse_args()
    if args.list:
        print("\n".join(case_line(s) for s in sessions()))
    elif args.session is not None:
        run_session(os.path.abspath(args.lib), args.session)
    else:
        write_fixture(args.out, record_sessions(os.path.abspath(args.lib), keep=args.keep))


if __name__ == "__main__":
    main()
