"""Build libspecscan.so (HIP, gfx950) in-tree with hipcc. hipcc cross-compiles without a GPU."""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "libspecscan.so")
# the same sources with -DSS_DIAG: implementation choices can be overridden from the environment at ss_create / sc_create.
# Used by the A/B tests and the measurement scripts only; the product library never reads the environment.
LIB_DIAG = os.path.join(CSRC, "libspecscan_diag.so")
SOURCES = ["specscan.hip", "channelizer.hip"]
INCLUDE = os.path.join(HERE, "..", "include")
# every header a library can depend on: what csrc holds (plain file names) and the public headers (relative to csrc, like SOURCES)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + sorted(os.path.join("..", "..", "include", f) for f in os.listdir(INCLUDE) if f.endswith(".h"))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fPIC", "-shared", "-Wall", "-Wno-unused-result"]


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP engine cannot be built (there is no CPU fallback)")


def needs_build(lib: str = LIB) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build_variant(tag: str, defines, force: bool = False, verbose: bool = False) -> str:
    """A/B builds for the measurement scripts: the diagnostics build of this tree, with extra -D switches where an experiment adds
    one (the sources define none of their own any more) -> scripts/ab/libspecscan_<tag>.so (git-ignored; travels to the GPU box).
    How a parent tree's library gets built for a comparison (bench.py --lib). Never loaded by the product."""
    out_dir = os.path.join(HERE, "..", "scripts", "ab")
    os.makedirs(out_dir, exist_ok=True)
    lib = os.path.abspath(os.path.join(out_dir, f"libspecscan_{tag}.so"))
    if force or needs_build(lib):
        cmd = [_hipcc(), *FLAGS, "-DSS_DIAG", *[f"-D{d}" for d in defines], "-o", lib, *[os.path.join(CSRC, s) for s in SOURCES]]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=CSRC)
    return lib


def build_lib(force: bool = False, verbose: bool = False, diag: bool = False) -> str:
    lib = LIB_DIAG if diag else LIB
    if force or needs_build(lib):
        cmd = [_hipcc(), *FLAGS, *(["-DSS_DIAG"] if diag else []), "-o", lib, *[os.path.join(CSRC, s) for s in SOURCES]]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=CSRC)
    return lib


HOST_DIR = os.path.join(HERE, "host")
HOST_LIB = os.path.join(HOST_DIR, "libspecscan_host.so")
# the recording route above the ABI: the two GPU-free classes and the feed recorder that owns them (specscan_replay --record-out)
RECORDING_HEADERS = ("range_planner.h", "recording_store.h", "feed_recorder.h")


def build_host_lib(force: bool = False, verbose: bool = False) -> str:
    """g++ -> host/libspecscan_host.so: the host-side signal tracker, the raw dump files, the range planner and the recording
    store (no GPU code)."""
    srcs = [os.path.join(HOST_DIR, f) for f in ("signal_tracker.cpp", "raw_file.cpp", "recording_host.cpp")]
    deps = srcs + [os.path.join(HOST_DIR, f) for f in ("signal_tracker.h", "raw_file.h", *RECORDING_HEADERS)] + [
        os.path.join(INCLUDE, f) for f in ("specscan_channelizer.h", "specscan_record_feed.h")]
    if force or not os.path.exists(HOST_LIB) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(HOST_LIB):
        cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + INCLUDE, "-o", HOST_LIB,
               *srcs, "-lpthread"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=HOST_DIR)
    return HOST_LIB


REPLAY_TOOL = os.path.join(HOST_DIR, "specscan_replay")


def build_replay_tool(force: bool = False, verbose: bool = False) -> str:
    """g++ -> host/specscan_replay: the C++ replay host (host/replay_main.cpp) linked against libspecscan.so."""
    src = os.path.join(HOST_DIR, "replay_main.cpp")
    tracker = os.path.join(HOST_DIR, "signal_tracker.cpp")
    deps = [src, tracker, os.path.join(HOST_DIR, "raw_file.h"), os.path.join(HOST_DIR, "signal_tracker.h"), os.path.join(HERE, "..", "include", "specscan.h"),
            *[os.path.join(HOST_DIR, f) for f in RECORDING_HEADERS], os.path.join(HERE, "..", "include", "specscan_record_feed.h"),
            os.path.join(HERE, "..", "include", "specscan_channelizer.h"),
            os.path.join(HERE, "..", "include", "specscan_track_feed.h"), os.path.join(HERE, "..", "include", "specscan_track_sparse.h"),
            os.path.join(HERE, "..", "include", "specscan_track_feed_ring.h"),
            os.path.join(HERE, "..", "include", "specscan_spectrogram_feed.h"), os.path.join(HERE, "..", "include", "specscan_spectrogram_feed_ring.h"), LIB]
    if force or not os.path.exists(REPLAY_TOOL) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(REPLAY_TOOL):
        build_lib()
        cmd = [shutil.which("g++") or "g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wpedantic", "-Werror",
               "-I" + os.path.join(HERE, "..", "include"), "-o", REPLAY_TOOL, src, tracker, "-L" + CSRC, "-lspecscan", "-Wl,-rpath,$ORIGIN/../csrc",
               "-Wl,-rpath-link," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib"), "-lpthread"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=HOST_DIR)
    return REPLAY_TOOL


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
    print(build_lib(force=True, verbose=True, diag=True))
    print(build_host_lib(force=True, verbose=True))
    print(build_replay_tool(force=True, verbose=True))
