"""Sample ranges in the channeliser and the recorder bound to the feed, without a GPU: the declared and exported names, null
contexts, the host-side planner (csrc/chan_ranges.h) alone under the sanitizers (tests/host/chan_ranges_check.cpp), RangePlanner
against a literal per-frame run of the reference's updateRecordings, and what the in0 / out0 fields cost the kernels on gfx950:
nothing, against the figures of the commit before them (tests/golden/channelizer_resources_parent.json)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import recorder
from rtl_sdr_scanner_cpp_amd.abi import SS_ERR_INVALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRF = ["srf_create", "srf_destroy", "srf_last_error", "srf_record", "srf_release"]


def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_exactly_the_srf_names():
    text = _header("specscan_record_feed.h")
    names = sorted(set(re.findall(r"\b([a-z]+_[a-z_0-9]+)\s*\(", text)))
    assert names == SRF, names
    assert '#include "specscan.h"' in text and '#include "specscan_channelizer.h"' in text
    assert sorted(recorder.SRF_EXPORTS) == SRF
    fields = re.search(r"typedef struct srf_config \{(.*?)\} srf_config;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in recorder.SrfConfig._fields_]
    fields = re.search(r"typedef struct srf_result \{(.*?)\} srf_result;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)[,;]", fields) == [f for f, _ in recorder.SrfResult._fields_]


def test_ranges_are_declared_as_the_abi_says():
    text = _header("specscan_channelizer.h")
    assert re.search(r"#define\s+SC_MAX_RANGES\s+64\b", text) and re.search(r"#define\s+SC_ABI_VERSION\s+1u", text)
    fields = re.search(r"typedef struct sc_range \{(.*?)\} sc_range;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)[,;]", fields) == ["channel", "shift_hz", "begin", "end"] == [f for f, _ in pkg.channelizer.ScRange._fields_]
    assert C.sizeof(pkg.channelizer.ScRange) == 16 and pkg.channelizer.SC_MAX_RANGES == 64
    for name in ("sc_process_ranges", "sc_process_ranges_device"):
        assert re.search(r"int\s+" + name + r"\s*\(\s*sc_ctx\s*\*", text) and name in pkg.channelizer.EXPORTS


def test_library_exports_the_new_names():
    pkg.build.build_lib()
    lib = pkg.channelizer._bind(pkg.load_library())
    for name in SRF + ["sc_process_ranges", "sc_process_ranges_device"]:
        assert hasattr(lib, name), name
    assert not [e for e in pkg.engine.EXPORTS if e.startswith("srf_")] and pkg.abi.SS_ABI_VERSION == 3  # (the scan ABI is untouched)
    assert pkg.channelizer.SC_ABI_VERSION == 1


def test_null_contexts_are_refused():
    pkg.build.build_lib()
    lib = recorder.bind_record_feed(pkg.channelizer._bind(pkg.load_library()))
    cfg = recorder.SrfConfig(recorder.SRF_ABI_VERSION, 16_000, 125, 2, 127.0, 0)
    h = C.c_void_p()
    assert lib.srf_create(None, C.byref(cfg), C.byref(h)) == SS_ERR_INVALID and not h.value
    assert b"null" in lib.srf_last_error(None)
    res = recorder.SrfResult()
    rng = (pkg.channelizer.ScRange * 1)(pkg.channelizer.ScRange(0, 0, 0, 1))
    assert lib.srf_record(None, rng, 1, C.byref(res)) == SS_ERR_INVALID
    assert lib.srf_release(None) == SS_ERR_INVALID
    lib.srf_destroy(None)
    counts = (C.c_int32 * 16)()
    assert lib.sc_process_ranges(None, None, 0, rng, 1, None, None, counts, None, 0) == SS_ERR_INVALID
    assert lib.sc_process_ranges_device(None, None, 0, rng, 1, None, None, counts, None, 0) == SS_ERR_INVALID


def test_planner_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not found")
    exe = tmp_path / "chan_ranges_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "chan_ranges_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1].split()  # sets <n> valid <v> invalid <i> bad <b>
    assert int(last[1]) >= 100_000 and int(last[3]) > 30_000 and int(last[5]) > 10_000 and last[-2:] == ["bad", "0"], last
    assert "chan_ranges.h" in " ".join(pkg.build.HEADERS)


# ---------------------------------------------------------------------------------------------------------------------------
# RangePlanner against the per-frame logic of tests/test_gpu_recorder_bank.py's _model (sdr_device.cpp:103-136), run literally
# ---------------------------------------------------------------------------------------------------------------------------
IDLE = 2**31 - 1
A_, B_, C_, D_ = 100_000, -250_000, 30_000, -40_000


def _script(g):
    """The tracker's list of global frame g: A spans three batches and flushes now and then; B starts and stops inside a batch;
    C takes B's slot in the frame B leaves it (a retune in mid-batch); D finds no free slot, and one later."""
    want = []
    if 2 <= g < 20:
        want.append((A_, g % 5 == 0))
    if 4 <= g < 6:
        want.append((B_, False))
    if 6 <= g < 11:
        want.append((C_, g in (8, 10)))
    if 7 <= g < 10 or 12 <= g < 14:
        want.append((D_, True))
    return want


def _literal(nslots, lists):
    """Per frame: which slot records which shift in it, and the flushes and stops in front of it."""
    slots = [dict(rec=False, shift=IDLE) for _ in range(nslots)]
    member, flushes, stops, ignored = [], [], [], set()
    for g, want in enumerate(lists):
        shifts = [s for s, _ in want]
        for k, s in enumerate(slots):
            if s["rec"] and s["shift"] not in shifts:
                s.update(rec=False, shift=IDLE)
                stops.append((k, g))
        for shift, flush in want:
            hit = [k for k, s in enumerate(slots) if s["shift"] == shift]
            if hit:
                if flush:
                    flushes.append((hit[0], g))
            else:
                free = [k for k, s in enumerate(slots) if not s["rec"]]
                if free:
                    slots[free[0]].update(rec=True, shift=shift)
                else:
                    ignored.add(shift)
        member.append({k: s["shift"] for k, s in enumerate(slots) if s["rec"]})
    return member, flushes, stops, ignored


def test_range_planner_against_the_literal_per_frame_run():
    n, nslots, batches = 256, 2, [(0, 8), (8, 16), (16, 24)]
    lists = [_script(g) for g in range(24)]
    member, flushes, stops, ignored = _literal(nslots, lists)
    assert ignored == {D_} and any(m.get(1) == D_ for m in member)  # D found no slot, and one later
    assert [m.get(1) for m in member[4:7]] == [B_, B_, C_]  # the retune in mid-batch
    assert all(m.get(0) == A_ for m in member[2:20]) and len(flushes) >= 4
    planner = recorder.RangePlanner(nslots, n)
    got_member = [dict() for _ in range(24)]
    got_stops, per_slot = [], {k: [] for k in range(nslots)}
    for a, b in batches:
        ranges, ends, flushed = planner.plan(lists[a:b])
        assert len(ranges) == len(ends) == len(flushed) <= recorder.SC_MAX_RANGES
        for (k, shift, begin, end), why, fl in zip(ranges, ends, flushed):
            assert begin % n == 0 and end % n == 0 and 0 <= begin <= end <= (b - a) * n
            for f in range(begin // n, end // n):
                assert k not in got_member[a + f]
                got_member[a + f][k] = shift
            if why == "stop":
                got_stops.append((k, a + end // n))
            else:
                assert why == "batch" and end == (b - a) * n
            # the range ends with a flush: the literal run flushed this slot in front of the range's last frame
            assert fl == (end > begin and (k, a + end // n - 1) in flushes), (k, shift, begin, end, why, fl)
            per_slot[k].append((a * n + begin, a * n + end, shift, why, fl))
        for k in range(nslots):  # what sc_process_ranges asks of one channel's ranges
            mine = [r for r in ranges if r[0] == k]
            assert all(p[3] <= q[2] for p, q in zip(mine, mine[1:]))
    assert got_member == member
    assert sorted(got_stops) == sorted(stops)
    for k, rs in per_slot.items():  # merged: two ranges of a slot abut on one shift only at a batch edge
        for p, q in zip(rs, rs[1:]):
            if p[1] == q[0] and p[2] == q[2]:
                assert p[3] == "batch", (k, p, q)
    a_ranges = [r for r in per_slot[0] if r[2] == A_]
    assert [(r[0] // n, r[1] // n, r[3]) for r in a_ranges] == [(2, 8, "batch"), (8, 16, "batch"), (16, 20, "stop")]  # one recording through three batches
    assert [r[4] for r in a_ranges] == [False, True, False]  # A flushes in frames 5, 10 and 15: only 15 is a range's last frame
    assert any(r[4] for r in per_slot[1]) and planner.ignored == set()


# ---------------------------------------------------------------------------------------------------------------------------
# kernel resources
# ---------------------------------------------------------------------------------------------------------------------------
def test_first_stage_kernels_cost_what_they_cost_before_the_ranges(tmp_path):
    """hipcc -Rpass-analysis=kernel-resource-usage on csrc/channelizer.hip with the product's code-generation flags, beside the
    same figures of the commit before in0 / out0 (recorded with the same command): every first-stage kernel in all four formats
    keeps scratch 0 and loses no wave per SIMD. Both columns are printed."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    parent = json.load(open(os.path.join(ROOT, "tests", "golden", "channelizer_resources_parent.json")))
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"),
                          os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc", "channelizer.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), scratch=get(r"ScratchSize \[bytes/lane\]"), occupancy=get(r"Occupancy \[waves/SIMD\]"))
    first = [k for k in seen if "k_chan_dec" in k or "k_chan_stageILb1" in k or "k_chan_keepILb1" in k]
    assert len(first) == 4 * (1 + 8 + 1 + 1), sorted(first)  # per format: k_chan_dec<6,1>, 4 x 2 k_chan_dec_split, k_chan_stage<true>, k_chan_keep<true>
    assert set(seen) == set(parent), set(seen) ^ set(parent)  # no kernel renamed, added or dropped
    print(f"{'kernel':76s} parent (VGPRs, scratch, waves/SIMD) -> this tree")
    for k in sorted(seen):
        p, s = parent[k], seen[k]
        print(f"{k:76s} {p['vgprs']:4d} {p['scratch']:3d} {p['occupancy']:2d}  -> {s['vgprs']:4d} {s['scratch']:3d} {s['occupancy']:2d}")
    for k in first:
        assert seen[k]["scratch"] == 0 and parent[k]["scratch"] == 0, (k, seen[k])
        assert seen[k]["occupancy"] >= parent[k]["occupancy"], (k, seen[k], parent[k])
