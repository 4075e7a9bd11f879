"""The ring spectrogram object on the CPU (include/specscan_spectrogram_feed_ring.h, csrc/spectrogram_rows_ring.h): the header declares
only its two names and the library exports them next to an untouched scan ABI and an untouched sgf_* list; k_spec_rows_ring compiles
for gfx950 without scratch or spills; and the kernel's address functions pass a CPU walk of its load / LDS / walk order against a
restatement of Spectrogram::process / send, as a stand-alone host program under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

import rtl_sdr_scanner_cpp_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = ["sgf_batch_db_rows", "sgf_create_ring"]
SGF = ["sgf_create", "sgf_destroy", "sgf_gate_plan", "sgf_last_error", "sgf_rows"]


def test_header_declares_only_its_two_names():
    text = open(os.path.join(ROOT, "include", "specscan_spectrogram_feed_ring.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z]+_[a-z_0-9]+)\s*\(", text)))
    assert names == RING, names
    assert '#include "specscan_spectrogram_feed.h"' in text and "SGF_ABI_VERSION" not in text  # (no version of its own: sgf_config is unchanged)
    assert sorted(pkg.spectrogram.SGF_RING_EXPORTS) == RING


def test_library_exports_them_and_nothing_else_moved():
    pkg.build.build_lib()
    lib = pkg.load_library()
    for name in RING + SGF:
        assert hasattr(lib, name), name
    assert sorted(pkg.spectrogram.SGF_EXPORTS) == SGF and (pkg.spectrogram.SGF_ABI_VERSION, pkg.spectrogram.SGF_MAX_ROWS) == (1, 64)
    assert not [e for e in pkg.engine.EXPORTS if e.startswith("sgf_")] and pkg.abi.SS_ABI_VERSION == 3  # (the scan ABI is untouched)
    import inspect
    assert "ring" in inspect.signature(pkg.engine.Feed.spectrogram).parameters
    assert "ring" in inspect.signature(pkg.spectrogram.SpectrogramFeed.__init__).parameters
    assert "spectrogram_ring" in inspect.signature(pkg.replay.replay_file).parameters
    assert hasattr(pkg.spectrogram.SpectrogramFeed, "batch_db_rows")
    assert "spectrogram_rows_ring.h" in pkg.build.HEADERS
    assert "specscan_spectrogram_feed_ring.h" in open(os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "build.py")).read().split("def build_replay_tool")[1]


def test_ring_row_kernel_uses_no_scratch(tmp_path):
    """tests/host/spectrogram_rows_ring_resources.hip holds k_spec_rows_ring alone — one form for both radices and every ratio; hipcc
    compiles it for gfx950 with the product's code-generation flags and reports what it uses (the figures are in DESIGN.md)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"),
                          os.path.join(ROOT, "tests", "host", "spectrogram_rows_ring_resources.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), sgprs=get("SGPRs"), spill=get("VGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"),
                          occupancy=get(r"Occupancy \[waves/SIMD\]"))
    print(seen)
    assert len(seen) == 1 and "k_spec_rows_ring" in next(iter(seen)), list(seen)  # one form
    r = next(iter(seen.values()))
    assert r["scratch"] == 0 and r["spill"] == 0, r
    assert r["lds"] <= 40 * 1024, r  # the step's image and its means, 16 KiB each: four workgroups to a CU's 160 KiB


def test_ring_check_program_under_sanitizers(tmp_path):
    """tests/host/spectrogram_rows_ring_check.cpp: logq 3 and 4, every m from 1 to n / 64, cuts at the first frame, the last frame
    and none — the CPU walk of the kernel's order against the reference's arithmetic, bit for bit, built with
    -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "spectrogram_rows_ring_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "host", "spectrogram_rows_ring_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "all ok" in out.stdout and "FAIL" not in out.stdout
