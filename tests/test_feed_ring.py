"""The pipelined feed's slot ring without a GPU: csrc/feed_ring.h is plain C++ (no HIP include), and its stand-alone check
(tests/host/feed_ring_check.cpp: the transitions by hand at depth 2 and 8, and a seeded random walk against a queue with and without
a recorder) passes under the sanitizers. The host-side headers specscan.hip ends in are among the library's dependencies."""
import os
import re
import shutil
import subprocess

import pytest

import rtl_sdr_scanner_cpp_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc")
HOST_HEADERS = ["device_buffers.h", "feed_ring.h", "host_feed.h", "host_track.h", "host_track_feed.h", "host_record_feed.h", "host_spectrogram_feed.h"]


def test_the_ring_is_plain_cpp():
    text = open(os.path.join(CSRC, "feed_ring.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", text) and "hipError_t" not in text
    for state in ("free", "acquired", "submitted", "held"):
        assert re.search(r"enum class slot_state \{[^}]*\b" + state + r"\b", text)


def test_ring_check_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not found")
    exe = tmp_path / "feed_ring_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "feed_ring_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1].split()  # cases <n> ops <n> refused <n> collected <n> bad <b>
    assert last[0::2] == ["cases", "ops", "refused", "collected", "bad"], last
    cases, ops, refused, collected = (int(v) for v in last[1:8:2])
    assert cases >= 40 and ops >= 4_000 and refused > 100 and collected > 1_000 and last[-2:] == ["bad", "0"], last


def test_the_host_headers_are_dependencies_of_the_library():
    for name in HOST_HEADERS:
        assert os.path.exists(os.path.join(CSRC, name)) and name in pkg.build.HEADERS, name
    tail = open(os.path.join(CSRC, "specscan.hip")).read().rsplit('}  // extern "C"', 1)[1]
    assert re.findall(r'#include "(\w+\.h)"', tail) == HOST_HEADERS  # specscan.hip ends in them, in this order
    assert "spectrogram_rows.h" in pkg.build.HEADERS and "chan_ranges.h" in " ".join(pkg.build.HEADERS)
    assert all(os.path.exists(os.path.join(CSRC, h)) for h in pkg.build.HEADERS)
