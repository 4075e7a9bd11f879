"""Where a digest finds its batch's rows (csrc/rows_source.h: decide_rows_source), checked on the CPU: tests/host/rows_source_check.cpp, a
stand-alone program under the address and undefined-behaviour sanitizers, holds every combination of dB plane / ring rows / fold
order / radix to a table written out by hand. The header has no HIP in it; st_digest and stf_enqueue both call it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc")


def test_rows_source_check_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = tmp_path / "rows_source_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "rows_source_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"rows_source_check: (\d+) combinations, bad 0", out.stdout)
    assert m and int(m.group(1)) >= 24 + 64, out.stdout[-600:]


def test_the_header_has_no_hip_and_both_digests_ask_it():
    text = open(os.path.join(CSRC, "rows_source.h")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower() and "#include" not in text
    for name in ("host_track.h", "host_track_feed.h"):
        assert "ss::decide_rows_source(" in open(os.path.join(CSRC, name)).read(), name
