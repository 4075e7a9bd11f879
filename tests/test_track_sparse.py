"""The sparse tracked feed on the CPU (include/specscan_track_sparse.h, csrc/track_sparse.h): the header declares the two entry points
and libspecscan.so cross-compiles and exports them; the window -> tile-column arithmetic the replay marks its columns with, as a
stand-alone program under the sanitizers (tests/host/watch_cols_check.cpp); and the replay kernel's resources on gfx950 against the
stand-alone detect launch whose tile it runs, both built from this tree in the same compile (tests/host/track_sparse_resources.hip)."""
import os
import re
import shutil
import subprocess

import pytest

import rtl_sdr_scanner_cpp_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE = ["stf_create_sparse", "stf_sparse_stats"]


def test_header_declares_the_two_entry_points_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "specscan_track_sparse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z]+_[a-z_0-9]+)\s*\(", text)))
    assert names == SPARSE, names
    assert '#include "specscan_track_feed.h"' in text
    assert sorted(pkg.tracker.STF_SPARSE_EXPORTS) == SPARSE
    pkg.build.build_lib()
    lib = pkg.load_library()
    for name in SPARSE:
        assert hasattr(lib, name), name
    pkg.tracker.bind_track_sparse(lib)
    assert pkg.abi.SS_ABI_VERSION == 3 and pkg.tracker.STF_ABI_VERSION == 1  # (neither ABI moves)


def test_watch_cols_check_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = tmp_path / "watch_cols_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "watch_cols_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"watch_cols_check: (\d+) windows, (\d+) lists, bad 0", out.stdout)
    assert m and int(m.group(1)) >= 4 * 8 * 300 and int(m.group(2)) >= 4 * 8 * 20, out.stdout[-600:]


def test_replay_kernel_costs_no_more_than_the_detect_launch(tmp_path):
    """k_watch_tiles may use no more scratch and no fewer waves per SIMD than k_detect_fused<21, 21, 16, 256, false>, measured in the same
    compile; k_feed_watch_cols touches no scratch at all."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"),
                          os.path.join(ROOT, "tests", "host", "track_sparse_resources.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), spill=get("VGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"),
                          occupancy=get(r"Occupancy \[waves/SIMD\]"))
    one = lambda part: [r for name, r in seen.items() if part in name]  # noqa: E731
    replay, detect, cols = one("k_watch_tiles"), one("k_detect_fused"), one("k_feed_watch_cols")
    assert len(replay) == len(detect) == len(cols) == 1, list(seen)
    print("k_watch_tiles", replay[0])
    print("k_detect_fused<21,21,16,256,false>", detect[0])
    print("k_feed_watch_cols", cols[0])
    assert replay[0]["scratch"] <= detect[0]["scratch"] and replay[0]["occupancy"] >= detect[0]["occupancy"], (replay[0], detect[0])
    assert cols[0]["scratch"] == 0 and cols[0]["spill"] == 0, cols[0]
    # the tile body is the scan's own: track_sparse.h restates none of it
    text = open(os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc", "track_sparse.h")).read()
    assert "detect_tile<21, 21, kWatchTF, kWatchCol, false>(a.det" in text and "div_const" not in text and "time_means_to_tile" not in text
