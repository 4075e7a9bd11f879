"""The sparse tracking digest on the CPU (include/specscan_track_digest_sparse.h, csrc/track_digest_sparse.h): the header declares the two
entry points and libspecscan.so cross-compiles and exports them; the ring-row cell address the ring-source kernels read their rel values
through, as a stand-alone program under the sanitizers (tests/host/ring_rows_check.cpp); and the new kernels' resources on gfx950
(tests/host/track_digest_sparse_resources.hip) — every replay instantiation against the stand-alone detect launch, the ring-source
candidates' kernel against k_best_blocked, all built from this tree in the same compile."""
import os
import re
import shutil
import subprocess

import pytest

import rtl_sdr_scanner_cpp_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE = ["st_create_sparse", "st_sparse_stats"]


def test_header_declares_the_two_entry_points_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "specscan_track_digest_sparse.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z]+_[a-z_0-9]+)\s*\(", text)))
    assert names == SPARSE, names
    assert '#include "specscan_track.h"' in text
    assert sorted(pkg.tracker.ST_SPARSE_EXPORTS) == SPARSE
    assert sorted(pkg.tracker.STF_SPARSE_EXPORTS) == ["stf_create_sparse", "stf_sparse_stats"]  # (the feed's list stays as it is)
    pkg.build.build_lib()
    lib = pkg.load_library()
    for name in SPARSE:
        assert hasattr(lib, name), name
    pkg.tracker.bind_track_digest_sparse(lib)
    assert pkg.abi.SS_ABI_VERSION == 3 and pkg.tracker.ST_ABI_VERSION == 1  # (neither ABI moves)
    assert "#define ST_ABI_VERSION 1u" in re.sub(r"[ \t]+", " ", open(os.path.join(ROOT, "include", "specscan_track.h")).read())


def test_ring_rows_check_program_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = tmp_path / "ring_rows_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "ring_rows_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-600:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"ring_rows_check: (\d+) rows, (\d+) cells, bad 0", out.stdout)
    # every bin of a row at 65536 points / logq 3, 131072 / logq 4 and the natural-order sizes, eight kinds of batch each
    assert m and int(m.group(2)) >= 8 * 5 * (65536 + 131072 + 65536 + 8192), out.stdout[-600:]


def _resources(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"),
                          os.path.join(ROOT, "tests", "host", "track_digest_sparse_resources.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), spill=get("VGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"),
                          occupancy=get(r"Occupancy \[waves/SIMD\]"))
    return seen


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    return _resources(tmp_path_factory.mktemp("digest_sparse_resources"))


def _one(seen, part):
    hit = [r for name, r in seen.items() if part in name]
    assert len(hit) == 1, (part, list(seen))
    return hit[0]


@pytest.mark.parametrize("layout", [0, 3, 4])
def test_replay_kernel_costs_no_more_than_the_detect_launch(resources, layout):
    """k_digest_tiles<LAYOUT> may use no more scratch and no fewer waves per SIMD than k_detect_fused<21, 21, 16, 256, false>, measured in
    the same compile.

    Layout 0 (rows in bin order): 61 VGPRs, no scratch, 8 waves per SIMD, the detect launch's own figures. Layouts 3 and 4 (the fold's
    rows): 62 VGPRs, no scratch, 8 waves — the tile takes its 276 columns in two passes there (detect_tile's ONE_FLIGHT = false); in one
    flight, as k_scan_step's fold kinds run it, it needs 124 VGPRs and 4 waves. hipcc for gfx950 at -O3 -fno-slp-vectorize."""
    detect, replay = _one(resources, "k_detect_fused"), _one(resources, f"k_digest_tilesILi{layout}E")
    print(f"k_digest_tiles<{layout}>", replay)
    print("k_detect_fused<21,21,16,256,false>", detect)
    assert replay["scratch"] <= detect["scratch"] and replay["occupancy"] >= detect["occupancy"], (replay, detect)


def test_column_and_ring_source_kernels(resources):
    """k_digest_cols touches no scratch; k_ring_best costs no more scratch than k_best_blocked and, like it, keeps all of its LDS in the
    dynamic region, which the host sizes with blocked_lds_bytes for both; k_ring_tail spills nothing either."""
    cols, ring, blocked, tail = (_one(resources, k) for k in ("k_digest_cols", "k_ring_best", "k_best_blocked", "k_ring_tail"))
    for name, r in (("k_digest_cols", cols), ("k_ring_best", ring), ("k_best_blocked", blocked), ("k_ring_tail", tail)):
        print(name, r)
    assert cols["scratch"] == 0 and cols["spill"] == 0, cols
    assert tail["scratch"] == 0 and tail["spill"] == 0, tail
    assert ring["scratch"] <= blocked["scratch"] and ring["spill"] == 0, (ring, blocked)
    assert ring["lds"] == blocked["lds"] == 0, (ring, blocked)  # (everything in the dynamic region: the host's figure is the whole of it)
    host = open(os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc", "host_track.h")).read()
    launch = re.search(r"void launch_cand_best_of\(.*?\n}\n", host, flags=re.S).group(0)
    assert "hipLaunchKernelGGL(kernel," in launch and "ss::blocked_lds_bytes(r.nrows, a.half)" in launch  # one launch, one LDS figure, both kernels
    assert "launch_cand_best_of(ss::k_ring_best," in host and "launch_cand_best_of(ss::k_best_blocked," in host
    # the tile body and the candidates' body are the shipped ones: track_digest_sparse.h restates neither
    text = open(os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc", "track_digest_sparse.h")).read()
    assert "detect_tile<21, 21, kWatchTF, kWatchCol, false, LAYOUT, false>(a.det" in text and "best_blocked_tile(a," in text and "save_tail_rows(rows," in text
    assert "div_const" not in text and "time_means_to_tile" not in text and "blocked_query" not in text
