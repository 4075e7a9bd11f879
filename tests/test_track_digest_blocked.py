"""The blocked sliding arg-max of the tracking digest (csrc/track_digest_blocked.h) on the CPU: the header's own table build and query,
compiled for the host with the sanitizers and run with the 256 lanes played by loops, against std::max_element written out
(tests/host/blocked_argmax_check.cpp); the kernel's resources on gfx950 (no scratch, no spills; the figures are in DESIGN.md); and the
wide recording bandwidths the kernel now admits on the ORACLE's planes: the numpy restatement (tests/digest_ref.py) through the host
tracker's digest form must give, frame by frame, what process_batch gives on the planes. Integers and copies of plane floats: equality,
no tolerance."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from digest_ref import DigestRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTER = 145_000_000


def test_table_build_and_query_against_the_literal_walk(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not found")
    exe = tmp_path / "blocked_argmax_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "blocked_argmax_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1]
    assert last.endswith("bad 0") and int(last.split()[1]) > 100_000, last


def test_blocked_kernel_uses_no_scratch(tmp_path):
    """tests/host/track_digest_blocked_resources.hip instantiates the kernel; hipcc compiles it for gfx950 with the product's
    code-generation flags and reports what it uses."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"),
                          os.path.join(ROOT, "tests", "host", "track_digest_blocked_resources.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), sgprs=get("TotalSGPRs"), spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"),
                          lds=get(r"LDS Size \[bytes/block\]"), occupancy=get(r"Occupancy \[waves/SIMD\]"))
    new = {name: r for name, r in seen.items() if "blocked" in name}
    print(new)
    assert len(new) == 1 and "k_best_blocked" in next(iter(new)), list(seen)
    for name, r in new.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] == 0, (name, r)  # (everything in the dynamic region: the host's LDS figure is the whole of it)


def _batches(nframes, sizes):
    edges, k = [0], 0
    while edges[-1] < nframes:
        edges.append(min(nframes, edges[-1] + sizes[k % len(sizes)]))
        k += 1
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("n,g,nframes,sizes,min_cand,min_tx", [(256, 600, 150, (7, 64, 1, 30), 100, 50), (2048, 1100, 120, (7, 64, 1, 30), 1000, 50),
                                                              (8192, 2048, 100, (7, 64, 1, 100), 1000, 50), (8192, 4096, 100, (7, 64, 1, 100), 1000, 50)])
def test_wide_windows_digest_form_matches_the_planes(oracle_mod, n, g, nframes, sizes, min_cand, min_tx):
    """Recording bandwidths of 600 to 4096 bins (the walk stopped near 977): the restatement and the digest form take them as the
    plane tracker does. g = 600 at n = 256 clips every window on both sides."""
    O = oracle_mod
    fs = 250 * n
    iq = pkg.synth.SyntheticBand(n, seed=5, on_frame=30, off_frame=10_000).frames_cf32(nframes)
    t = (1_000 + 40 * np.arange(nframes)).astype(np.int64)
    O.lib().orc_set_fft_backend(0)
    r = O.oracle_chain(fs, CENTER, fft_size=n, decim=1, max_batch=nframes, learn_ms=280).process(iq, t_ms=t)
    tk = dict(group_size=g, min_time_ms=200, timeout_ms=400)
    planes = pkg.tracker.SignalTracker(n, fs, **tk).process_batch(t, r["avg"], r["rel"], r["cand_off"], r["cand_idx"])
    tr = pkg.tracker.SignalTracker(n, fs, **tk)
    ref = DigestRef(n, g, tr.start_level)
    off, idx = r["cand_off"].astype(np.int64), r["cand_idx"]
    got = []
    for a, b in _batches(nframes, sizes):
        d = ref.digest(r["rel"][a:b], r["avg"][a:b], off[a:b + 1] - off[a], idx[off[a]:off[b]], tr.keys)
        got.extend(tr.process_batch_digest(t[a:b], d))
    assert len(got) == nframes
    for f in range(nframes):
        for k in (0, 1):
            np.testing.assert_array_equal(got[f][k], planes[f][k], err_msg=f"frame {f}: digest form vs process_batch")
    ncand, ntx = int(off[nframes]), sum(len(x[0]) for x in got)
    print(f"n {n} g {g}: {ncand} candidates, {ntx} transmissions")
    assert ncand > min_cand and ntx > min_tx, (ncand, ntx)
