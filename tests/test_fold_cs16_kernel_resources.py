"""The register budget of the fold's CS16 instantiations (k_scan_step KIND 8 / 9, FMT_CS16), checked without a GPU as
test_cs16_kernel_resources.py checks the 8192-point one: hipcc compiles tests/host/fold_cs16_kernel_resources.hip for gfx950 with the
product's code-generation flags. They must keep what the int8 fold has: at most 128 VGPRs, four waves per SIMD, no spill, no scratch.
The CS16 pieces go through the two 16 KiB halves of the exchange plane as the int8 ones do, so the launch's LDS size is unchanged."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "fold_cs16_kernel_resources.hip")


def test_cs16_fold_kernels_keep_the_int8_fold_budget(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    import rtl_sdr_scanner_cpp_amd as pkg
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"), SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        if "k_scan_step" not in name:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), spill=get("VGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"), occupancy=get(r"Occupancy \[waves/SIMD\]"),
                          lds=get(r"LDS Size \[bytes/block\]"))
    print(seen)
    assert sorted(seen) == ["_ZN2ss11k_scan_stepILi3ELb0ELi2ELb1ELb0ELi8EEEvNS_8StepArgsE", "_ZN2ss11k_scan_stepILi3ELb0ELi2ELb1ELb0ELi9EEEvNS_8StepArgsE"], list(seen)  # FMT_CS16, KIND 8 and 9
    for name, r in seen.items():
        assert r["vgprs"] <= 128 and r["occupancy"] == 4, (name, r)
        assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["lds"] == 0, (name, r)  # (dynamic LDS only: kStepLdsBytes at launch, as for every form of the step kernel)
    text = open(os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc", "fold_cs16_staging.h")).read()
    assert re.search(r"kFoldCs16PieceBytes = 16384;", text)  # two pieces = the exchange plane's two halves
