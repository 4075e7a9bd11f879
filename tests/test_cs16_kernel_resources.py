"""The register budget of the step kernel's CS16 instantiation (8192 points, KIND 0), checked without a GPU as
test_kernel_resources.py checks the CF32 one: hipcc compiles tests/host/cs16_kernel_resources.hip for gfx950 with the product's
code-generation flags. The frame load of 16-bit complex samples (one 4-byte buffer load per sample, both halves sign-extended) must
cost no occupancy and put no scratch access into the frame path."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "cs16_kernel_resources.hip")


def _compile(tmp_path, *extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    import rtl_sdr_scanner_cpp_amd as pkg
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", *extra, SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out


def test_cs16_step_kernel_keeps_the_cf32_budget(tmp_path):
    out = _compile(tmp_path, "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"))
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        if "k_scan_step" not in name:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), spill=get("VGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"), occupancy=get(r"Occupancy \[waves/SIMD\]"))
    assert len(seen) == 1, seen
    (name, r), = seen.items()
    assert name.startswith("_ZN2ss11k_scan_stepILi3E"), name  # FMT_CS16
    assert r["vgprs"] <= 64 and r["occupancy"] == 8, r
    assert r["spill"] <= 18 and r["scratch"] <= 40, r


def test_cs16_frame_path_touches_no_scratch(tmp_path):
    """From the first of the sixteen non-temporal 4-byte frame loads to the dB stores behind the last v_permlane32_swap: no
    spill or reload."""
    asm = tmp_path / "k.s"
    _compile(tmp_path, "-S", "-o", str(asm))
    lines = asm.read_text().splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith("_ZN2ss11k_scan_stepILi3E"))
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i] or lines[i].strip() == "s_endpgm")
    body = lines[start:end]
    loads = [i for i, ln in enumerate(body) if re.search(r"\bbuffer_load_dword\b", ln) and " nt" in ln]
    swaps = [i for i, ln in enumerate(body) if "v_permlane32_swap" in ln]
    assert len(loads) == 16 and swaps, (len(loads), len(swaps))
    assert not any("buffer_load_dwordx2" in ln and " nt" in ln for ln in body)  # (no CF32-sized frame load left in this instantiation)
    stores_after = [i for i, ln in enumerate(body) if i > swaps[-1] and "buffer_store_dword" in ln and "sc1" in ln]
    first, last = loads[0], (stores_after[1] if len(stores_after) > 1 else swaps[-1])
    inside = [ln.strip() for ln in body[first:last + 1] if "scratch_" in ln]
    assert not inside, inside[:4]
