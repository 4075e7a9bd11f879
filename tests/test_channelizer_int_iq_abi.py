"""Integer IQ input of the recorder channeliser (sc_set_input_format), checked without a GPU: the entry point is declared,
exported and bound, refuses a null context, and every first-stage kernel exists for all four input formats with an integer
instantiation that costs no scratch and no occupancy against its CF32 sibling (hipcc compiles csrc/channelizer.hip for gfx950
with the product's code-generation flags, as tests/test_cs16_kernel_resources.py does for the scan step)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import rtl_sdr_scanner_cpp_amd as pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc", "channelizer.hip")
FORMATS = (pkg.abi.SS_FMT_CF32, pkg.abi.SS_FMT_CS8, pkg.abi.SS_FMT_CU8, pkg.abi.SS_FMT_CS16)
SS_ERR_INVALID = -1


def test_set_input_format_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "specscan_channelizer.h")).read()
    assert re.search(r"int\s+sc_set_input_format\s*\(\s*sc_ctx\s*\*\s*ctx\s*,\s*int32_t\s+in_format\s*,\s*float\s+int_scale\s*\)\s*;", text)
    assert "sc_set_input_format" in pkg.channelizer.EXPORTS
    lib = pkg.channelizer._bind(pkg.load_library())
    assert hasattr(lib, "sc_set_input_format")
    assert lib.sc_set_input_format.argtypes == [C.c_void_p, C.c_int32, C.c_float]


def test_set_input_format_refuses_a_null_context():
    lib = pkg.channelizer._bind(pkg.load_library())
    for fmt in FORMATS:
        assert lib.sc_set_input_format(None, fmt, 0.0) == SS_ERR_INVALID
    assert lib.sc_set_input_format(None, 7, 0.0) == SS_ERR_INVALID


def _resources(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "c.o"), SRC],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), scratch=get(r"ScratchSize \[bytes/lane\]"), occupancy=get(r"Occupancy \[waves/SIMD\]"))
    return seen


def _first_stage_names(fmt):
    """Mangled names of the eleven kernels that read the raw stream, for one ss_format."""
    ns, args = "_ZN12_GLOBAL__N_1", "EEEvNS_8ChanArgsE"
    names = [f"{ns}10k_chan_decILi{fmt}ELi6ELi1{args}"]  # merged <6,1>
    for logg, passes in ((3, 1), (4, 1), (5, 1), (6, 2)):  # split forms, edge and full-tile
        names += [f"{ns}16k_chan_dec_splitILi{fmt}ELi{logg}ELi{passes}ELb{full}{args}" for full in (0, 1)]
    names += [f"{ns}12k_chan_stageILb1ELi{fmt}{args}", f"{ns}11k_chan_keepILb1ELi{fmt}{args}"]  # generic first stage, history
    return names


def test_every_first_stage_kernel_exists_per_format_and_integers_cost_nothing(tmp_path):
    seen = _resources(tmp_path)
    for fmt in FORMATS:
        for name in _first_stage_names(fmt):
            assert name in seen, (name, sorted(seen))
    for fmt in FORMATS[1:]:
        for name, sibling in zip(_first_stage_names(fmt), _first_stage_names(pkg.abi.SS_FMT_CF32)):
            r, base = seen[name], seen[sibling]
            assert r["scratch"] == 0, (name, r)
            assert r["occupancy"] >= base["occupancy"], (name, r, base)
