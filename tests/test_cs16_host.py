"""CS16 input (interleaved little-endian int16 I,Q) on the host side, CPU only: the public header's format code, dump names,
re-framing of .cs16 dumps, the replay overrides, the synthetic generator and the GNU Radio adapter's item size."""
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHEN = time.struct_time((2025, 3, 7, 9, 5, 1, 0, 0, -1))


def test_header_format_code_matches_python():
    text = open(os.path.join(ROOT, "include", "specscan.h")).read()
    m = re.search(r"SS_FMT_CS16\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 3 == pkg.abi.SS_FMT_CS16
    assert pkg.abi.SS_FMT_BYTES[pkg.abi.SS_FMT_CS16] == 4
    assert re.search(r"#define SS_ABI_VERSION 3\b", text)  # a new format code, the same struct: no ABI bump


@pytest.mark.parametrize("name", ["./full_20250307_090501_145000000_2048000_cs16.raw", "recording_20250307_090501_145000000_2048000.cs16",
                                  "/tmp/x/full_20250307_090501_145000000_2048000_fc.cs16"])
def test_cs16_names_parse(name):
    info = replay.parse_raw_file_name(name)
    assert info.kind == replay.KIND_CS16 == 4
    assert info.frequency == 145_000_000 and info.sample_rate == 2_048_000


def test_engine_overrides_for_cs16():
    info = replay.parse_raw_file_name(replay.make_raw_file_name("full", "cs16", 145_000_000, 2_048_000, WHEN))
    ov = replay.engine_overrides_for(info)
    assert ov == {"in_format": pkg.abi.SS_FMT_CS16, "int_scale": 1.0 / 32768}


@pytest.mark.parametrize("decim", [1, 3])
def test_reader_reframes_cs16(tmp_path, decim):
    n, items = 64, 7
    rng = np.random.default_rng(5)
    stream = rng.integers(-32768, 32768, size=(items * n * decim + 17, 2), dtype=np.int64).astype(np.int16)  # a trailing partial item
    path = tmp_path / replay.make_raw_file_name("full", "cs16", 145_000_000, 2_048_000, WHEN)[2:]
    stream.tofile(path)
    r = replay.RawIqReader(str(path), replay.KIND_CS16, n, decim)
    assert r.items == items
    got = r.read(items + 5)
    assert got.dtype == np.int16 and got.shape == (items, n, 2)
    want = stream[: items * n * decim].reshape(items, n * decim, 2)[:, :n]
    np.testing.assert_array_equal(got, want)
    assert r.read(4).shape[0] == 0
    r.close()


def test_frames_cs16_rounds_and_saturates():
    band = pkg.synth.SyntheticBand(256, seed=3, on_frame=0, off_frame=100)
    x = pkg.synth.SyntheticBand(256, seed=3, on_frame=0, off_frame=100).frames_cf32(4)
    q = band.frames_cs16(4, full_scale=0.01)  # a tiny full scale: most values clip
    assert q.dtype == np.int16 and q.shape == (4, 256, 2)
    y = np.stack([x.real, x.imag], axis=-1).astype(np.float64) * (32768.0 / 0.01)
    np.testing.assert_array_equal(q, np.clip(np.rint(y), -32768, 32767).astype(np.int16))
    assert (q == 32767).any() and (q == -32768).any()


ITEM_MAIN = r"""
#include <gpu_spectrum_block.h>
#include <cstdio>
int main() {
  ss_config cfg;
  cfg.fft_size = 8192;
  cfg.decim = 5;
  const int fmts[4] = {SS_FMT_CF32, SS_FMT_CS8, SS_FMT_CU8, SS_FMT_CS16};
  for (int f : fmts) {
    cfg.in_format = f;
    printf("%d %d\n", f, GpuSpectrum::inputItemBytes(cfg));
  }
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_adapter_input_item_follows_format(tmp_path):
    src = tmp_path / "item.cpp"
    src.write_text(ITEM_MAIN)
    exe = tmp_path / "item"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wpedantic", "-I" + os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "host"),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle", "stubs"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {int(a): int(b) for a, b in (ln.split() for ln in out if ln)}
    assert got[0] == 8 * 8192 * 5  # sizeof(gr_complex) * N * D, as before
    assert got[3] == 4 * 8192 * 5
    assert got[1] == got[2] == 2 * 8192 * 5
