"""Recording from a decimated scan, without a GPU: the whole-item feed (ss_feed_create_items), the channeliser entry that uploads
only what its ranges read (sc_process_ranges_upload) and srf_result's upload count are declared, listed and exported, null
contexts are refused, and the interval plan of the upload (csrc/chan_ranges.h: upload_intervals, item_samples) passes its
stand-alone check (tests/host/chan_upload_check.cpp) under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import recorder
from rtl_sdr_scanner_cpp_amd.abi import SS_ERR_INVALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEED_ARGS = r"\(\s*ss_ctx\s*\*\s*\w*,\s*int32_t\s+depth,\s*int32_t\s+cand_cap,\s*int32_t\s+want_psd,\s*ss_feed\s*\*\*\s*out\s*\)"


def _header(name):
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_items_feed_is_declared_listed_and_exported():
    text = _header("specscan.h")
    assert re.search(r"int\s+ss_feed_create_items\s*" + FEED_ARGS, text)
    assert re.search(r"int\s+ss_feed_create\s*" + FEED_ARGS, text)  # the same arguments
    assert "ss_feed_create_items" in pkg.engine.EXPORTS
    pkg.build.build_lib()
    lib = pkg.load_library()
    assert hasattr(lib, "ss_feed_create_items")
    assert pkg.abi.SS_ABI_VERSION == 3
    # the footprint of the pinned slots is stated where the entry is described
    raw = open(os.path.join(ROOT, "include", "specscan.h")).read()
    assert re.search(r"depth \* max_batch \* N \* decim \* bytes per sample", raw)


def test_the_upload_entry_is_declared_listed_and_exported():
    text = _header("specscan_channelizer.h")
    m = re.search(r"int\s+sc_process_ranges_upload\s*\(\s*sc_ctx\s*\*\s*\w+,\s*const\s+void\s*\*\s*iq,(.*?)\)\s*;", text, flags=re.S)
    assert m and re.search(r"uint64_t\s*\*\s*uploaded_bytes\s*$", m.group(1))
    dev = re.search(r"int\s+sc_process_ranges_device\s*\(\s*sc_ctx\s*\*\s*\w+,\s*const\s+void\s*\*\s*d_iq,(.*?)\)\s*;", text, flags=re.S).group(1)
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    assert squeeze(m.group(1)) == squeeze(dev) + ", uint64_t* uploaded_bytes"  # the device form's arguments, and the count
    assert "sc_process_ranges_upload" in pkg.channelizer.EXPORTS and pkg.channelizer.SC_ABI_VERSION == 1
    pkg.build.build_lib()
    lib = pkg.channelizer._bind(pkg.load_library())
    assert hasattr(lib, "sc_process_ranges_upload")
    assert hasattr(pkg.channelizer.Channelizer, "process_ranges_upload")


def test_the_result_ends_in_the_upload_count():
    text = _header("specscan_record_feed.h")
    fields = re.search(r"typedef struct srf_result \{(.*?)\} srf_result;", text, flags=re.S).group(1)
    names = re.findall(r"(\w+)[,;]", fields)
    assert names[-1] == "h2d_bytes" and re.search(r"uint64_t\s+h2d_bytes\s*;\s*$", fields)
    assert recorder.SrfResult._fields_[-1] == ("h2d_bytes", C.c_uint64)
    assert names == [f for f, _ in recorder.SrfResult._fields_]
    assert len(recorder.SrfConfig._fields_) == 6  # built positionally with six values
    assert re.search(r"#define\s+SRF_ABI_VERSION\s+2u", text) and recorder.SRF_ABI_VERSION == 2
    raw = open(os.path.join(ROOT, "include", "specscan_record_feed.h")).read()
    assert "ss_feed_create_items" in raw and "must have decim == 1" not in raw


def test_null_contexts_are_refused():
    pkg.build.build_lib()
    lib = pkg.channelizer._bind(pkg.load_library())
    h = C.c_void_p()
    assert lib.ss_feed_create_items(None, 2, 16, 0, C.byref(h)) == SS_ERR_INVALID and not h.value
    rng = (pkg.channelizer.ScRange * 1)(pkg.channelizer.ScRange(0, 0, 0, 1))
    counts = (C.c_int32 * 16)()
    up = C.c_uint64(77)
    assert lib.sc_process_ranges_upload(None, None, 0, rng, 1, None, None, counts, None, 0, C.byref(up)) == SS_ERR_INVALID
    assert up.value == 77  # a refused call changes nothing
    assert lib.sc_process_ranges_upload(None, None, 0, rng, 1, None, None, counts, None, 0, None) == SS_ERR_INVALID


def test_python_takes_the_items_switch():
    import inspect
    assert inspect.signature(pkg.SpectrumEngine.feed).parameters["items"].default is False
    assert inspect.signature(pkg.replay.replay_file).parameters["items"].default is False
    assert list(inspect.signature(pkg.engine.Feed.__init__).parameters)[:5] == ["self", "engine", "depth", "cand_cap", "want_psd"]


def test_interval_plan_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not found")
    exe = tmp_path / "chan_upload_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "chan_upload_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1].split()  # hand <n> random <n> intervals <n> bad <b>
    assert int(last[1]) >= 12 and int(last[3]) >= 3_000 and int(last[5]) > int(last[3]) and last[-2:] == ["bad", "0"], last
    assert "chan_ranges.h" in " ".join(pkg.build.HEADERS)
