"""Recorder channeliser fed CS8 / CU8 / CS16 IQ (sc_set_input_format) on the GPU. Run with -m gpu.

The integer path must equal, bit for bit, the CF32 path fed the exact fp32 conversion (x - offset) * scale, at every
first-stage form, under start / stop / restart and format switches, from the device entry point, and when one device
upload of the receiver's native stream feeds the scan chain and the channeliser at once; the C++ RecorderBank publishes the
same records. One case per format ties the claim to the CPU oracle (oracle/channelizer_oracle.c), which stays CF32."""
import json
import os
import subprocess

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import abi as A
from rtl_sdr_scanner_cpp_amd.channelizer import Channelizer
from chan_ref import first_stage
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (format, int_scale as passed, numpy dtype, offset, resolved scale)
FORMATS = {
    "cs8": (A.SS_FMT_CS8, 0.0, np.int8, 0.0, np.float32(1.0) / np.float32(128.0)),
    "cu8": (A.SS_FMT_CU8, 0.0, np.uint8, 127.5, np.float32(1.0) / np.float32(127.5)),
    "cs16": (A.SS_FMT_CS16, 0.0, np.int16, 0.0, np.float32(1.0) / np.float32(32768.0)),
    "cs16_12bit": (A.SS_FMT_CS16, 1.0 / 2048.0, np.int16, 0.0, np.float32(1.0 / 2048.0)),
}


def _ints(n, fs, name, seed):
    """A receiver's native stream: noise plus modulated carriers at fs/7 and -fs/5, quantised to the format (the 12-bit case
    keeps its samples within +-2047), with a few samples at the extremes of the type."""
    _fmt, _s, dt, off, _scale = FORMATS[name]
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.05
    for k, f in enumerate((fs / 7.0, -fs / 5.0)):
        x += 0.25 * np.exp(2j * np.pi * (f * t + 0.3 * np.sin(2 * np.pi * (900 + 400 * k) * t)))
    full = {"cs8": 127.0, "cu8": 127.5, "cs16": 32767.0, "cs16_12bit": 2047.0}[name]
    info = np.iinfo(dt)
    y = np.stack([x.real, x.imag], axis=-1) * full + off
    q = np.clip(np.rint(y), info.min, info.max).astype(dt)
    q[rng.integers(0, n, 16)] = info.min
    q[rng.integers(0, n, 16)] = info.max
    return q


def _to_cf32(q, name):
    """The exact conversion the library applies: (x - offset) * scale in fp32."""
    _fmt, _s, _dt, off, scale = FORMATS[name]
    y = (q.astype(np.float32) - np.float32(off)) * np.float32(scale)
    return np.ascontiguousarray(y).view(np.complex64).reshape(-1)


def _pair(fs, bw, name, channels, max_samples):
    fmt, s, *_ = FORMATS[name]
    ci = Channelizer(fs, bw, in_format=fmt, int_scale=s, channels=channels, max_samples=max_samples)
    cf = Channelizer(fs, bw, channels=channels, max_samples=max_samples)
    return ci, cf


def _same(a, b, what):
    """Byte-for-byte equality of two process() results: the same slots, counts, int8 and cf32 bytes."""
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k][0].shape == b[k][0].shape, (what, k, a[k][0].shape, b[k][0].shape)
        assert a[k][0].tobytes() == b[k][0].tobytes(), (what, k, "int8")
        if a[k][1] is not None or b[k][1] is not None:
            assert a[k][1].tobytes() == b[k][1].tobytes(), (what, k, "cf32", np.abs(a[k][1] - b[k][1]).max())


CASES = [  # (fs, bw, stages (interp, decim), first-stage form)
    (2_048_000, 32_000, [(1, 64)], "<6,1>"),
    (2_048_000, 16_000, [(1, 8), (1, 16)], "<3,1>"),
    (250_000, 25_000, [(1, 10)], "<4,1>"),
    (1_024_000, 32_000, [(1, 32)], "<5,1>"),
    (2_400_000, 32_000, [(1, 75)], "<6,2>"),
    (1_000_000, 16_000, [(2, 125)], "generic"),
    (1_024_000, 20_000, [(1, 16), (5, 16)], "<4,1>"),  # interpolating second stage
]
CALLS = (1, 777, 5_003, 1 << 16, 23_456, 3)  # one sample, below and above a tile, max_samples, ragged ends


@pytest.mark.parametrize("name", list(FORMATS))
@pytest.mark.parametrize("fs,bw,stages,form", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_integer_input_is_bit_identical_to_cf32(fs, bw, stages, form, name):
    n = sum(CALLS)
    q = _ints(n, fs, name, seed=fs // 1000 + bw // 1000)
    x = _to_cf32(q, name)
    ci, cf = _pair(fs, bw, name, channels=4, max_samples=1 << 16)
    assert [(i, d) for i, d, _ in ci.stages] == stages and first_stage(ci.stages).form == form
    for ch in (ci, cf):  # three active slots, slot 2 idle
        ch.start(0, int(fs / 7))
        ch.start(1, int(-fs / 5))
        ch.start(3, 0)
    pos, total = 0, 0
    for size in CALLS:
        a = ci.process(q[pos:pos + size])
        b = cf.process(x[pos:pos + size])
        _same(a, b, (name, fs, bw, size))
        assert sorted(a) == [0, 1, 3]
        total += len(a[0][0])
        pos += size
    assert total >= n * bw // fs - 2
    ci.close()
    cf.close()


@pytest.mark.parametrize("name", list(FORMATS))
@pytest.mark.parametrize("fs,bw", [(2_048_000, 32_000), (2_048_000, 16_000)])
def test_generic_first_stage_integer_path(fs, bw, name, monkeypatch, diag_lib):
    """SC_GENERIC=1 (diagnostics build): the one-output-per-lane first stage reads the integer stream like the branch kernel."""
    monkeypatch.setenv("SC_GENERIC", "1")
    n = 90_000
    q = _ints(n, fs, name, seed=5)
    x = _to_cf32(q, name)
    ci, cf = _pair(fs, bw, name, channels=3, max_samples=1 << 16)
    for ch in (ci, cf):
        ch.start(0, int(fs / 7))
        ch.start(2, int(-fs / 5))
    pos = 0
    for size in (1, 4_000, 1 << 16, 19_463):
        _same(ci.process(q[pos:pos + size]), cf.process(x[pos:pos + size]), (name, size))
        pos += size
    ci.close()
    cf.close()


def test_start_stop_restart_and_format_switch():
    """Slots stop, restart on other shifts, and the stream switches CU8 -> CF32 -> CU8 between calls: histories and phases
    carry across, so the whole session equals an all-CF32 session fed the converted stream."""
    fs, bw, name = 2_048_000, 32_000, "cu8"
    n = 193_000
    q = _ints(n, fs, name, seed=11)
    x = _to_cf32(q, name)
    mixed = Channelizer(fs, bw, in_format=A.SS_FMT_CU8, channels=3, max_samples=1 << 16)
    ref = Channelizer(fs, bw, channels=3, max_samples=1 << 16)
    script = [  # (call size, events before it, input format of the mixed context)
        (30_000, [("start", 0, 250_000), ("start", 1, -400_000)], "cu8"),
        (12_345, [("stop", 0)], "cu8"),
        (40_000, [("start", 0, -613_500), ("start", 2, 12_500)], "cf32"),
        (7, [("stop", 1)], "cf32"),
        (50_000, [("start", 1, 300_000)], "cu8"),
        (60_648, [("stop", 2)], "cu8"),
    ]
    pos = 0
    for size, events, fmt in script:
        for ev in events:
            for ch in (mixed, ref):
                ch.start(ev[1], ev[2]) if ev[0] == "start" else ch.stop(ev[1])
        mixed.set_input_format(A.SS_FMT_CU8 if fmt == "cu8" else A.SS_FMT_CF32)
        a = mixed.process(q[pos:pos + size] if fmt == "cu8" else x[pos:pos + size])
        _same(a, ref.process(x[pos:pos + size]), (size, fmt))
        pos += size
    assert pos == n
    with pytest.raises(TypeError):
        mixed.process(x[:10])  # CU8 context, complex64 samples
    with pytest.raises(TypeError):
        mixed.process(q[:10].astype(np.int8))
    mixed.set_input_format(A.SS_FMT_CF32)
    with pytest.raises(TypeError):
        mixed.process(q[:10])
    with pytest.raises(pkg.abi.SpecscanError):
        mixed.set_input_format(4)
    with pytest.raises(pkg.abi.SpecscanError):
        mixed.set_input_format(A.SS_FMT_CS16, -1.0)
    with pytest.raises(pkg.abi.SpecscanError):
        mixed.set_input_format(A.SS_FMT_CS16, float("nan"))
    mixed.close()
    ref.close()


@pytest.mark.parametrize("name", ["cs8", "cu8", "cs16"])
def test_device_entry_point_equals_host_entry_point(name):
    import torch
    fs, bw, n = 2_048_000, 32_000, 1 << 17
    fmt, s, *_ = FORMATS[name]
    q = _ints(n, fs, name, seed=21)
    dev = torch.device("cuda:0")
    d = Channelizer(fs, bw, in_format=fmt, int_scale=s, channels=3, max_samples=n)
    h = Channelizer(fs, bw, in_format=fmt, int_scale=s, channels=3, max_samples=n)
    for ch in (d, h):
        ch.start(0, 250_000)
        ch.start(2, -100_000)
    cap = d.output_capacity(n)
    d_iq = torch.from_numpy(q).to(dev)
    d_i8 = torch.zeros((3, cap, 2), dtype=torch.int8, device=dev)
    d_cf = torch.zeros((3, cap, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    counts = d.process_device(d_iq, n, d_i8, d_cf, cap)
    d.sync()
    want = h.process(q)
    assert list(counts) == [n // 64, 0, n // 64]
    for k in (0, 2):
        assert d_i8[k, :counts[k]].cpu().numpy().tobytes() == want[k][0].tobytes()
        assert d_cf[k, :counts[k]].cpu().numpy().tobytes() == want[k][1].tobytes()
    with pytest.raises(TypeError):
        d.process_device(d_iq.to(torch.float32), n, d_i8, None, cap)
    if name == "cs16":
        flat = d_iq.reshape(-1)
        with pytest.raises(pkg.abi.SpecscanError) as e:
            d.process_device(flat[1:], n - 1, d_i8, None, cap)  # 2 bytes off the 4-byte sample
        assert e.value.status == A.SS_ERR_INVALID
    d.close()
    h.close()


def test_one_upload_feeds_the_scan_chain_and_the_channeliser():
    """One CU8 device tensor of nframes items of N*D samples: ss_process_device of a CU8 scan context and sc_process_device of
    a CU8 channeliser read it at once, and each equals its host entry point on the same bytes."""
    import torch
    fs, center, nframes = 2_048_000, 145_000_000, 40
    scan_d = pkg.SpectrumEngine(fs, center, in_format=A.SS_FMT_CU8, learn_frames=2, max_batch=nframes)
    scan_h = pkg.SpectrumEngine(fs, center, in_format=A.SS_FMT_CU8, learn_frames=2, max_batch=nframes)
    n, decim = scan_d.cfg.fft_size, scan_d.cfg.decim
    assert (n, decim) == (8192, 5)
    band = pkg.synth.SyntheticBand(n, decim=decim, seed=3, on_frame=6, off_frame=nframes - 4)
    u8 = band.frames_cu8(nframes)  # [nframes, N*D, 2]
    dev = torch.device("cuda:0")
    d_iq = torch.from_numpy(u8).to(dev)
    planes = [torch.empty((nframes, n), dtype=torch.float32, device=dev) for _ in range(3)]
    off = torch.zeros(nframes + 1, dtype=torch.int32, device=dev)
    idx = torch.empty(nframes * n, dtype=torch.int32, device=dev)
    cav = torch.empty(nframes * n, dtype=torch.float32, device=dev)
    nsamples = nframes * n * decim
    ch_d = Channelizer(fs, 32_000, in_format=A.SS_FMT_CU8, channels=2, max_samples=nsamples)
    ch_h = Channelizer(fs, 32_000, in_format=A.SS_FMT_CU8, channels=2, max_samples=nsamples)
    for ch in (ch_d, ch_h):
        ch.start(0, 100_000)
        ch.start(1, -300_000)
    cap = ch_d.output_capacity(nsamples)
    d_i8 = torch.zeros((2, cap, 2), dtype=torch.int8, device=dev)
    d_cf = torch.zeros((2, cap, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    scan_d.process_device(d_iq, nframes, *planes, off, idx, cav)
    counts = ch_d.process_device(d_iq, nsamples, d_i8, d_cf, cap)
    scan_d.sync()
    ch_d.sync()
    want = scan_h.process(u8)
    got_off = off.cpu().numpy()
    np.testing.assert_array_equal(got_off, want["cand_off"])
    np.testing.assert_array_equal(idx[:got_off[-1]].cpu().numpy(), want["cand_idx"][:want["cand_off"][-1]])
    assert got_off[-1] > 0
    want_ch = ch_h.process(u8)
    for k in (0, 1):
        assert d_i8[k, :counts[k]].cpu().numpy().tobytes() == want_ch[k][0].tobytes()
        assert d_cf[k, :counts[k]].cpu().numpy().tobytes() == want_ch[k][1].tobytes()
    assert torch.equal(d_iq.cpu(), torch.from_numpy(u8))  # both only read it
    ch_d.close()
    ch_h.close()


MAIN = r"""
#include <recorder_bank.h>
#include <specscan.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

static unsigned crc32_of(const int8_t* p, size_t n) {  // zlib's CRC-32, bitwise
  unsigned c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= (unsigned char)p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return ~c;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int fs = 1024000, bw = 16000, chunk = 40960, center = 145000000;
  const int fmt = atoi(argv[3]);
  const size_t bytes = (size_t)SS_FMT_BYTES(fmt);
  FILE* fp = fopen(argv[1], "rb");
  const int nchunks = atoi(argv[2]);
  std::vector<unsigned char> iq(bytes * chunk * nchunks);
  if (!fp || fread(iq.data(), 1, iq.size(), fp) != iq.size()) return 3;
  fclose(fp);
  printf("[");
  bool first = true;
  specscan::RecorderBank bank(fs, bw, 2, chunk, [&](int64_t t, int32_t f, int32_t rate, const int8_t* d, int n) {
    printf("%s[%lld,%d,%d,%d,%u]", first ? "" : ",", (long long)t, f, rate, n, crc32_of(d, (size_t)n * 2));
    first = false;
  }, 0, fmt);
  for (int c = 0; c < nchunks; ++c) {
    const int64_t now = 1000 + 40 * c;
    std::vector<specscan::RecorderBank::ShiftFlush> want;
    if (c >= 2 && c < 40) want.push_back({100000, c % 5 == 0});
    if (c >= 10 && c < 30) want.push_back({-250000, c % 7 == 0});
    if (c >= 45) want.push_back({-250000, c % 3 == 0});  // a new recording on a slot that was used before
    bank.updateRecordings(want, center, now);
    bank.work(iq.data() + bytes * chunk * c, chunk, now);
  }
  printf("]\n");
  return 0;
}
"""


def test_recorder_bank_cu8_publishes_what_cf32_publishes(tmp_path):
    fs, chunk, nchunks = 1_024_000, 40_960, 60
    q = _ints(chunk * nchunks, fs, "cu8", seed=8)
    x = _to_cf32(q, "cu8")
    src = tmp_path / "bank_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "bank_main"
    csrc = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "host"),
           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + csrc, "-lspecscan", "-Wl,-rpath," + csrc,
           "-Wl,-rpath-link," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    records = {}
    for fmt, data in ((A.SS_FMT_CU8, q), (A.SS_FMT_CF32, x)):
        raw = tmp_path / f"stream{fmt}"
        data.tofile(raw)
        r = subprocess.run([str(exe), str(raw), str(nchunks), str(fmt)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        records[fmt] = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(records[A.SS_FMT_CF32]) > 5
    assert records[A.SS_FMT_CU8] == records[A.SS_FMT_CF32]


def _decreep(got, ref):
    """Residual max |error| / max |ref| after removing the best-fit linear phase ramp (the reference rotator's fp32 creep)."""
    w = np.abs(ref) ** 2
    d = np.angle(got * np.conj(ref))
    k = np.arange(len(ref), dtype=np.float64)
    slope = float((w * k) @ d / ((w * k) @ k))
    return float(np.abs(got * np.exp(-1j * slope * k) - ref).max() / np.abs(ref).max()), slope


@pytest.mark.parametrize("name", ["cs8", "cu8", "cs16"])
def test_integer_input_against_the_oracle(name):
    fs, bw, n = 2_048_000, 32_000, 150_000
    fmt, s, *_ = FORMATS[name]
    q = _ints(n, fs, name, seed=31)
    x = _to_cf32(q, name)
    ch = Channelizer(fs, bw, in_format=fmt, int_scale=s, channels=2, max_samples=1 << 16)
    ch.start(1, int(fs / 7))
    o = oracle.ChannelizerOracle(fs, bw)
    o.set_shift(int(fs / 7))
    got, ref, pos = [], [], 0
    for size in (1 << 16, 30_001, 1 << 16, n - (1 << 17) - 30_001):
        got.append(ch.process(q[pos:pos + size])[1][1])
        ref.append(o.process(x[pos:pos + size])[0])
        pos += size
    g, r = np.concatenate(got), np.concatenate(ref)
    assert len(g) == len(r) and np.abs(r).max() > 0.05
    resid, slope = _decreep(g, r)
    assert resid < 1.5e-4 and abs(slope) < 1e-7 * fs / bw, (name, resid, slope)
    ch.close()
