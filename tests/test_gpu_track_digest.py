"""The tracking digest on the GPU (include/specscan_track.h, csrc/track_digest.h): st_digest against the numpy restatement
(tests/digest_ref.py) fed with the ENGINE'S OWN rel / avg planes, copied back by the same ss_process call — cand_best, watch and
peak_idx equal, cand_avg / peak_avg bit-equal to the plane's floats — and, end to end, the transmissions through st_digest +
process_batch_digest equal to those through the planes + process_batch on the same engine, frame by frame. Integers and copies of
plane values: equality, no tolerance. Needs an MI355X: run with -m gpu."""
import json
import os
import subprocess

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from digest_ref import DigestRef, assert_digest_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = pkg.abi.SS_FLAG_KEEP_PLANES
CENTER = 145_000_000


def _batches(nframes, sizes):
    edges, k = [0], 0
    while edges[-1] < nframes:
        edges.append(min(nframes, edges[-1] + sizes[k % len(sizes)]))
        k += 1
    return list(zip(edges[:-1], edges[1:]))


def _grid_lists(nframes, n, every, rng):
    """Candidate lists nobody detected: bins 0 and N - 1 of every frame and a jittered grid in between (ascending inside a frame),
    so that every kind of rel row — learning frames (-100: all ties), warm-up, noise, signal, -inf, NaN — meets getBestIndex."""
    off, idx = [0], []
    for _ in range(nframes):
        bins = np.unique(np.concatenate([[0, n - 1], np.arange(int(rng.integers(1, every)), n - 1, every)])).astype(np.int32)
        idx.append(bins)
        off.append(off[-1] + bins.size)
    return np.asarray(off, np.int32), np.concatenate(idx)


class _Route:
    """One st_ctx with the restatement next to it, and one tracker on each."""

    def __init__(self, eng, n, fs, g, start_level, gy, **tk):
        self.dig = eng.track_digest(g, start_level=start_level, max_watch=4096)
        self.ref = DigestRef(n, g, start_level, gy)
        self.tr_digest = pkg.tracker.SignalTracker(n, fs, group_size=g, grouping_y=gy, start_level=start_level, **tk)
        self.tr_planes = pkg.tracker.SignalTracker(n, fs, group_size=g, grouping_y=gy, start_level=start_level, **tk)
        self.tx = []
        self.moved = 0

    def reset(self):
        self.dig.reset()
        self.ref.reset()
        self.tr_digest.reset()
        self.tr_planes.reset()

    def batch(self, r, t, off, idx, extra_keys, what, track=True):
        keys = np.concatenate([self.tr_digest.keys, np.asarray(extra_keys, np.int32)])
        got = self.dig.digest(off, idx, keys)
        want = self.ref.digest(r["rel"], r["avg"], off, idx, keys)
        assert_digest_equal(got, want, what)
        nf, nc, nw = got["nframes"], got["cand_idx"].size, got["watch"].size
        assert got["d2h_bytes"] <= 8 * nc + 4 * nw + 8 * nf * nw, (what, got["d2h_bytes"])
        self.moved += int((got["cand_best"] != got["cand_idx"]).sum())
        if track:
            a = self.tr_digest.process_batch_digest(t, got)
            b = self.tr_planes.process_batch(t, r["avg"], r["rel"], off, idx)
            for f in range(nf):
                np.testing.assert_array_equal(a[f][0], b[f][0], err_msg=f"{what} frame {f}: transmissions")
                np.testing.assert_array_equal(a[f][1], b[f][1], err_msg=f"{what} frame {f}: signal keys")
            self.tx.extend(x[0] for x in a)
        return got


def _run(n, frames, fmt=pkg.abi.SS_FMT_CF32, g=128, sizes=(7, 64, 1, 100), max_batch=128, flags=KEEP, nframes=None, retune_after=None, grid_every=37,
         gy=21, zero_frame=None, on=30, off=10_000, seed=5, **cfg):
    """A stream through one engine in uneven batches; after every batch the detected lists (start_level 8, with both trackers) and
    grid lists (start_level -30: noise rows qualify, so the mode is taken of eleven values) go through st_digest and the restatement."""
    fs = n * 250
    band = pkg.synth.SyntheticBand(n, seed=seed, on_frame=on, off_frame=off)
    iq = getattr(band, frames)(nframes)
    if zero_frame is not None:
        iq[zero_frame] = 128 if frames == "frames_cu8" else 0
    t = (1_000 + 40 * np.arange(nframes)).astype(np.int64)
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=max_batch, flags=flags, in_format=fmt, learn_ms=280, grouping_y=gy, **cfg)
    real = _Route(eng, n, fs, g, 8.0, gy, min_time_ms=200, timeout_ms=400)
    grid = _Route(eng, n, fs, g, -30.0, gy)
    rng = np.random.default_rng(3)
    total = same_avg = 0
    for k, (a, b) in enumerate(_batches(nframes, sizes)):
        r = eng.process(iq[a:b], t_ms=t[a:b])
        d = real.batch(r, t[a:b], r["cand_off"], r["cand_idx"], [0, n - 1], f"batch {k} [{a}, {b})")
        total += d["cand_idx"].size
        same_avg += int((d["cand_avg"].view(np.uint32) == r["cand_avg"].view(np.uint32)).sum())
        goff, gidx = _grid_lists(b - a, n, grid_every, rng)
        grid.batch(r, t[a:b], goff, gidx, [0, n - 1, n // 2], f"grid lists, batch {k} [{a}, {b})", track=False)
        if retune_after is not None and k == retune_after:  # SdrDevice::setFrequencyRange: another range, every buffer reset
            eng.set_frequency_range(CENTER + fs - fs // 2, CENTER + fs + fs // 2)
            eng.reset()
            real.reset()
            grid.reset()
    print(f"n {n} {frames}: {total} candidates, gathered cand_avg bit-equal to the ss_process list for {same_avg}; cand_best != cand_idx for {real.moved} "
          f"(grid lists: {grid.moved}); {sum(len(x) for x in real.tx)} transmissions")
    return real, grid, total


def test_digest_small_fused_and_unfused():
    real, grid, total = _run(256, "frames_cf32", g=128, nframes=150, sizes=(7, 64, 1, 30), max_batch=64)
    assert total > 100 and grid.moved > 100
    # another grouping: the unfused back end (rel rows stored), ceil(9 / 2) = 5 rows
    real, grid, total = _run(256, "frames_cf32", g=40, nframes=150, sizes=(3, 64, 1, 30), max_batch=64, gy=9)
    assert total > 100 and grid.moved > 100


@pytest.mark.parametrize("frames,fmt", [("frames_cf32", pkg.abi.SS_FMT_CF32), ("frames_cs16", pkg.abi.SS_FMT_CS16)])
def test_digest_8192_uneven_batches_and_a_retune(frames, fmt):
    real, grid, total = _run(8192, frames, fmt=fmt, g=128, nframes=300, retune_after=3)  # batches 7, 64, 1, 100 | reset | 7, 64, 57
    assert total > 1000 and real.moved > 0 and grid.moved > 1000


def test_digest_65536_cs8():
    real, grid, total = _run(65536, "frames_cs8", fmt=pkg.abi.SS_FMT_CS8, g=128, nframes=64, sizes=(5, 32, 1), max_batch=32, grid_every=301)
    assert total > 1000 and grid.moved > 100


def test_digest_2_20_wide_windows():
    real, grid, total = _run(1 << 20, "frames_cf32", g=547, nframes=44, sizes=(16, 3, 16, 9), max_batch=16, grid_every=4099, on=25)
    assert total > 1000 and grid.moved > 100


@pytest.mark.parametrize("flags", [KEEP, KEEP | pkg.abi.SS_FLAG_REFERENCE_NAN])
def test_digest_zero_frame_and_the_nan_rows_behind_it(flags):
    """A frame of zeros is a -inf row; with SS_FLAG_REFERENCE_NAN the avg rows behind it are NaN from ten below the first poisoned bin
    upwards (tests/test_gpu_degenerate_input.py). The grid lists and the keys at 0, N / 2 and N - 1 take every such row through both kernels."""
    real, grid, total = _run(2048, "frames_cf32", flags=flags, g=128, nframes=200, sizes=(50,), max_batch=64, zero_frame=90, on=40)
    assert total > 1000


def test_end_to_end_transmissions_equal_the_plane_route():
    real, _grid, total = _run(1024, "frames_cf32", g=128, nframes=170, sizes=(1, 16, 7, 3, 16, 16, 5), max_batch=16, on=28, off=110, seed=21)
    seen = sum(len(x) for x in real.tx)
    assert seen > 100 and len(real.tx) == 170 and len(real.tx[-1]) == 0, seen  # appeared, and timed out again
    assert any(x[:, 1].any() for x in real.tx if len(x))  # (some were flushed)


def test_error_paths():
    n, fs = 1024, 256_000
    iq = pkg.synth.SyntheticBand(n, seed=2, on_frame=25, off_frame=10_000).frames_cf32(80)
    t = (1_000 + 40 * np.arange(80)).astype(np.int64)
    plain = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=32, learn_ms=280)
    with pytest.raises(pkg.abi.SpecscanError) as e:
        plain.track_digest(128)
    assert e.value.status == pkg.abi.SS_ERR_INVALID and "KEEP_PLANES" in str(e.value)
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=32, flags=KEEP, learn_ms=280)
    with pytest.raises(pkg.abi.SpecscanError):
        eng.track_digest(1 << 14)  # (eleven rows of such windows do not fit a workgroup's LDS)
    dig = eng.track_digest(128, max_watch=8, cand_cap=1 << 16)
    none = np.zeros(0, np.int32)

    def refused(off, idx, keys, word):
        with pytest.raises(pkg.abi.SpecscanError) as e:
            dig.digest(off, idx, keys)
        assert e.value.status == pkg.abi.SS_ERR_INVALID and word in str(e.value), str(e.value)
    refused(np.zeros(2, np.int32), none, none, "no batch")
    r = eng.process(iq[:32], t_ms=t[:32], want=())
    refused(r["cand_off"], r["cand_idx"], np.arange(9, dtype=np.int32), "max_watch")  # too many keys
    refused(r["cand_off"], r["cand_idx"], np.array([n], np.int32), "outside")
    d = dig.digest(r["cand_off"], r["cand_idx"], none)  # ... and nothing was half-done: the batch is still there to digest
    assert d["nframes"] == 32
    refused(r["cand_off"], r["cand_idx"], none, "already")
    eng.process(iq[32:48], t_ms=t[32:48], want=())  # a batch goes by without st_digest
    r = eng.process(iq[48:80], t_ms=t[48:80], want=())
    assert r["cand_idx"].size > 100
    refused(r["cand_off"], r["cand_idx"], none, "without st_digest")
    dig.reset()
    refused(r["cand_off"], r["cand_idx"], none, "already")  # (st_reset starts from the next batch)
    tight = eng.track_digest(128, max_watch=4096, cand_cap=16)
    r = eng.process(iq[48:80], t_ms=t[48:80], want=())
    with pytest.raises(pkg.abi.SpecscanError) as e:
        tight.digest(r["cand_off"], r["cand_idx"], none)
    assert "cand_cap" in str(e.value)
    d = dig.digest(r["cand_off"], r["cand_idx"], none)
    assert d["cand_idx"].size == r["cand_idx"].size
    eng.process(iq[48:80], t_ms=t[48:80], want=())
    eng.set_frequency_range(CENTER, CENTER + fs)
    refused(r["cand_off"], r["cand_idx"], none, "ss_set_frequency_range")


def test_d2h_bytes_of_the_benchmark_batch():
    """1024 frames of 8192 points: the rel and avg planes are 64 MiB; the digest's traffic is counted, not measured."""
    n, nframes = 8192, 1024
    band = pkg.synth.SyntheticBand(n, seed=0, on_frame=130, off_frame=330, period=400)
    eng = pkg.SpectrumEngine(2_048_000, CENTER, fft_size=n, decim=1, max_batch=nframes, flags=KEEP, learn_ms=280)
    dig = eng.track_digest(128, max_watch=4096)
    tr = pkg.tracker.SignalTracker(n, 2_048_000, group_size=128, min_time_ms=200, timeout_ms=400)
    t0 = 1_000
    for k in range(2):
        iq = band.frames_cf32(nframes)
        t = (t0 + 40 * np.arange(nframes)).astype(np.int64)
        t0 += 40 * nframes
        r = eng.process(iq, t_ms=t, want=(), cand_cap=nframes * 1024)
        d = dig.digest(r["cand_off"], r["cand_idx"], tr.keys)
        nc, nw = d["cand_idx"].size, d["watch"].size
        assert d["d2h_bytes"] <= 8 * nc + 4 * nw + 8 * nframes * nw and d["d2h_bytes"] < 64 << 20, d["d2h_bytes"]
        out = tr.process_batch_digest(t, d)
        print(f"batch {k}: {nc} candidates, {nw} watch keys, {d['d2h_bytes']} bytes device to host (two planes: {8 * n * nframes}), "
              f"{sum(len(x[0]) for x in out)} transmissions")
    assert nc > 10_000


ADAPTER_MAIN = r"""
// Two adapter blocks on the same stream, driven like the scheduler drives a sync_block: one with enableTracker (planes), one with
// enableDeviceTracker (digest; its config carries SS_FLAG_KEEP_PLANES). A retune in the middle, as SdrDevice::setFrequencyRange does it.
#include <gpu_spectrum_block.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

using Tx = std::vector<std::vector<specscan::FrequencyFlush>>;

static void print(const char* name, const Tx& tx) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < tx.size(); ++i) {
    printf("%s[", i ? "," : "");
    for (size_t k = 0; k < tx[i].size(); ++k) printf("%s[%d,%d]", k ? "," : "", tx[i][k].shift_hz, (int)tx[i][k].flush);
    printf("]");
  }
  printf("]");
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int n = atoi(argv[2]), nframes = atoi(argv[3]);
  ss_config cfg;
  ss_default_config(&cfg, n * 250, 145000000);
  cfg.fft_size = n;
  cfg.decim = 1;
  cfg.learn_frames = 20;
  cfg.learn_ms = 0;
  cfg.max_batch = 16;
  std::vector<gr_complex> iq((size_t)n * nframes);
  FILE* fp = fopen(argv[1], "rb");
  if (!fp || fread(iq.data(), sizeof(gr_complex), iq.size(), fp) != iq.size()) return 3;
  fclose(fp);
  specscan::TrackerConfig tc;
  tc.fft_size = n;
  tc.sample_rate = n * 250;
  tc.group_size = 128;
  tc.min_time_ms = 200;
  tc.timeout_ms = 400;
  GpuSpectrum planes(cfg, nullptr);
  ss_config keep = cfg;
  keep.flags |= SS_FLAG_KEEP_PLANES;
  GpuSpectrum digest(keep, nullptr);
  bool refused = false;
  try {
    planes.enableDeviceTracker(tc, nullptr);  // no SS_FLAG_KEEP_PLANES: must throw
  } catch (const std::runtime_error&) {
    refused = true;
  }
  Tx tx_planes, tx_digest;
  planes.enableTracker(tc, [&](const std::vector<specscan::FrequencyFlush>& tx) { tx_planes.push_back(tx); });
  digest.enableDeviceTracker(tc, [&](const std::vector<specscan::FrequencyFlush>& tx) { tx_digest.push_back(tx); });
  int clock_pos = 0;
  for (GpuSpectrum* b : {&planes, &digest}) b->setClock([&] { return (int64_t)(1000 + 40 * clock_pos); });
  std::vector<float> psd((size_t)n * 16);
  const int sizes[] = {1, 16, 7, 3, 16, 16, 5};
  int pos = 0, k = 0;
  bool retuned = false;
  while (pos < nframes) {
    int want = sizes[k++ % 7];
    if (want > nframes - pos) want = nframes - pos;
    clock_pos = pos;
    for (GpuSpectrum* b : {&planes, &digest}) {
      gr_vector_const_void_star in{iq.data() + (size_t)pos * n};
      gr_vector_void_star out{psd.data()};
      if (b->work(want, in, out) != want || !b->lastError().empty()) {
        fprintf(stderr, "work: %s\n", b->lastError().c_str());
        return 4;
      }
    }
    pos += want;
    if (!retuned && pos >= nframes / 2) {
      retuned = true;
      for (GpuSpectrum* b : {&planes, &digest}) {
        b->setFrequencyRange(145000000 + n * 125, 145000000 + n * 375);
        b->resetBuffers();
      }
    }
  }
  printf("{\"refused\": %d, ", (int)refused);
  print("planes", tx_planes);
  printf(", ");
  print("digest", tx_digest);
  printf("}\n");
  return 0;
}
"""


def test_adapter_device_tracker_delivers_what_the_plane_tracker_delivers(tmp_path):
    n, nframes = 1024, 240
    band = pkg.synth.SyntheticBand(n, seed=21, on_frame=28, off_frame=90, period=120)
    iq = band.frames_cf32(nframes)
    raw = tmp_path / "iq.cf32"
    iq.tofile(raw)
    src = tmp_path / "adapter_main.cpp"
    src.write_text(ADAPTER_MAIN)
    exe = tmp_path / "adapter_main"
    csrc = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "host"),
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "oracle", "stubs"), str(src),
           os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "host", "signal_tracker.cpp"), "-o", str(exe), "-L" + csrc, "-lspecscan",
           "-Wl,-rpath," + csrc, "-Wl,-rpath-link," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(raw), str(n), str(nframes)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["refused"] == 1
    assert len(rep["planes"]) == nframes and rep["digest"] == rep["planes"]
    first, second = rep["planes"][:nframes // 2], rep["planes"][nframes // 2:]
    assert sum(len(t) for t in first) > 50 and sum(len(t) for t in second) > 50  # before and after the retune
    assert any(f for t in rep["planes"] for _, f in t)
