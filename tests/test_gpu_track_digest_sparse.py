"""The tracking digest on an engine that keeps no planes (include/specscan_track_digest_sparse.h, csrc/track_digest_sparse.h), on the GPU.

Oracle P — the forms that leave a bin-ordered dB plane: a second engine WITH SS_FLAG_KEEP_PLANES and st_digest on the same frames with
the same cuts (existing code); the digests equal, the trackers' transmissions equal frame by frame.
Oracle F — the forms that leave no plane: a second engine of the identical configuration with start_level = -3e38 and room for every
passed bin of every frame. Its cand_avg lists ARE the avg plane of that form (cells that never appear: NaN); the rel rows come from
ss_read_window(SS_PLANE_REL) of the tested engine; tests/digest_ref.py on those two gives the expected digest for the tested engine's
lists and keys. The tested engine's lists must be lists_at_level of that plane and its digest's cand_avg its own call's.
Integers equal, floats bit-equal: no tolerance anywhere. Needs an MI355X: run with -m gpu."""
import json
import os
import subprocess

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from digest_ref import DigestRef, assert_digest_equal
from parity import lists_at_level, pass_mask
from test_gpu_track_feed import TK, _batches
from test_gpu_track_sparse import CULL_LEVEL, TILE_B, TILE_F, marked_columns

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP, REF_NAN = pkg.abi.SS_FLAG_KEEP_PLANES, pkg.abi.SS_FLAG_REFERENCE_NAN
CF32, CS8, CS16 = pkg.abi.SS_FMT_CF32, pkg.abi.SS_FMT_CS8, pkg.abi.SS_FMT_CS16
CENTER = 145_000_000
INVALID = pkg.abi.SS_ERR_INVALID
G = 128
FRAMES = {CF32: "frames_cf32", CS8: "frames_cs8", CS16: "frames_cs16"}


def _stream(n, fmt, nframes, **band):
    iq = getattr(pkg.synth.SyntheticBand(n, seed=5, on_frame=30, off_frame=10_000, **band), FRAMES[fmt])(nframes)
    return iq, (1_000 + 40 * np.arange(nframes)).astype(np.int64)


def _engine(n, fmt, max_batch, **cfg):
    # (seven learning frames either way: 280 ms of frames 40 ms apart for calls with clocks, learn_frames for device calls, which have none)
    return pkg.SpectrumEngine(n * 250, CENTER, fft_size=n, decim=1, max_batch=max_batch, learn_ms=280, learn_frames=7, in_format=fmt, **cfg)


class Runner:
    """One engine driven batch by batch, through eng.process (clocks) or process_device + sync (device tensors), lists only."""

    def __init__(self, eng, device, cap_per_frame, clocks=True):
        self.eng, self.device, self.cap, self.clocks = eng, device, cap_per_frame, clocks

    def batch(self, iq, t):
        nf = len(iq)
        if not self.device:
            r = self.eng.process(iq, t_ms=t if self.clocks else None, want=(), cand_cap=nf * self.cap)
            assert r["status"] == 0
            return r["cand_off"], r["cand_idx"], r["cand_avg"]
        import torch
        dev = torch.device("cuda", 0)
        d_iq = torch.from_numpy(iq.view(np.float32) if iq.dtype == np.complex64 else iq).to(dev)
        off = torch.zeros(nf + 1, dtype=torch.int32, device=dev)
        idx = torch.empty(nf * self.cap, dtype=torch.int32, device=dev)
        cav = torch.empty(nf * self.cap, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()  # (torch's fills run on torch's stream, the library writes from its own)
        self.eng.process_device(d_iq, nf, cand_off=off, cand_idx=idx, cand_avg=cav)
        self.eng.sync()
        off = off.cpu().numpy()
        return off, idx[:int(off[nf])].cpu().numpy(), cav[:int(off[nf])].cpu().numpy()


class Books:
    """The replay's two counters as the watch lists and the cuts define them (tests/test_gpu_track_sparse.py's book-keeping)."""

    def __init__(self, n):
        self.n, self.frames, self.want_eval, self.want_total = n, 0, 0, 0

    def count(self, nframes, watch):
        ft = (nframes + self.frames % TILE_F + TILE_F - 1) // TILE_F
        self.frames += nframes
        self.want_total += ft * (self.n // TILE_B)
        self.want_eval += ft * marked_columns(watch, G // 2, self.n)

    def check(self, dig):
        s = dig.sparse_stats()
        print(f"sparse_stats {s}, expected {self.want_eval} of {self.want_total}")
        assert s == {"tiles_evaluated": self.want_eval, "tiles_in_batches": self.want_total}, (s, self.want_eval, self.want_total)
        assert s["tiles_evaluated"] < s["tiles_in_batches"], s

    def reset(self):
        self.frames = self.want_eval = self.want_total = 0


def _tracker(n, level):
    return pkg.tracker.SignalTracker(n, n * 250, group_size=G, start_level=level, **TK)


def _tile_counters(eng):
    eng.sync()
    s = eng.stats()
    return {k: s[k] for k in ("tiles_total", "tiles_tested", "tiles_culled")}


def _oracle_p(n, fmt, sizes, nframes, max_batch, device=False, level=8.0, reset_after=None, untracked=False):
    iq, t = _stream(n, fmt, nframes)
    a_eng = _engine(n, fmt, max_batch, flags=KEEP, start_level=level)
    b_eng = _engine(n, fmt, max_batch, start_level=level)
    c_eng = _engine(n, fmt, max_batch, start_level=level) if untracked else None
    a_dig = a_eng.track_digest(G, start_level=level, max_watch=4096)
    b_dig = b_eng.track_digest(G, start_level=level, max_watch=4096, sparse=True)
    a_run, b_run = Runner(a_eng, False, 4096, clocks=not device), Runner(b_eng, device, 4096)  # (device calls carry no clocks: the planes engine learns by count too)
    c_run = Runner(c_eng, device, 4096) if untracked else None
    a_trk, b_trk, books = _tracker(n, level), _tracker(n, level), Books(n)
    ntx = ncand = 0
    for k, (lo, hi) in enumerate(_batches(nframes, sizes)):
        what = f"batch {k} [{lo}, {hi})"
        a_off, a_idx, _ = a_run.batch(iq[lo:hi], t[lo:hi])
        a_d = a_dig.digest(a_off, a_idx, a_trk.keys)
        keys = b_trk.keys.copy()  # the tracker's own, taken before the batch
        b_off, b_idx, b_cav = b_run.batch(iq[lo:hi], t[lo:hi])
        b_d = b_dig.digest(b_off, b_idx, keys)
        if c_run:
            c_run.batch(iq[lo:hi], t[lo:hi])
        np.testing.assert_array_equal(keys, a_trk.keys, err_msg=what)
        assert_digest_equal(b_d, a_d, what)
        np.testing.assert_array_equal(b_d["cand_avg"].view(np.uint32), b_cav.view(np.uint32), err_msg=f"{what}: cand_avg against the call's own")
        assert not np.isnan(b_d["peak_avg"]).any(), what
        books.count(hi - lo, b_d["watch"])
        tx_a, tx_b = a_trk.process_batch_digest(t[lo:hi], a_d), b_trk.process_batch_digest(t[lo:hi], b_d)
        for f in range(hi - lo):
            np.testing.assert_array_equal(tx_b[f][0], tx_a[f][0], err_msg=f"{what} frame {f}: transmissions")
            np.testing.assert_array_equal(tx_b[f][1], tx_a[f][1], err_msg=f"{what} frame {f}: signal keys")
        ntx += sum(len(x[0]) for x in tx_b)
        ncand += b_idx.size
        if reset_after is not None and k == reset_after:  # retune, ss_reset and st_reset
            books.check(b_dig)
            for eng, dig, trk in ((a_eng, a_dig, a_trk), (b_eng, b_dig, b_trk)):
                eng.set_frequency_range(CENTER + n * 250 - n * 125, CENTER + n * 250 + n * 125)
                eng.reset()
                dig.reset()
                trk.reset()
            books.reset()
            assert b_dig.sparse_stats() == {"tiles_evaluated": 0, "tiles_in_batches": 0}
    books.check(b_dig)
    print(f"oracle P n {n}: {ncand} candidates, {ntx} transmissions")
    assert ntx > 0 and ncand > 100
    return b_eng, c_eng


def test_1024_host_calls_with_a_retune():
    _oracle_p(1024, CF32, (7, 64, 1, 30), 150, 64, reset_after=2)


@pytest.mark.parametrize("fmt", [CF32, CS16])
def test_8192_culled_host_calls(fmt):
    b_eng, c_eng = _oracle_p(8192, fmt, (7, 64, 1, 100), 300, 128, level=CULL_LEVEL, untracked=True)
    tiles_b, tiles_c = _tile_counters(b_eng), _tile_counters(c_eng)
    print(tiles_b, tiles_c)
    assert tiles_b["tiles_culled"] > 0, tiles_b
    assert tiles_b == tiles_c, (tiles_b, tiles_c)  # tracking does not move the scan's counters


def test_8192_device_calls():
    _oracle_p(8192, CF32, (64, 64, 35, 20), 183, 64, device=True)


def _rel_rows(eng, n, nframes):
    return np.stack([eng.read_window(pkg.abi.SS_PLANE_REL, f, 0, n) for f in range(nframes)])


def _oracle_f(n, fmt, sizes, no_plane, restricted=False):
    """sizes: the cuts, once through; no_plane: the cut sizes after which the call must have left no dB plane."""
    nframes, max_batch, fs = sum(sizes), max(sizes), n * 250
    band, cfg = {}, {}
    if restricted:  # 32768 scanned bins around DC, the combs at least 512 bins inside its edges (and so every watch window)
        band["centres"] = tuple(b / n for b in (-9000, -3000, 4000, 11000))
        cfg = dict(range_lo=CENTER - 16384 * 250, range_hi=CENTER + 16384 * 250)
    passes = pass_mask(n, fs, cfg.get("range_lo", CENTER - fs // 2), cfg.get("range_hi", CENTER + fs // 2))
    assert not restricted or 32000 <= passes.sum() <= 32770
    iq, t = _stream(n, fmt, nframes, **band)
    b_eng = _engine(n, fmt, max_batch, **cfg)
    f_eng = _engine(n, fmt, max_batch, start_level=-3e38, **cfg)
    b_dig = b_eng.track_digest(G, max_watch=4096, sparse=True)
    b_run, f_run = Runner(b_eng, True, 8192), Runner(f_eng, True, int(passes.sum()))
    trk, ref, books = _tracker(n, 8.0), DigestRef(n, G, 8.0), Books(n)
    ntx = ncand = 0
    for k, (lo, hi) in enumerate(_batches(nframes, sizes)):
        what, nf = f"batch {k} [{lo}, {hi})", hi - lo
        keys = trk.keys.copy()  # the tracker's own, taken before the batch
        b_off, b_idx, b_cav = b_run.batch(iq[lo:hi], t[lo:hi])
        f_off, f_idx, f_cav = f_run.batch(iq[lo:hi], t[lo:hi])
        for eng in (b_eng, f_eng):
            if nf in no_plane:  # the no-plane form ran: there is no dB plane to read
                with pytest.raises(pkg.abi.SpecscanError) as e:
                    eng.read_window(pkg.abi.SS_PLANE_PSD, 0, 0, 64)
                assert e.value.status == INVALID, what
        rel = _rel_rows(b_eng, n, nf)
        if k > 0 and ref.tail.shape[0]:  # the ring's rows in front of the batch are the rows the digest kept
            back = min(ref.tail.shape[0], lo)
            for j in range(1, back + 1):
                np.testing.assert_array_equal(b_eng.read_window(pkg.abi.SS_PLANE_REL, -j, 0, n).view(np.uint32), ref.tail[-j].view(np.uint32), err_msg=f"{what}: ring row -{j}")
        avg = np.full((nf, n), np.nan, np.float32)  # the avg plane of this form: every passed bin of every frame is a candidate
        avg[np.repeat(np.arange(nf), np.diff(f_off)), f_idx] = f_cav
        want_off, want_idx = lists_at_level(avg, 8.0, passes)
        np.testing.assert_array_equal(b_off, want_off, err_msg=f"{what}: lists")
        np.testing.assert_array_equal(b_idx, want_idx, err_msg=f"{what}: lists")
        b_d = b_dig.digest(b_off, b_idx, keys)
        assert_digest_equal(b_d, ref.digest(rel, avg, b_off, b_idx, keys), what)
        np.testing.assert_array_equal(b_d["cand_avg"].view(np.uint32), b_cav.view(np.uint32), err_msg=f"{what}: cand_avg against the call's own")
        books.count(nf, b_d["watch"])
        ntx += sum(len(x[0]) for x in trk.process_batch_digest(t[lo:hi], b_d))
        ncand += b_idx.size
    books.check(b_dig)
    b_dig.reset()
    assert b_dig.sparse_stats() == {"tiles_evaluated": 0, "tiles_in_batches": 0}
    print(f"oracle F n {n}: {ncand} candidates, {ntx} transmissions")
    assert ntx > 0 and ncand > 100


def test_65536_cs8_the_radix_8_fold():
    _oracle_f(65536, CS8, (7, 16, 40, 9, 16), no_plane=(16, 40))


def test_131072_cs8_the_radix_16_fold():
    _oracle_f(131072, CS8, (7, 16, 25), no_plane=(16, 25))


def test_65536_cf32_the_culled_chain():
    _oracle_f(65536, CF32, (7, 16, 40, 9), no_plane=(16, 40))


def test_262144_cf32_range_restricted():
    _oracle_f(262144, CF32, (7, 16, 25), no_plane=(16, 25), restricted=True)


def test_2_20_cf32_ring_only_range_restricted():
    _oracle_f(1 << 20, CF32, (7, 16, 16, 9), no_plane=(16,), restricted=True)


def test_refusals():
    def refused(call, word, status=INVALID):
        with pytest.raises(pkg.abi.SpecscanError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)
    mk = lambda n=1024, **kw: pkg.SpectrumEngine(n * 250, CENTER, fft_size=n, decim=1, max_batch=32, learn_ms=280, **kw)  # noqa: E731
    refused(lambda: mk(grouping_y=9).track_digest(40, sparse=True), "unfused")
    refused(lambda: mk(flags=REF_NAN).track_digest(G, sparse=True), "REFERENCE_NAN")
    refused(lambda: mk().track_digest(G, max_watch=0, sparse=True), "max_watch")  # (and what st_create refuses)
    refused(lambda: mk().track_digest(G), "KEEP_PLANES")  # st_create itself is unchanged
    keep = mk(flags=KEEP)
    refused(keep.track_digest(G, sparse=True).sparse_stats, "not a sparse object")  # with the flag it is st_create
    refused(keep.track_digest(G).sparse_stats, "not a sparse object")
    n = 1024
    iq, t = _stream(n, CF32, 96)
    eng = mk()
    dig = eng.track_digest(G, sparse=True)
    none = np.zeros(0, np.int32)
    eng.process(iq[:32], t_ms=t[:32], want=())  # a batch goes by without st_digest
    r = eng.process(iq[32:64], t_ms=t[32:64], want=())
    refused(lambda: dig.digest(r["cand_off"], r["cand_idx"], none), "without st_digest")
    dig.reset()
    r = eng.process(iq[64:96], t_ms=t[64:96], want=())
    assert dig.digest(r["cand_off"], r["cand_idx"], none)["nframes"] == 32


ADAPTER_MAIN = r"""
// Two adapter blocks on the same stream, driven like the scheduler drives a sync_block: one with enableTracker (planes), one with
// enableSparseDeviceTracker, neither config carrying SS_FLAG_KEEP_PLANES. A retune in the middle, as SdrDevice::setFrequencyRange does it.
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
  GpuSpectrum planes(cfg, nullptr), sparse(cfg, nullptr);
  bool refused = false;
  try {
    sparse.enableDeviceTracker(tc, nullptr);  // no SS_FLAG_KEEP_PLANES: must still throw
  } catch (const std::runtime_error&) {
    refused = true;
  }
  Tx tx_planes, tx_sparse;
  planes.enableTracker(tc, [&](const std::vector<specscan::FrequencyFlush>& tx) { tx_planes.push_back(tx); });
  sparse.enableSparseDeviceTracker(tc, [&](const std::vector<specscan::FrequencyFlush>& tx) { tx_sparse.push_back(tx); });
  int clock_pos = 0;
  for (GpuSpectrum* b : {&planes, &sparse}) b->setClock([&] { return (int64_t)(1000 + 40 * clock_pos); });
  std::vector<float> psd((size_t)n * 16);
  const int sizes[] = {1, 16, 7, 3, 16, 16, 5};
  int pos = 0, k = 0;
  bool retuned = false;
  while (pos < nframes) {
    int want = sizes[k++ % 7];
    if (want > nframes - pos) want = nframes - pos;
    clock_pos = pos;
    for (GpuSpectrum* b : {&planes, &sparse}) {
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
      for (GpuSpectrum* b : {&planes, &sparse}) {
        b->setFrequencyRange(145000000 + n * 125, 145000000 + n * 375);
        b->resetBuffers();
      }
    }
  }
  printf("{\"refused\": %d, ", (int)refused);
  print("planes", tx_planes);
  printf(", ");
  print("sparse", tx_sparse);
  printf("}\n");
  return 0;
}
"""


def test_adapter_sparse_device_tracker_delivers_what_the_plane_tracker_delivers(tmp_path):
    n, nframes = 1024, 240
    iq = pkg.synth.SyntheticBand(n, seed=21, on_frame=28, off_frame=90, period=120).frames_cf32(nframes)
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
    assert len(rep["planes"]) == nframes and rep["sparse"] == rep["planes"]
    first, second = rep["planes"][:nframes // 2], rep["planes"][nframes // 2:]
    assert sum(len(t) for t in first) > 50 and sum(len(t) for t in second) > 50  # before and after the retune
