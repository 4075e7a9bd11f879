"""The tracked feed on an engine that keeps no planes (include/specscan_track_sparse.h, csrc/track_sparse.h), on the GPU.

Route A — existing code, not under test — is test_gpu_track_feed.RouteA: an engine WITH SS_FLAG_KEEP_PLANES, eng.process with the rel
and avg planes, the trackers on them. Route B is an engine WITHOUT the flag, feed.track(..., sparse=True), on the same frames with the
same batch cuts. For every batch: the lists equal, the watch list K_p U cand_best(p + 1 .. k), the whole digest bit-equal to the numpy
restatement (tests/digest_ref.py) on route A's planes with route B's watch list, the tracker's transmissions equal frame by frame — all
through RouteB.collect as it stands. On top: the scan's own counters (tiles culled, and equal to an untracked engine's) and the
replay's (exactly the watch windows' tile columns, computed here from the collected watch lists and the batch cuts).
Integers equal, floats bit-equal: no tolerance anywhere. Needs an MI355X: run with -m gpu."""
import json
import subprocess
import time

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import replay
from digest_ref import DigestRef, assert_digest_equal
from test_gpu_track_feed import RouteA, RouteB, _batches, _stream

pytestmark = pytest.mark.gpu

KEEP, SPEC, NO_CULL, REF_NAN = pkg.abi.SS_FLAG_KEEP_PLANES, pkg.abi.SS_FLAG_SPECTROGRAM, pkg.abi.SS_FLAG_NO_CULL, pkg.abi.SS_FLAG_REFERENCE_NAN
CENTER = 145_000_000
INVALID = pkg.abi.SS_ERR_INVALID
TK = dict(min_time_ms=200, timeout_ms=400)
TILE_F, TILE_B = 16, 256  # the averaging tile: frames x bins
# Where tiles are culled. The streams here learn their noise ceiling from 7 frames (RouteA / RouteB: learn_ms=280 at 40 ms a frame), which
# leaves it low: on the ORACLE's planes of _stream(8192) (oracle_chain + parity.tile_bounds, reach="runs") the culling bounds of the
# noise-only tiles are 9.33 .. 12.03 dB (median 10.44), those of the comb tiles up to 41.6 dB. At the default 8 dB no tile can be
# dropped; at 15 dB every noise tile that is tested is, and the 25 dB combs still give 47590 of the 56756 candidates of 8 dB.
CULL_LEVEL = 15.0


def marked_columns(watch, half, n):
    """How many 256-bin tile columns the windows [max(0, key - half), min(n - 1, key + half)] touch, bin by bin."""
    cols = set()
    for key in np.asarray(watch, np.int64).tolist():
        cols.update(b // TILE_B for b in range(max(0, key - half), min(n - 1, key + half) + 1))
    return len(cols)


class SparseB(RouteB):
    """RouteB on feed.track(..., sparse=True), with the books the replay's counters are held to."""

    def __init__(self, n, g, start_level=8.0, gy=21, max_batch=64, depth=3, cand_cap=1 << 20, max_watch=4096, engine_level=None, **cfg):
        self.n, self.fs, self.g, self.gy, self.start = n, n * 250, g, gy, start_level
        if engine_level is not None:
            cfg["start_level"] = engine_level
        self.eng = pkg.SpectrumEngine(self.fs, CENTER, fft_size=n, decim=1, max_batch=max_batch, learn_ms=280, grouping_y=gy, **cfg)
        self.feed = self.eng.feed(depth=depth, cand_cap=cand_cap)
        self.trk = self.feed.track(g, start_level=start_level, max_watch=max_watch, sparse=True)
        self.tracker = pkg.tracker.SignalTracker(n, self.fs, group_size=g, grouping_y=gy, start_level=start_level, **TK)
        self.ref = DigestRef(n, g, start_level, gy)
        self.posted = (0, np.zeros(0, np.int32))
        self.at_submit, self.best, self.seq, self.larger = {}, {}, 0, 0
        self.frames = 0          # frames since the last reset
        self.frame_tiles = {}    # seq -> frame tiles of that batch
        self.want_eval = self.want_total = 0

    def submit(self, iq, t):
        super().submit(iq, t)
        self.frame_tiles[self.seq] = (len(iq) + self.frames % TILE_F + TILE_F - 1) // TILE_F
        self.frames += len(iq)

    def count(self, got):
        """The batch's share of the two counters, from its delivered watch list (an overflowed list marks nothing)."""
        ft = self.frame_tiles[got["seq"]]
        self.want_total += ft * (self.n // TILE_B)
        if got["digest_status"] == 0:
            self.want_eval += ft * marked_columns(got["watch"], self.g // 2, self.n)

    def collect(self, a, what, track=True, post=True):
        got = super().collect(a, what, track=track, post=post)
        self.count(got)
        return got

    def check_counters(self, less=False):
        s = self.trk.sparse_stats()
        print(f"sparse_stats {s}, expected {self.want_eval} of {self.want_total}")
        assert s == {"tiles_evaluated": self.want_eval, "tiles_in_batches": self.want_total}, (s, self.want_eval, self.want_total)
        if less:
            assert s["tiles_evaluated"] < s["tiles_in_batches"], s
        return s

    def reset(self, retune=False):
        super().reset(retune)
        self.frames, self.frame_tiles, self.want_eval, self.want_total = 0, {}, 0, 0


class Untracked:
    """An engine like route B's with a plain feed: what the scan's counters are without a tracker."""

    def __init__(self, n, max_batch, **cfg):
        self.fs = n * 250
        self.eng = pkg.SpectrumEngine(self.fs, CENTER, fft_size=n, decim=1, max_batch=max_batch, learn_ms=280, **cfg)
        self.feed = self.eng.feed(depth=3, cand_cap=1 << 20)

    def batch(self, iq, t):
        buf = self.feed.acquire()
        buf[:len(iq)] = iq
        self.feed.submit(len(iq), t_ms=t)
        return self.feed.collect()

    def reset(self, retune=False):
        if retune:
            self.eng.set_frequency_range(CENTER + self.fs - self.fs // 2, CENTER + self.fs + self.fs // 2)
        self.eng.reset()


def _tile_counters(eng):
    eng.sync()
    s = eng.stats()
    return {k: s[k] for k in ("tiles_total", "tiles_tested", "tiles_culled")}


def _in_flight(n, iq, t, sizes, max_batch, g=128, reset_after=None, untracked=False, less=False, level=8.0, flags_a=KEEP, flags_b=0, **cfg):
    """Depth 3, two batches in flight, keys posted after every collect (test_gpu_track_feed._in_flight on the sparse route).
    level: start_level of the engines and of the trackers alike."""
    lv = dict(start_level=level, engine_level=level)
    a, b = RouteA(n, g, max_batch=max_batch, flags=flags_a, **lv, **cfg), SparseB(n, g, max_batch=max_batch, flags=flags_b, **lv, **cfg)
    c = Untracked(n, max_batch, flags=flags_b, start_level=level, **cfg) if untracked else None
    cuts = _batches(len(t), sizes)
    waiting, total, tx, most = [], 0, 0, 0

    def collect_one():
        nonlocal total, tx
        k, ra = waiting.pop(0)
        got = b.collect(ra, f"batch {k} {cuts[k]}")
        total += got["cand_idx"].size
        tx += sum(len(x[0]) for x in ra["tx"])
    for k, (lo, hi) in enumerate(cuts):
        waiting.append((k, a.batch(iq[lo:hi], t[lo:hi])))
        b.submit(iq[lo:hi], t[lo:hi])
        if c:
            c.batch(iq[lo:hi], t[lo:hi])
        if len(waiting) == 2:
            collect_one()
        if reset_after is not None and k == reset_after:  # drain, retune, ss_reset and stf_reset
            while waiting:
                collect_one()
            most = max(most, b.check_counters(less)["tiles_evaluated"])
            a.reset(retune=True)
            b.reset(retune=True)
            if c:
                c.reset(retune=True)
            assert b.trk.sparse_stats() == {"tiles_evaluated": 0, "tiles_in_batches": 0}
    while waiting:
        collect_one()
    stats = b.check_counters(less)
    assert max(most, stats["tiles_evaluated"]) > 0  # (behind a retune with the signals on, the new ceiling holds them: no watch key, nothing replayed)
    tiles_b = _tile_counters(b.eng)
    tiles_c = _tile_counters(c.eng) if c else None
    lags = sorted({s - p for s, (p, _) in b.at_submit.items()})
    b.close()
    print(f"in flight n {n} g {g}: {total} candidates, {tx} transmissions, lags {lags}, scan {tiles_b}, untracked {tiles_c}, replay {stats}")
    return total, tx, lags, tiles_b, tiles_c, stats


@pytest.mark.parametrize("frames,fmt", [("frames_cf32", pkg.abi.SS_FMT_CF32), ("frames_cs16", pkg.abi.SS_FMT_CS16)])
def test_8192_culled_two_in_flight_and_a_retune(frames, fmt):
    """Case 1: the scan culls, its counters are an untracked engine's, the replay ran exactly the watch windows' columns."""
    iq, t = _stream(8192, frames, nframes=300)
    total, tx, lags, tiles_b, tiles_c, stats = _in_flight(8192, iq, t, (7, 64, 1, 100), 128, reset_after=3, untracked=True, less=True, level=CULL_LEVEL,
                                                              in_format=fmt)  # (less: a replay of every tile fails)
    assert total > 1000 and 2 in lags
    assert tiles_b["tiles_culled"] > 0, tiles_b
    assert tiles_b == tiles_c, (tiles_b, tiles_c)  # tracking does not move the scan's counters


def test_quiet_batches_with_posted_keys():
    """Case 2: the signals stop, the scan finds nothing and culls every tile it tests — and the peaks of eight hand-posted keys, the
    band's edges among them, are still the restatement's in every frame. Nothing but the replay writes those cells. Batches of 128
    frames: a call through the feed tests the frame tiles that neither reach back in front of the batch nor write ring rows, here
    those at frames 32, 48 and 64 of each batch."""
    n, g, lv = 8192, 128, dict(start_level=CULL_LEVEL, engine_level=CULL_LEVEL)
    keys = np.array([0, 5, 255, 256, 4095, 4096, n - 257, n - 1], np.int32)
    iq, t = _stream(n, nframes=400, on=30, off=100)
    a, b = RouteA(n, g, max_batch=128, flags=KEEP, **lv), SparseB(n, g, max_batch=128, **lv)
    quiet = 0
    for k, (lo, hi) in enumerate(_batches(400, (128,))):  # 128 | 128, 128, 16 behind the hand post
        ra = a.batch(iq[lo:hi], t[lo:hi])
        before = _tile_counters(b.eng)
        b.submit(iq[lo:hi], t[lo:hi])
        if k == 0:
            got = b.collect(ra, f"batch {k}")
            assert got["cand_idx"].size > 1000
            b.trk.post_keys(got["seq"], keys)  # (over the tracker's own post)
            b.posted = (got["seq"], keys.copy())
            continue
        got = b.collect(ra, f"quiet batch {k}", track=False, post=False)  # (holds every column of the peaks to the restatement)
        after = _tile_counters(b.eng)
        tested, culled = after["tiles_tested"] - before["tiles_tested"], after["tiles_culled"] - before["tiles_culled"]
        print(f"quiet batch {k}: {got['cand_idx'].size} candidates, tested {tested}, culled {culled}, watch {got['watch'].tolist()}")
        assert got["cand_idx"].size == 0 and ra["idx"].size == 0
        assert culled == tested and (tested > 0 or hi - lo < 128), (k, tested, culled)
        np.testing.assert_array_equal(got["watch"], keys)
        assert got["peak_idx"].shape == (hi - lo, 8) and not np.isnan(got["peak_avg"]).any()
        quiet += 1
    assert 0 < b.check_counters(less=True)["tiles_evaluated"]
    b.close()
    assert quiet == 3


def test_quiet_batches_post_goes_in_behind_the_last_busy_batch():
    """Case 2, the other order: the eight keys posted while candidates still come — the watch list is the keys and the batch's cand_best."""
    n, g = 8192, 128
    keys = np.array([0, 5, 255, 256, 4095, 4096, n - 257, n - 1], np.int32)
    iq, t = _stream(n, nframes=192, on=30, off=100)
    a, b = RouteA(n, g, max_batch=64, flags=KEEP), SparseB(n, g, max_batch=64)
    for k, (lo, hi) in enumerate(_batches(192, (64,))):
        ra = a.batch(iq[lo:hi], t[lo:hi])
        b.submit(iq[lo:hi], t[lo:hi])
        got = b.collect(ra, f"batch {k}", track=False, post=False)
        assert set(keys.tolist()) <= set(got["watch"].tolist()) or k == 0
        b.trk.post_keys(got["seq"], keys)
        b.posted = (got["seq"], keys.copy())
    assert got["cand_idx"].size == 0  # (the last batch is a quiet one)
    b.check_counters()
    b.close()


@pytest.mark.parametrize("g,sizes,nframes", [(2048, (7, 64, 1, 100), 172), (128, (3, 16, 5, 35, 1), 150)])
def test_wide_windows_and_tiles_that_reach_back(g, sizes, nframes):
    """Case 3: nine columns per key with overlapping windows; and cuts that start batches off the tile grid, the first one inside the
    learning phase (280 ms = 7 frames), with a batch of one frame."""
    iq, t = _stream(8192, nframes=nframes)
    total, tx, lags, tiles_b, _, stats = _in_flight(8192, iq, t, sizes, 128, g=g)
    assert total > 1000 and tx > 0


def test_small_transform_in_order_path():
    """Case 4: 1024 points — the stand-alone detect launch, no culling."""
    iq, t = _stream(1024, nframes=170, on=28, off=110, seed=21)
    total, tx, lags, tiles_b, _, stats = _in_flight(1024, iq, t, (1, 16, 7, 3, 16, 16, 5), 16)
    assert tx > 100 and 2 in lags and tiles_b["tiles_culled"] == 0


def test_spectrogram_context_accumulates_nothing_twice():
    """Case 5: SS_FLAG_SPECTROGRAM + sparse tracking + feed.spectrogram(): the rows of every batch byte-equal to those of an engine with
    the flag and no tracker, the engine's own accumulator too, and the digest as everywhere."""
    n, g, sizes = 2048, 128, (64, 40, 64, 7, 64, 33)
    iq, t = _stream(n, nframes=sum(sizes))
    a, b = RouteA(n, g, max_batch=64, flags=KEEP), SparseB(n, g, max_batch=64, flags=SPEC)
    c = Untracked(n, 64, flags=SPEC)
    sg_b, sg_c = b.feed.spectrogram(max_rows=8, want_mean=True), c.feed.spectrogram(max_rows=8, want_mean=True)
    rows = 0
    for k, (lo, hi) in enumerate(_batches(sum(sizes), sizes)):
        ra = a.batch(iq[lo:hi], t[lo:hi])
        b.submit(iq[lo:hi], t[lo:hi])
        b.collect(ra, f"batch {k}")
        c.batch(iq[lo:hi], t[lo:hi])
        rb, rc = sg_b.rows(), sg_c.rows()
        assert (rb["nrows"], rb["size"], rb["open_count"]) == (rc["nrows"], rc["size"], rc["open_count"]), (k, rb["nrows"], rc["nrows"])
        for field in ("time_ms", "frame", "count", "rows", "mean"):
            assert np.asarray(rb[field]).tobytes() == np.asarray(rc[field]).tobytes(), (k, field)
        assert rb["payloads"]() == rc["payloads"]()
        rows += rb["nrows"]
    assert rows >= 8
    b.eng.sync()
    c.eng.sync()
    row_b, mean_b, cnt_b = b.eng.spectrogram_read()
    row_c, mean_c, cnt_c = c.eng.spectrogram_read()
    assert cnt_b == cnt_c and row_b.tobytes() == row_c.tobytes() and mean_b.tobytes() == mean_c.tobytes()
    b.check_counters()
    sg_b.close()
    sg_c.close()
    b.close()


def test_no_cull_context():
    """Case 6: SS_FLAG_NO_CULL at 8192 points is accepted and digests the same."""
    iq, t = _stream(8192, nframes=100)
    total, tx, lags, tiles_b, _, stats = _in_flight(8192, iq, t, (7, 64, 29), 64, flags_b=NO_CULL)
    assert total > 1000 and tiles_b["tiles_culled"] == 0


def test_watch_list_overflow():
    """Case 7: 64 posted keys and room for 64: the first candidates overflow the list — the batch says so, nothing is replayed for it —
    and after a post that cuts the list back the next batch is digested correctly."""
    n, g = 8192, 128
    iq, t = _stream(n, nframes=128)
    a, b = RouteA(n, g, max_batch=64, flags=KEEP), SparseB(n, g, max_batch=64, max_watch=64)
    many = (64 + 128 * np.arange(64)).astype(np.int32)  # every tile column
    b.trk.post_keys(0, many)
    b.posted = (0, many.copy())
    ra = a.batch(iq[:64], t[:64])
    b.submit(iq[:64], t[:64])
    got = b.trk.collect()
    want = np.unique(np.concatenate([many, ra["digest"]["cand_best"]])).size
    assert got["digest_status"] == INVALID and got["nwatch"] == want and want > 64 and got["watch"].size == 0, (got["digest_status"], got["nwatch"], want)
    np.testing.assert_array_equal(got["cand_best"], ra["digest"]["cand_best"])
    b.best[1] = got["cand_best"]
    b.ref.digest(ra["rel"], ra["avg"], ra["off"], ra["idx"], many)  # (the restatement keeps this batch's last rel rows for the next one)
    b.count(got)
    assert b.check_counters()["tiles_evaluated"] == 0
    few = np.array([100, 4000], np.int32)
    b.trk.post_keys(1, few)
    b.posted = (1, few.copy())
    ra = a.batch(iq[64:], t[64:])
    b.submit(iq[64:], t[64:])
    got = b.collect(ra, "the batch behind the overflow", track=False, post=False)
    assert 2 <= got["watch"].size <= 64
    b.check_counters()
    b.close()


def test_refusals_and_a_planes_engine():
    """Case 8."""
    def refused(call, word, status=INVALID):
        with pytest.raises(pkg.abi.SpecscanError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)
    mk = lambda n=1024, **kw: pkg.SpectrumEngine(n * 250, CENTER, fft_size=n, decim=1, max_batch=16, learn_ms=280, **kw)  # noqa: E731
    refused(lambda: mk(grouping_y=9).feed(depth=3).track(40, sparse=True), "unfused")
    refused(lambda: mk(flags=REF_NAN).feed(depth=3).track(128, sparse=True), "REFERENCE_NAN")
    refused(lambda: mk(65536, in_format=pkg.abi.SS_FMT_CS8).feed(depth=2, cand_cap=1 << 16).track(128, sparse=True), "65536")
    refused(lambda: mk().feed(depth=3, cand_cap=0).track(128, sparse=True), "cand_cap")  # (and what stf_create refuses)
    refused(lambda: mk().feed(depth=3).track(128, max_watch=0, sparse=True), "max_watch")
    refused(lambda: mk().feed(depth=3).track(128), "KEEP_PLANES")  # stf_create itself is unchanged
    # on an engine that keeps its planes sparse=True is stf_create: the digest is st_digest's in lock-step, and there is nothing to count
    n, g = 256, 128
    iq, t = _stream(n)
    a, b = RouteA(n, g, flags=KEEP), SparseB(n, g, flags=KEEP)
    refused(b.trk.sparse_stats, "not a sparse object")
    plain = RouteB(n, g, flags=KEEP)
    refused(plain.trk.sparse_stats, "not a sparse object")
    plain.close()
    total = 0
    for k, (lo, hi) in enumerate(_batches(len(t), (7, 64, 1, 30))):
        ra = a.batch(iq[lo:hi], t[lo:hi])
        RouteB.submit(b, iq[lo:hi], t[lo:hi])
        got = RouteB.collect(b, ra, f"batch {k}")
        assert_digest_equal(got, ra["digest"], f"batch {k} against st_digest")
        total += got["cand_idx"].size
    b.close()
    assert total > 100


def test_replay_tool_track_sparse(tmp_path):
    """Case 9: specscan_replay --track-sparse reports what --track reports, and the two counters."""
    n = 1024
    fs, nframes, batch, learn = n * 250, 400, 64, 30
    iq = pkg.synth.SyntheticBand(n, seed=21, on_frame=60, off_frame=300).frames_cf32(nframes)
    path = tmp_path / replay.make_raw_file_name("full", "fc", CENTER, fs, time.struct_time((2025, 3, 7, 9, 5, 1, 0, 0, -1)))[2:]
    sink = replay.RawFileSink(8)
    sink.start_recording(str(path))
    sink.work(iq)
    sink.close()
    tool = pkg.build.build_replay_tool()
    reports = {}
    for flag in ("--track", "--track-sparse"):
        r = subprocess.run([tool, str(path), "--fft", str(n), "--decim", "1", "--batch", str(batch), "--learn-frames", str(learn), flag, "--bandwidth", "32000"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        reports[flag] = json.loads(r.stdout.strip().splitlines()[-1])
    dense, sparse = reports["--track"], reports["--track-sparse"]
    print(dense, sparse)
    for key in ("frames", "batches", "candidates", "transmissions", "tracked_frames"):
        assert sparse[key] == dense[key], (key, sparse[key], dense[key])
    assert sparse["transmissions"] > 50 and "tiles_evaluated" not in dense
    assert sparse["tiles_in_batches"] == sum(((hi - lo) + lo % TILE_F + TILE_F - 1) // TILE_F for lo, hi in _batches(nframes, (batch,))) * (n // TILE_B)
    assert 0 < sparse["tiles_evaluated"] <= sparse["tiles_in_batches"], sparse  # (four columns: the three signals may touch them all)
