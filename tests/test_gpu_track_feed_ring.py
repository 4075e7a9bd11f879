"""The tracked feed at 65536 points and up (include/specscan_track_feed_ring.h: stf_create_ring), on the GPU.

Tested: an engine WITHOUT SS_FLAG_KEEP_PLANES, feed.track(..., sparse=True, ring=True), depth 3 with two batches in flight, keys posted
after every collect. Oracle — existing code, held to tests/digest_ref.py by tests/test_gpu_track_digest_sparse.py — a second engine of
the same configuration on the same frames with the same cuts, driven in lock-step: process_device + sync per batch, the synchronous
st_create_sparse digest, a host SignalTracker of its own. A third engine runs the same device calls with no tracker at all, for the
scan's counters. The feed's watch list is a superset of the lock-step tracker's (K_p U cand_best(p + 1 .. k), checked here from what
was posted and collected, as test_gpu_track_feed.RouteB.collect checks it), so the comparison is RouteB's for a superset: the lists,
cand_best and cand_avg whole; peak_idx / peak_avg in every column the oracle watches; the transmissions of every frame.
Integers equal, floats bit-equal: no tolerance anywhere. Batches carry no clocks (learn_frames = 7 on every engine): a device call has
none. Needs an MI355X: run with -m gpu."""
import json
import subprocess
import time

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import replay
from test_gpu_track_feed import _batches
from test_gpu_track_sparse import SparseB, TILE_B, TILE_F, marked_columns
from test_gpu_track_sparse import _stream as _stream_8192
from test_gpu_track_digest_sparse import Runner, _engine, _stream, _tile_counters, _tracker

pytestmark = pytest.mark.gpu

KEEP, REF_NAN = pkg.abi.SS_FLAG_KEEP_PLANES, pkg.abi.SS_FLAG_REFERENCE_NAN
CF32, CS8 = pkg.abi.SS_FMT_CF32, pkg.abi.SS_FMT_CS8
CENTER = 145_000_000
INVALID = pkg.abi.SS_ERR_INVALID
G = 128


def _restricted(n):
    """test_gpu_track_digest_sparse._oracle_f(restricted=True): 32768 scanned bins around DC, the combs well inside them."""
    return dict(centres=tuple(b / n for b in (-9000, -3000, 4000, 11000))), dict(range_lo=CENTER - 16384 * 250, range_hi=CENTER + 16384 * 250)


class Oracle:
    """The lock-step route: device calls with a sync behind each, st_digest on an st_create_sparse object, the host tracker."""

    def __init__(self, n, fmt, max_batch, **cfg):
        self.n = n
        self.eng = _engine(n, fmt, max_batch, **cfg)
        self.dig = self.eng.track_digest(G, max_watch=4096, sparse=True)
        self.run = Runner(self.eng, True, 8192)
        self.trk = _tracker(n, 8.0)

    def batch(self, iq, t):
        keys = self.trk.keys.copy()
        off, idx, cav = self.run.batch(iq, t)
        d = self.dig.digest(off, idx, keys)
        np.testing.assert_array_equal(d["cand_avg"].view(np.uint32), cav.view(np.uint32))
        return dict(off=off, idx=idx, digest=d, tx=self.trk.process_batch_digest(t, d), t=t)

    def reset(self, retune):
        if retune:
            self.eng.set_frequency_range(CENTER + self.n * 250 - self.n * 125, CENTER + self.n * 250 + self.n * 125)
        self.eng.reset()
        self.dig.reset()
        self.trk.reset()


class RingB:
    """The tested route, with RouteB.collect's rule for the watch list and SparseB's books for the replay's counters."""

    def __init__(self, n, fmt, max_batch, depth=3, track=None, **cfg):
        self.n = n
        self.eng = _engine(n, fmt, max_batch, **cfg)
        self.feed = self.eng.feed(depth=depth, cand_cap=1 << 20)
        self.trk = self.feed.track(G, max_watch=4096, **(track or dict(sparse=True, ring=True)))
        self.tracker = _tracker(n, 8.0)
        self.posted = (0, np.zeros(0, np.int32))
        self.at_submit, self.best, self.seq = {}, {}, 0
        self.frames, self.frame_tiles, self.want_eval, self.want_total = 0, {}, 0, 0
        self.no_plane = []  # per submitted batch: PSD reads refused right behind the submit

    def submit(self, iq):
        buf = self.feed.acquire()
        buf[:len(iq)] = iq
        self.feed.submit(len(iq))
        self.seq += 1
        self.at_submit[self.seq] = self.posted
        self.frame_tiles[self.seq] = (len(iq) + self.frames % TILE_F + TILE_F - 1) // TILE_F
        self.frames += len(iq)
        try:  # (ss_read_window speaks of the batch submitted last, in flight or not)
            self.eng.read_window(pkg.abi.SS_PLANE_PSD, 0, 0, 64)
            self.no_plane.append(False)
        except pkg.abi.SpecscanError as e:
            assert e.status == INVALID and "kept no dB" in str(e), str(e)
            self.no_plane.append(True)

    def collect(self, o, what):
        got = self.trk.collect()
        seq = got["seq"]
        p, keys = self.at_submit[seq]
        self.best[seq] = got["cand_best"]
        assert got["keys_seq"] == p and got["digest_status"] == 0 and got["status"] == 0, (what, got["keys_seq"], p, got["digest_status"], got["status"])
        want_watch = np.unique(np.concatenate([keys] + [self.best[q] for q in range(p + 1, seq + 1)])).astype(np.int32)
        np.testing.assert_array_equal(got["watch"], want_watch, err_msg=f"{what}: watch list against K_{p} U cand_best({p + 1}..{seq})")
        d = o["digest"]
        np.testing.assert_array_equal(got["cand_off"], o["off"], err_msg=f"{what}: lists")
        np.testing.assert_array_equal(got["cand_idx"], o["idx"], err_msg=f"{what}: lists")
        np.testing.assert_array_equal(got["cand_best"], d["cand_best"], err_msg=f"{what}: cand_best")
        np.testing.assert_array_equal(got["cand_avg"].view(np.uint32), d["cand_avg"].view(np.uint32), err_msg=f"{what}: cand_avg")
        np.testing.assert_array_equal(got["feed_cand_avg"].view(np.uint32), d["cand_avg"].view(np.uint32), err_msg=f"{what}: the feed's own cand_avg")
        col = np.searchsorted(got["watch"], d["watch"])
        assert col.size == 0 or (col.max() < got["watch"].size and np.array_equal(got["watch"][col], d["watch"])), f"{what}: the lock-step tracker's keys are watched"
        np.testing.assert_array_equal(got["peak_idx"][:, col], d["peak_idx"], err_msg=f"{what}: peak_idx")
        np.testing.assert_array_equal(got["peak_avg"][:, col].view(np.uint32), d["peak_avg"].view(np.uint32), err_msg=f"{what}: peak_avg")
        assert not np.isnan(got["peak_avg"]).any(), what
        tx = self.tracker.process_batch_digest(o["t"], got)
        for f in range(got["nframes"]):
            np.testing.assert_array_equal(tx[f][0], o["tx"][f][0], err_msg=f"{what} frame {f}: transmissions")
            np.testing.assert_array_equal(tx[f][1], o["tx"][f][1], err_msg=f"{what} frame {f}: signal keys")
        self.trk.post_keys(seq, self.tracker.keys)
        self.posted = (seq, self.tracker.keys.copy())
        ft = self.frame_tiles[seq]
        self.want_total += ft * (self.n // TILE_B)
        self.want_eval += ft * marked_columns(got["watch"], G // 2, self.n)
        return got

    def check_counters(self):
        s = self.trk.sparse_stats()
        print(f"sparse_stats {s}, expected {self.want_eval} of {self.want_total}")
        assert s == {"tiles_evaluated": self.want_eval, "tiles_in_batches": self.want_total}, (s, self.want_eval, self.want_total)
        return s

    def reset(self, retune):
        assert self.feed.pending == 0
        if retune:
            self.eng.set_frequency_range(CENTER + self.n * 250 - self.n * 125, CENTER + self.n * 250 + self.n * 125)
        self.eng.reset()
        self.trk.reset()
        self.tracker.reset()
        self.posted, self.at_submit, self.best, self.seq = (0, np.zeros(0, np.int32)), {}, {}, 0
        self.frames, self.frame_tiles, self.want_eval, self.want_total = 0, {}, 0, 0

    def close(self):
        self.trk.close()
        self.feed.close()


def _in_flight(n, fmt, iq, t, sizes, max_batch, no_plane=(), reset_after=None, before_batch=None, in_flight=2, **cfg):
    """Depth 3, `in_flight` batches in flight, keys posted after every collect. no_plane: the cut sizes after which the call must have
    kept no dB plane, unless the batch starts inside the seven learning frames (behind the start, a reset or ss_reset_noise): such a
    batch must have kept one, whatever its size. before_batch(k, engines): what a test does between two drained batches; true if it
    made the engines learn again. Returns the candidates, the transmissions, those behind the last reset, the lags, the scan's tile
    counters and the replay's."""
    o, b = Oracle(n, fmt, max_batch, **cfg), RingB(n, fmt, max_batch, **cfg)
    c_eng = _engine(n, fmt, max_batch, **cfg)
    c_run = Runner(c_eng, True, 8192)
    cuts = _batches(len(t), sizes)
    waiting, total, tx, tx_behind, most = [], 0, 0, 0, 0
    since, learning = 0, []  # frames since the engines last started to learn; per batch: it starts inside the learning frames

    def collect_one():
        nonlocal total, tx, tx_behind
        k, ro = waiting.pop(0)
        got = b.collect(ro, f"batch {k} {cuts[k]}")
        total += got["cand_idx"].size
        tx += sum(len(x[0]) for x in ro["tx"])
        tx_behind += sum(len(x[0]) for x in ro["tx"])
    for k, (lo, hi) in enumerate(cuts):
        if before_batch and before_batch(k, [o.eng, b.eng, c_eng]):
            assert not waiting
            since = 0
        learning.append(since < 7)
        since += hi - lo
        waiting.append((k, o.batch(iq[lo:hi], t[lo:hi])))
        b.submit(iq[lo:hi])
        c_run.batch(iq[lo:hi], t[lo:hi])
        if len(waiting) == in_flight:
            collect_one()
        if reset_after is not None and k == reset_after:  # drain, retune, ss_reset and stf_reset
            while waiting:
                collect_one()
            most = max(most, b.check_counters()["tiles_evaluated"])
            for r in (o, b):
                r.reset(True)
            c_eng.set_frequency_range(CENTER + n * 250 - n * 125, CENTER + n * 250 + n * 125)
            c_eng.reset()
            since = tx_behind = 0
            assert b.trk.sparse_stats() == {"tiles_evaluated": 0, "tiles_in_batches": 0}
    while waiting:
        collect_one()
    stats = b.check_counters()
    assert 0 < max(most, stats["tiles_evaluated"]) and stats["tiles_evaluated"] < stats["tiles_in_batches"], stats
    assert len(b.no_plane) == len(cuts) == len(learning)
    for (lo, hi), kept_none, learns in zip(cuts, b.no_plane, learning):  # the fast form really ran, and a batch with learning frames kept its plane
        assert not (learns and kept_none) and not (not learns and hi - lo in no_plane and not kept_none), (cuts, b.no_plane, learning)
    tiles_b, tiles_c = _tile_counters(b.eng), _tile_counters(c_eng)
    assert tiles_b == tiles_c, (tiles_b, tiles_c)  # the scan is the one the same device calls run without a tracker
    assert tiles_b == _tile_counters(o.eng), (tiles_b, _tile_counters(o.eng))  # ... and with the synchronous digest behind each
    lags = sorted({s - p for s, (p, _) in b.at_submit.items()})
    b.close()
    print(f"ring feed n {n}: {total} candidates, {tx} transmissions ({tx_behind} behind the last reset), lags {lags}, scan {tiles_b}, replay {stats}, no plane {b.no_plane}")
    return total, tx, tx_behind, lags, tiles_b, stats


def _form_case(n, fmt, sizes, no_plane, restricted=False):
    band, cfg = _restricted(n) if restricted else ({}, {})
    iq, t = _stream(n, fmt, sum(sizes), **band)
    total, tx, _, lags, tiles, stats = _in_flight(n, fmt, iq, t, sizes, max(sizes), no_plane=no_plane, **cfg)
    assert tx > 0 and total > 100 and 2 in lags, (tx, total, lags)


def test_65536_cs8_the_radix_8_fold():
    _form_case(65536, CS8, (7, 16, 40, 9, 16), no_plane=(16, 40))


def test_131072_cs8_the_radix_16_fold():
    _form_case(131072, CS8, (7, 16, 25), no_plane=(16, 25))


def test_65536_cf32_the_culled_chain():
    _form_case(65536, CF32, (7, 16, 40, 9), no_plane=(16, 40))


def test_262144_cf32_range_restricted():
    _form_case(262144, CF32, (7, 16, 25), no_plane=(16, 25), restricted=True)


def test_2_20_cf32_ring_only_range_restricted():
    _form_case(1 << 20, CF32, (7, 16, 16, 9), no_plane=(16,), restricted=True)


def test_ring_wrap_with_two_batches_in_flight():
    """28 batches of 40 frames at 65536 points, CS8: the 1024-row ring's window reaches the buffer's end and is moved to the front while
    two digests are still in the stream. The stream is 160 frames repeated (the combs come and go every 160 frames). Every batch
    behind the first (which holds the learning frames) must have gone through the fold, and the scan's counters are those of the same
    28 device calls with no tracker."""
    n, nframes = 65536, 1120
    base, _ = _stream(n, CS8, 160, period=160)
    iq = np.concatenate([base] * 7)
    t = (1_000 + 40 * np.arange(nframes)).astype(np.int64)
    total, tx, _, lags, tiles, stats = _in_flight(n, CS8, iq, t, (40,), 40, no_plane=(40,))
    assert tx > 0 and total > 100 and 2 in lags


def test_retune_and_resets_behind_a_drain():
    """A retune, ss_reset and stf_reset in mid-run: the retune settles the ring's dB rows in place (settle_ring_db) behind the digests
    of the batches before, the batch after it learns the new centre's ceiling (a plane batch), the batches behind that one take the
    fold again, and the counters start from zero. The combs are on in frames 30 .. 69 and 110 .. 149 and off in between, where the
    reset (frame 72) and the new centre's seven learning frames lie: the tracker finds transmissions on both sides of the retune."""
    n, nframes = 65536, 150
    iq = pkg.synth.SyntheticBand(n, seed=5, on_frame=30, off_frame=70, period=80).frames_cs8(nframes)
    t = (1_000 + 40 * np.arange(nframes)).astype(np.int64)
    total, tx, tx_behind, lags, tiles, stats = _in_flight(n, CS8, iq, t, (7, 16, 40, 9, 16), 40, no_plane=(16, 40), reset_after=3)
    assert total > 100 and 2 in lags and tx_behind > 0 and tx > tx_behind, (total, lags, tx, tx_behind)


def test_plane_and_no_plane_batches_alternate():
    """Cycles of 28 frames: ss_reset_noise, a 12-frame batch (seven learning frames: it keeps its dB plane) whose last four frames
    carry the combs, then a 16-frame batch that keeps none. The kept rows pass from one source to the other both ways, and the next
    batch's cand_best reads them: the plane batch's frames 8 .. 11 reach back over its learning frames into the ring batch before."""
    n, cycles = 65536, 4
    iq = pkg.synth.SyntheticBand(n, seed=5, on_frame=8, off_frame=28, period=28).frames_cs8(28 * cycles)
    t = (1_000 + 40 * np.arange(28 * cycles)).astype(np.int64)

    def before_batch(k, engines):
        if k == 0 or k % 2:
            return False
        for e in engines:
            e.sync()
            e.reset_noise()
        return True
    # One batch in flight: ss_reset_noise waits for the stream, so the run is drained there anyway. A ring batch followed by a plane
    # batch with no wait for the stream between them cannot be made through the public interface: a plane form behind a ring form
    # needs new learning frames, which come from ss_reset_noise (waits for the stream) or a retune to a centre not yet learnt (the
    # next batch uploads a new pass mask and waits for the stream: run_batch, pass_dirty); want_psd is fixed at ss_feed_create and
    # sgf_create wants an idle feed. The other direction — the learning batch's plane, then a ring batch, both digests in the
    # stream — is what every form case above starts with.
    total, tx, _, lags, tiles, stats = _in_flight(n, CS8, iq, t, (12, 16), 16, no_plane=(16,), before_batch=before_batch, in_flight=1)
    assert total > 100


def test_small_sizes_equal_the_sparse_object():
    """stf_create_ring at 8192 points is stf_create_sparse: two engines, the same frames with clocks, every field of every batch and the
    replay's counters equal."""
    n, sizes = 8192, (7, 64, 1, 100)
    iq, t = _stream_8192(n, nframes=172)
    a, b = SparseB(n, G, max_batch=128), SparseB(n, G, max_batch=128)
    b.trk.close()  # (the same books, the other entry point)
    b.feed.close()
    b.feed = b.eng.feed(depth=3, cand_cap=1 << 20)
    b.trk = b.feed.track(G, start_level=8.0, max_watch=4096, sparse=True, ring=True)
    ncand = 0
    for k, (lo, hi) in enumerate(_batches(len(t), sizes)):
        outs = []
        for r in (a, b):
            buf = r.feed.acquire()
            buf[:hi - lo] = iq[lo:hi]
            r.feed.submit(hi - lo, t_ms=t[lo:hi])
            got = r.trk.collect()
            tx = r.tracker.process_batch_digest(t[lo:hi], got)
            r.trk.post_keys(got["seq"], r.tracker.keys)
            outs.append((got, tx))
        (ga, ta), (gb, tb) = outs
        assert sorted(ga) == sorted(gb)
        for key in ga:
            va, vb = np.asarray(ga[key]), np.asarray(gb[key])
            assert va.shape == vb.shape and va.tobytes() == vb.tobytes(), (k, key)
        for f in range(hi - lo):
            np.testing.assert_array_equal(ta[f][0], tb[f][0])
        ncand += ga["cand_idx"].size
    sa, sb = a.trk.sparse_stats(), b.trk.sparse_stats()
    assert sa == sb and 0 < sa["tiles_evaluated"] < sa["tiles_in_batches"], (sa, sb)
    assert ncand > 1000
    a.close()
    b.close()


def test_refusals():
    def refused(call, word, status=INVALID):
        with pytest.raises(pkg.abi.SpecscanError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)
    ring = dict(sparse=True, ring=True)
    mk = lambda n=1024, **kw: pkg.SpectrumEngine(n * 250, CENTER, fft_size=n, decim=1, max_batch=16, learn_ms=280, **kw)  # noqa: E731
    refused(lambda: mk(grouping_y=9).feed(depth=3).track(40, **ring), "unfused")
    refused(lambda: mk(flags=REF_NAN).feed(depth=3).track(128, **ring), "REFERENCE_NAN")
    refused(lambda: mk().feed(depth=3, cand_cap=0).track(128, **ring), "cand_cap")
    refused(lambda: mk().feed(depth=3).track(128, max_watch=0, **ring), "max_watch")
    big = mk(65536, in_format=CS8)
    refused(lambda: big.feed(depth=2, cand_cap=1 << 16).track(128, sparse=True), "65536")  # sparse=True alone is what it was
    feed = big.feed(depth=2, cand_cap=1 << 16)
    trk = feed.track(128, **ring)  # ... and the ring object is accepted there
    refused(lambda: feed.track(128, **ring), "already has")
    assert trk.sparse_stats() == {"tiles_evaluated": 0, "tiles_in_batches": 0}
    trk.close()
    feed.close()
    keep = mk(flags=KEEP)
    kfeed = keep.feed(depth=3)
    ktrk = kfeed.track(128, **ring)  # with the flag it is stf_create
    refused(ktrk.sparse_stats, "not a sparse object")
    ktrk.close()
    kfeed.close()


def test_replay_tool_track_ring(tmp_path):
    """specscan_replay --track-ring on a CS8 dump of 65536 points reports the transmissions --track reports, and the two counters; with
    --record-out both runs publish the same bytes."""
    n = 65536
    fs, nframes, batch, learn = n * 250, 152, 16, 7
    iq = pkg.synth.SyntheticBand(n, seed=21, on_frame=30, off_frame=120).frames_cs8(nframes)
    path = tmp_path / replay.make_raw_file_name("full", "cs8", CENTER, fs, time.struct_time((2025, 3, 7, 9, 5, 1, 0, 0, -1)))[2:]
    sink = replay.RawFileSink(2)
    sink.start_recording(str(path))
    sink.work(iq)
    sink.close()
    tool = pkg.build.build_replay_tool()
    reports, records = {}, {}
    for flag in ("--track", "--track-ring"):
        out = tmp_path / (flag.strip("-") + ".rec")
        r = subprocess.run([tool, str(path), "--fft", str(n), "--decim", "1", "--batch", str(batch), "--learn-frames", str(learn), flag, "--bandwidth", "32000",
                            "--min-time-ms", "200", "--timeout-ms", "400", "--record-out", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        reports[flag] = json.loads(r.stdout.strip().splitlines()[-1])
        records[flag] = out.read_bytes()
    dense, ring = reports["--track"], reports["--track-ring"]
    print(dense, ring)
    for key in ("frames", "batches", "transmissions", "tracked_frames"):
        assert ring[key] == dense[key], (key, ring[key], dense[key])
    assert ring["transmissions"] > 0 and "tiles_evaluated" not in dense
    assert ring["tiles_in_batches"] == sum(((hi - lo) + lo % TILE_F + TILE_F - 1) // TILE_F for lo, hi in _batches(nframes, (batch,))) * (n // TILE_B)
    assert 0 < ring["tiles_evaluated"] < ring["tiles_in_batches"], ring
    assert len(records["--track"]) > 0 and records["--track-ring"] == records["--track"]
    # replay.replay_file(track="ring"): the same route from Python, on the stream's own clock (1000 * frame * N / fs ms)
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=batch, learn_frames=learn, **replay.engine_overrides_for(replay.parse_raw_file_name(str(path))))
    tracker = pkg.tracker.SignalTracker(n, fs, bandwidth=32000, min_time_ms=200, timeout_ms=400)
    seen = dict(tx=0)

    def track(out):
        tf = 1000 * (out["first_frame"] + np.arange(out["nframes"], dtype=np.int64)) * n // fs
        seen["tx"] += sum(len(x[0]) for x in tracker.process_batch_digest(tf, out))
        return tracker.keys
    batches = list(replay.replay_file(eng, str(path), batch=batch, track="ring", track_group_size=128, track_keys=track))
    assert sum(b["nframes"] for b in batches) == nframes and seen["tx"] == ring["transmissions"], (seen, ring["transmissions"])
    with pytest.raises(pkg.abi.SpecscanError):  # the last batch kept no dB plane: the fold ran from Python too
        eng.read_window(pkg.abi.SS_PLANE_PSD, 0, 0, 64)
