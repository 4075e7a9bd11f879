"""The tracked feed on the GPU (include/specscan_track_feed.h, csrc/track_feed.h): every batch submitted through a feed with an
stf_ctx is digested in the stream and delivered by stf_collect.

Route A — existing code, not under test — is a second engine on the same frames with the same batch cuts: eng.process with the rel and
avg planes, TrackDigest.digest (st_digest), one tracker on the digest and one on the planes. Route B is the tracked feed. In lock-step
(submit, collect, post, repeat) the device's watch list is route A's and the whole digest must equal st_digest's; with batches in flight
the watch list must be sort(unique(K_p U cand_best(p + 1 .. k))) computed here from what was posted and collected, and the digest must
equal the numpy restatement (tests/digest_ref.py) on route A's planes with keys = that list — every column, the extra ones too.
Integers equal, floats bit-equal: no tolerance anywhere. Needs an MI355X: run with -m gpu."""
import json
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import replay
from digest_ref import DigestRef, assert_digest_equal

pytestmark = pytest.mark.gpu

KEEP = pkg.abi.SS_FLAG_KEEP_PLANES
CENTER = 145_000_000
INVALID = pkg.abi.SS_ERR_INVALID
TK = dict(min_time_ms=200, timeout_ms=400)


def _batches(nframes, sizes):
    edges, k = [0], 0
    while edges[-1] < nframes:
        edges.append(min(nframes, edges[-1] + sizes[k % len(sizes)]))
        k += 1
    return list(zip(edges[:-1], edges[1:]))


def _stream(n, frames="frames_cf32", nframes=150, on=30, off=10_000, seed=5, zero_frame=None):
    iq = getattr(pkg.synth.SyntheticBand(n, seed=seed, on_frame=on, off_frame=off), frames)(nframes)
    if zero_frame is not None:
        iq[zero_frame] = 0
    return iq, (1_000 + 40 * np.arange(nframes)).astype(np.int64)


class RouteA:
    """eng.process with planes + st_digest + the two trackers, batch by batch; everything a later comparison needs is kept."""

    def __init__(self, n, g, start_level=8.0, gy=21, max_batch=64, engine_level=None, **cfg):
        self.n, self.fs = n, n * 250
        if engine_level is not None:  # (the engine detects at another level than the reference's 8 dB too)
            cfg["start_level"] = engine_level
        self.eng = pkg.SpectrumEngine(self.fs, CENTER, fft_size=n, decim=1, max_batch=max_batch, learn_ms=280, grouping_y=gy, **cfg)
        self.dig = self.eng.track_digest(g, start_level=start_level, max_watch=8192)
        self.tr_digest = pkg.tracker.SignalTracker(n, self.fs, group_size=g, grouping_y=gy, start_level=start_level, **TK)
        self.tr_planes = pkg.tracker.SignalTracker(n, self.fs, group_size=g, grouping_y=gy, start_level=start_level, **TK)
        self.out = []

    def batch(self, iq, t):
        r = self.eng.process(iq, t_ms=t)
        d = self.dig.digest(r["cand_off"], r["cand_idx"], self.tr_digest.keys)
        self.tr_digest.process_batch_digest(t, d)
        tx = self.tr_planes.process_batch(t, r["avg"], r["rel"], r["cand_off"], r["cand_idx"])
        self.out.append(dict(rel=r["rel"], avg=r["avg"], off=r["cand_off"], idx=r["cand_idx"], digest=d, tx=tx, t=t))
        return self.out[-1]

    def reset(self, retune=False):
        if retune:
            self.eng.set_frequency_range(CENTER + self.fs - self.fs // 2, CENTER + self.fs + self.fs // 2)
        self.eng.reset()
        self.dig.reset()
        self.tr_digest.reset()
        self.tr_planes.reset()


class RouteB:
    def __init__(self, n, g, start_level=8.0, gy=21, max_batch=64, depth=3, cand_cap=1 << 20, max_watch=4096, engine_level=None, **cfg):
        self.n, self.fs, self.g, self.gy, self.start = n, n * 250, g, gy, start_level
        if engine_level is not None:
            cfg["start_level"] = engine_level
        self.eng = pkg.SpectrumEngine(self.fs, CENTER, fft_size=n, decim=1, max_batch=max_batch, learn_ms=280, grouping_y=gy, **cfg)
        self.feed = self.eng.feed(depth=depth, cand_cap=cand_cap)
        self.trk = self.feed.track(g, start_level=start_level, max_watch=max_watch)
        self.tracker = pkg.tracker.SignalTracker(n, self.fs, group_size=g, grouping_y=gy, start_level=start_level, **TK)
        self.ref = DigestRef(n, g, start_level, gy)
        self.posted = (0, np.zeros(0, np.int32))  # (p, K_p) as last posted
        self.at_submit = {}                       # seq -> the post the submit found
        self.best = {}                            # seq -> cand_best of that batch
        self.seq = 0
        self.larger = 0

    def submit(self, iq, t):
        buf = self.feed.acquire()
        buf[:len(iq)] = iq
        self.feed.submit(len(iq), t_ms=t)
        self.seq += 1
        self.at_submit[self.seq] = self.posted

    def post(self, seq):
        self.trk.post_keys(seq, self.tracker.keys)
        self.posted = (seq, self.tracker.keys.copy())

    def collect(self, a, what, track=True, post=True):
        """Collect the oldest batch, hold it to the rule and to the restatement on route A's planes `a`, run the tracker, post."""
        got = self.trk.collect()
        seq = got["seq"]
        p, keys = self.at_submit[seq]
        self.best[seq] = got["cand_best"]
        assert got["keys_seq"] == p and got["digest_status"] == 0 and got["status"] == 0, (what, got["keys_seq"], p, got["digest_status"])
        want_watch = np.unique(np.concatenate([keys] + [self.best[q] for q in range(p + 1, seq + 1)])).astype(np.int32)
        np.testing.assert_array_equal(got["watch"], want_watch, err_msg=f"{what}: watch list against K_{p} U cand_best({p + 1}..{seq})")
        assert_digest_equal(got, self.ref.digest(a["rel"], a["avg"], a["off"], a["idx"], got["watch"]), what)
        self.larger += got["watch"].size > a["digest"]["watch"].size
        assert set(a["digest"]["watch"].tolist()) <= set(got["watch"].tolist()) or not post, what
        nf, nc, nw = got["nframes"], got["cand_idx"].size, got["watch"].size
        assert got["d2h_bytes"] == 16 + 8 * nc + 4 * nw + 8 * nf * nw, (what, got["d2h_bytes"])
        if track:
            tx = self.tracker.process_batch_digest(a["t"], got)  # (raises when a tracked key is missing from the watch list)
            for f in range(nf):
                np.testing.assert_array_equal(tx[f][0], a["tx"][f][0], err_msg=f"{what} frame {f}: transmissions")
                np.testing.assert_array_equal(tx[f][1], a["tx"][f][1], err_msg=f"{what} frame {f}: signal keys")
            if post:
                self.post(seq)
        return got

    def reset(self, retune=False):
        assert self.feed.pending == 0
        if retune:
            self.eng.set_frequency_range(CENTER + self.fs - self.fs // 2, CENTER + self.fs + self.fs // 2)
        self.eng.reset()
        self.trk.reset()
        self.tracker.reset()
        self.ref.reset()
        self.posted, self.at_submit, self.best, self.seq = (0, np.zeros(0, np.int32)), {}, {}, 0

    def close(self):
        self.trk.close()
        self.feed.close()


def _lockstep(n, iq, t, sizes, g=128, gy=21, max_batch=64, **cfg):
    """submit, collect, post, repeat: p = k - 1, so W_k is route A's watch list and the whole digest is st_digest's."""
    a, b = RouteA(n, g, gy=gy, max_batch=max_batch, flags=KEEP, **cfg), RouteB(n, g, gy=gy, max_batch=max_batch, flags=KEEP, **cfg)
    total = tx = 0
    for k, (lo, hi) in enumerate(_batches(len(t), sizes)):
        ra = a.batch(iq[lo:hi], t[lo:hi])
        b.submit(iq[lo:hi], t[lo:hi])
        got = b.collect(ra, f"batch {k} [{lo}, {hi})")
        assert_digest_equal(got, ra["digest"], f"batch {k} [{lo}, {hi}) against st_digest")
        assert got["seq"] == k + 1
        total += got["cand_idx"].size
        tx += sum(len(x[0]) for x in ra["tx"])
    assert b.larger == 0
    b.close()
    print(f"lock-step n {n}: {total} candidates, {tx} transmissions")
    return total, tx


def test_lockstep_small_fused_and_unfused():
    iq, t = _stream(256)
    total, _ = _lockstep(256, iq, t, (7, 64, 1, 30), g=128)
    assert total > 100
    total, _ = _lockstep(256, iq, t, (3, 64, 1, 30), g=40, gy=9)  # the unfused back end (rel rows stored), ceil(9 / 2) = 5 rows
    assert total > 100


@pytest.mark.parametrize("flags", [KEEP, KEEP | pkg.abi.SS_FLAG_REFERENCE_NAN])
def test_lockstep_zero_frame_and_the_nan_rows_behind_it(flags):
    iq, t = _stream(2048, nframes=200, on=40, zero_frame=90)
    n, g = 2048, 128
    a, b = RouteA(n, g, flags=flags), RouteB(n, g, flags=flags)
    total = 0
    for k, (lo, hi) in enumerate(_batches(200, (50,))):
        ra = a.batch(iq[lo:hi], t[lo:hi])
        b.submit(iq[lo:hi], t[lo:hi])
        got = b.collect(ra, f"batch {k}")
        assert_digest_equal(got, ra["digest"], f"batch {k} against st_digest")
        total += got["cand_idx"].size
    b.close()
    assert total > 1000


def test_lockstep_65536_cs8():
    """256 blocks of 256 bins: the scan of the block counts takes more than one count per lane."""
    n = 65536
    iq, t = _stream(n, "frames_cs8", nframes=64)
    total, _ = _lockstep(n, iq, t, (5, 32, 1), g=128, max_batch=32, in_format=pkg.abi.SS_FMT_CS8)
    assert total > 1000


def _in_flight(n, iq, t, sizes, max_batch, reset_after=None, **cfg):
    """Depth 3, two batches in flight, keys posted after every collect: batch k is submitted with the post of batch k - 2."""
    g = 128
    a, b = RouteA(n, g, max_batch=max_batch, flags=KEEP, **cfg), RouteB(n, g, max_batch=max_batch, flags=KEEP, **cfg)
    cuts = _batches(len(t), sizes)
    waiting = []
    total = tx = 0

    def collect_one():
        nonlocal total, tx
        k, ra = waiting.pop(0)
        got = b.collect(ra, f"batch {k} {cuts[k]}")
        total += got["cand_idx"].size
        tx += sum(len(x[0]) for x in ra["tx"])
    for k, (lo, hi) in enumerate(cuts):
        waiting.append((k, a.batch(iq[lo:hi], t[lo:hi])))
        b.submit(iq[lo:hi], t[lo:hi])
        if len(waiting) == 2:
            collect_one()
        if reset_after is not None and k == reset_after:  # drain, retune, ss_reset and stf_reset
            while waiting:
                collect_one()
            a.reset(retune=True)
            b.reset(retune=True)
    while waiting:
        collect_one()
    lags = sorted({s - p for s, (p, _) in b.at_submit.items()})
    b.close()
    print(f"in flight n {n}: {total} candidates, {tx} transmissions, watch list strictly larger than route A's in {b.larger} batches, lags {lags}")
    return total, tx, b.larger, lags


def test_two_batches_in_flight_1024():
    iq, t = _stream(1024, nframes=170, on=28, off=110, seed=21)
    total, tx, larger, lags = _in_flight(1024, iq, t, (1, 16, 7, 3, 16, 16, 5), 16)
    assert tx > 100 and larger >= 1 and 2 in lags


@pytest.mark.parametrize("frames,fmt", [("frames_cf32", pkg.abi.SS_FMT_CF32), ("frames_cs16", pkg.abi.SS_FMT_CS16)])
def test_two_batches_in_flight_8192_and_a_retune(frames, fmt):
    iq, t = _stream(8192, frames, nframes=300)
    total, tx, larger, lags = _in_flight(8192, iq, t, (7, 64, 1, 100), 128, reset_after=3, in_format=fmt)  # batches 7, 64, 1, 100 | reset | 7, 64, 57
    assert total > 1000 and 2 in lags


def test_nothing_posted_then_a_post():
    """Without a post the watch list is every cand_best so far; the post of batch 5 cuts it back to K_5 U cand_best(6 ..)."""
    n = 1024
    iq, t = _stream(n, nframes=170, on=28, off=110, seed=21)
    a, b = RouteA(n, 128, max_batch=16, flags=KEEP), RouteB(n, 128, max_batch=16, flags=KEEP)
    sizes = []
    for k, (lo, hi) in enumerate(_batches(170, (16,))):
        ra = a.batch(iq[lo:hi], t[lo:hi])
        b.submit(iq[lo:hi], t[lo:hi])
        got = b.collect(ra, f"batch {k}", post=False)
        assert got["keys_seq"] == (0 if k < 5 else 5)
        if k < 5:
            np.testing.assert_array_equal(got["watch"], np.unique(np.concatenate([b.best[q] for q in range(1, k + 2)])))
        if k == 4:
            b.post(5)
        sizes.append(got["watch"].size)
    b.close()
    print("watch list sizes:", sizes)
    assert sizes[4] > 0 and sizes[:5] == sorted(sizes[:5]) and b.larger >= 1


def test_long_watch_lists_and_overflow():
    """start_level -30 (engine, digest and tracker alike) makes every in-range bin of every frame behind the warm-up a candidate; the
    range is a quarter of the band, which keeps the restatement's work small, and the windows are 17 bins wide, so that the noise rows'
    votes spread over hundreds of distinct cand_best (the oracle finds 315 in the first batch and 540 after two; windows of 129 bins over
    an eighth of the band gave 92). Two batches of 32 frames, a reset, two more."""
    n, g, fs = 4096, 16, 4096 * 250
    iq, t = _stream(n, nframes=128)
    cuts = _batches(128, (32,))
    kw = dict(start_level=-30.0, engine_level=-30.0, max_batch=32, flags=KEEP)
    a = RouteA(n, g, **kw)
    a.eng.set_frequency_range(CENTER - fs // 8, CENTER + fs // 8)
    for k, (lo, hi) in enumerate(cuts):
        a.batch(iq[lo:hi], t[lo:hi])
        if k == 1:
            a.reset()
    assert a.out[1]["idx"].size > 32 * 800
    b = RouteB(n, g, max_watch=8192, **kw)
    b.eng.set_frequency_range(CENTER - fs // 8, CENTER + fs // 8)
    most = 0
    for k, (lo, hi) in enumerate(cuts):
        b.submit(iq[lo:hi], t[lo:hi])
        got = b.collect(a.out[k], f"batch {k}", track=False)
        most = max(most, got["watch"].size)
        if k == 1:
            b.reset()
    b.close()
    assert most > 256, most  # the list crosses block boundaries
    # the same stream with room for 64 watch keys: the batch says so and nothing else goes wrong ...
    b = RouteB(n, g, max_watch=64, **kw)
    b.eng.set_frequency_range(CENTER - fs // 8, CENTER + fs // 8)
    for k, (lo, hi) in enumerate(cuts[:2]):
        b.submit(iq[lo:hi], t[lo:hi])
        got = b.trk.collect()
        want = np.unique(np.concatenate([a.out[q]["digest"]["cand_best"] for q in range(k + 1)])).size
        assert got["digest_status"] == INVALID and got["nwatch"] == want and want > 64 and got["watch"].size == 0, (k, got["digest_status"], got["nwatch"], want)
        np.testing.assert_array_equal(got["cand_best"], a.out[k]["digest"]["cand_best"])
    # ... and after a drain, ss_reset, stf_reset and a larger tracker the next batches are right again
    b.reset()
    b.trk.close()
    b.trk = b.feed.track(g, start_level=-30.0, max_watch=8192)
    for k, (lo, hi) in list(enumerate(cuts))[2:]:
        b.submit(iq[lo:hi], t[lo:hi])
        b.collect(a.out[k], f"batch {k} behind the overflow", track=False)
    b.close()


def test_feed_with_room_for_64_candidates():
    """SS_ERR_CAND_OVERFLOW leaves truncated lists: the digest covers them, with the offsets clipped."""
    n, g = 1024, 128
    iq, t = _stream(n, nframes=96, on=28, off=110, seed=21)
    a, b = RouteA(n, g, max_batch=16, flags=KEEP), RouteB(n, g, max_batch=16, cand_cap=64, flags=KEEP)
    ref = DigestRef(n, g)
    overflowed = 0
    for k, (lo, hi) in enumerate(_batches(96, (16,))):
        ra = a.batch(iq[lo:hi], t[lo:hi])
        b.submit(iq[lo:hi], t[lo:hi])
        got = b.trk.collect()
        total = int(ra["off"][-1])
        assert got["cand_total"] == total and got["cand_idx"].size == min(total, 64)
        assert got["status"] == (pkg.abi.SS_ERR_CAND_OVERFLOW if total > 64 else 0)
        overflowed += total > 64
        assert_digest_equal(got, ref.digest(ra["rel"], ra["avg"], np.minimum(ra["off"], 64), ra["idx"][:64], got["watch"]), f"batch {k}")
    b.close()
    assert overflowed >= 2


def test_producer_and_consumer_threads_and_the_replay_host(tmp_path):
    """A thread that submits and knows nothing of the tracker, a thread that collects and posts — as host/specscan_replay runs. What
    the submits find posted depends on timing; asserted is what does not: the digest against the restatement with the delivered watch
    list, no tracked key ever missing, the plane tracker's transmissions."""
    n, g = 1024, 128
    iq, t = _stream(n, nframes=170, on=28, off=110, seed=21)
    cuts = _batches(170, (1, 16, 7, 3, 16, 16, 5))
    a, b = RouteA(n, g, max_batch=16, flags=KEEP), RouteB(n, g, max_batch=16, flags=KEEP)
    for lo, hi in cuts:
        a.batch(iq[lo:hi], t[lo:hi])
    free, ready, errors = threading.Semaphore(3), threading.Semaphore(0), []

    def producer():
        try:
            for lo, hi in cuts:
                free.acquire()
                buf = b.feed.acquire()
                buf[:hi - lo] = iq[lo:hi]
                b.feed.submit(hi - lo, t_ms=t[lo:hi], tag=lo)
                ready.release()
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            ready.release()
    th = threading.Thread(target=producer)
    th.start()
    tx = 0
    for k, (lo, hi) in enumerate(cuts):
        ready.acquire()
        assert not errors, errors
        got = b.trk.collect()
        ra = a.out[k]
        assert (got["seq"], got["tag"], got["digest_status"]) == (k + 1, lo, 0) and got["keys_seq"] <= k
        assert_digest_equal(got, b.ref.digest(ra["rel"], ra["avg"], ra["off"], ra["idx"], got["watch"]), f"batch {k}")
        res = b.tracker.process_batch_digest(t[lo:hi], got)
        for f in range(hi - lo):
            np.testing.assert_array_equal(res[f][0], ra["tx"][f][0], err_msg=f"batch {k} frame {f}: transmissions")
            np.testing.assert_array_equal(res[f][1], ra["tx"][f][1], err_msg=f"batch {k} frame {f}: signal keys")
        tx += sum(len(x[0]) for x in res)
        b.trk.post_keys(got["seq"], b.tracker.keys)
        free.release()
    th.join()
    b.close()
    assert tx > 100 and not errors
    # specscan_replay --track on a dump of the same band: the clock is the stream's own (1000 * frame * N / fs ms = 4 ms a frame)
    fs, nframes, batch, learn = n * 250, 400, 64, 30
    iq = pkg.synth.SyntheticBand(n, seed=21, on_frame=60, off_frame=300).frames_cf32(nframes)
    path = tmp_path / replay.make_raw_file_name("full", "fc", CENTER, fs, time.struct_time((2025, 3, 7, 9, 5, 1, 0, 0, -1)))[2:]
    sink = replay.RawFileSink(8)
    sink.start_recording(str(path))
    sink.work(iq)
    sink.close()
    tool = pkg.build.build_replay_tool()
    r = subprocess.run([tool, str(path), "--fft", str(n), "--decim", "1", "--batch", str(batch), "--learn-frames", str(learn), "--track", "--bandwidth", "32000"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=batch, learn_frames=learn, flags=KEEP)
    tracker = pkg.tracker.SignalTracker(n, fs, bandwidth=32000)
    want = 0
    for lo in range(0, nframes, batch):
        res = eng.process(iq[lo:lo + batch])
        tf = 1000 * np.arange(lo, min(nframes, lo + batch), dtype=np.int64) * n // fs
        want += sum(len(x[0]) for x in tracker.process_batch(tf, res["avg"], res["rel"], res["cand_off"], res["cand_idx"]))
    assert (rep["frames"], rep["tracked_frames"], rep["transmissions"]) == (nframes, nframes, want) and want > 50, (rep, want)
    plain = subprocess.run([tool, str(path), "--fft", str(n), "--decim", "1", "--batch", str(batch), "--learn-frames", str(learn)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "transmissions" not in plain.stdout and json.loads(plain.stdout.strip().splitlines()[-1])["candidates"] == rep["candidates"]


def test_error_paths():
    n, fs = 1024, 256_000
    iq, t = _stream(n, nframes=48, on=25)

    def refused(call, word, status=INVALID):
        with pytest.raises(pkg.abi.SpecscanError) as e:
            call()
        assert e.value.status == status and word in str(e.value), str(e.value)
    plain = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=16, learn_ms=280)
    refused(lambda: plain.feed(depth=3).track(128), "KEEP_PLANES")
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=16, flags=KEEP, learn_ms=280)
    refused(lambda: eng.feed(depth=2, cand_cap=0).track(128), "cand_cap")
    feed = eng.feed(depth=3)
    refused(lambda: feed.track(128, max_watch=0), "max_watch")
    refused(lambda: feed.track(1 << 14), "LDS")  # (eleven rows of such windows do not fit a workgroup's LDS)
    buf = feed.acquire()
    buf[:16] = iq[:16]
    feed.submit(16, t_ms=t[:16])
    refused(lambda: feed.track(128), "pending")
    feed.collect()
    trk = feed.track(128, max_watch=512)
    refused(lambda: feed.track(128), "already has a tracker")
    none = np.zeros(0, np.int32)
    refused(lambda: trk.post_keys(1, none), "not collected")  # nothing collected yet
    buf = feed.acquire()
    buf[:16] = iq[16:32]
    feed.submit(16, t_ms=t[16:32])
    refused(lambda: trk.post_keys(1, none), "not collected")  # submitted, not collected
    refused(feed.collect, "stf_collect")
    got = trk.collect()
    assert (got["seq"], got["nframes"], feed.pending) == (1, 16, 0)
    refused(trk.collect, "nothing pending")
    refused(lambda: trk.post_keys(1, np.arange(513, dtype=np.int32) % n), "max_watch")
    refused(lambda: trk.post_keys(1, np.array([n], np.int32)), "outside")
    refused(lambda: trk.post_keys(1, np.array([-1], np.int32)), "outside")
    refused(lambda: trk.post_keys(2, none), "not collected")
    trk.post_keys(1, np.array([5, 5, 3], np.int32))  # any order, duplicates allowed
    buf = feed.acquire()
    buf[:16] = iq[32:48]
    feed.submit(16, t_ms=t[32:48])
    refused(trk.reset, "pending")
    got = trk.collect()
    assert (got["seq"], got["keys_seq"], got["digest_status"]) == (2, 1, 0) and {3, 5} <= set(got["watch"].tolist())
    trk.post_keys(2, none)
    refused(lambda: trk.post_keys(1, none), "older")
    trk.reset()
    refused(lambda: trk.post_keys(1, none), "not collected")  # seq restarts: nothing collected since the reset
    # the feed goes first: the tracker only closes from then on
    feed.close()
    refused(trk.collect, "destroyed")
    refused(lambda: trk.post_keys(0, none), "destroyed")
    refused(trk.reset, "destroyed")
    trk.close()
