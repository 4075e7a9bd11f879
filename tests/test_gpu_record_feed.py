"""The recorder bound to the pipelined feed (include/specscan_record_feed.h) on the GPU. Run with -m gpu.

srf_record channelises sample ranges of the batch that was collected last from the feed slot's own upload; a plain Channelizer fed
the same samples through process_ranges is the reference, byte for byte. N = 256, decim 1, max_batch 64, fs 1 024 000, recording
bandwidth 16 000, CF32 and CS8, six batches, through ss_feed_collect and through stf_collect; the hold (acquire and the next
collect refused until record or release; depth 2 still makes progress), a producer and a consumer thread, every srf_create refusal,
ss_feed_destroy first, and track -> RangePlanner -> record end to end against per-range start / process / stop."""
import queue
import threading

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd.abi import SpecscanError
from rtl_sdr_scanner_cpp_amd.channelizer import Channelizer
from rtl_sdr_scanner_cpp_amd.recorder import RangePlanner

pytestmark = pytest.mark.gpu

N, FS, BW, CENTER, MAX_BATCH = 256, 1_024_000, 16_000, 145_000_000, 64
KEEP = pkg.abi.SS_FLAG_KEEP_PLANES
INVALID = pkg.abi.SS_ERR_INVALID
SIZES = (64, 40, 64, 7, 64, 33)  # frames per batch
FORMATS = {"cf32": (pkg.abi.SS_FMT_CF32, "frames_cf32"), "cs8": (pkg.abi.SS_FMT_CS8, "frames_cs8")}
# per channel, in samples of the whole stream; they run across batch boundaries (16384, 26624, 43008, 44800, 61184)
GLOBAL = [(0, 100_000, 1_000, 30_001), (1, -250_000, 16_384 - 5, 20_480), (1, -250_000, 43_900, 60_000), (0, 7_000, 44_801, 44_802),
          (2, 30_000, 61_184, 61_184 + 33 * N)]

_streams = {}


def _frames(name, nframes=sum(SIZES)):
    if name not in _streams:
        iq = getattr(pkg.synth.SyntheticBand(N, seed=5, on_frame=30, off_frame=10_000), FORMATS[name][1])(nframes)
        iq.setflags(write=False)
        _streams[name] = iq
    return _streams[name]


def _edges():
    e = np.concatenate([[0], np.cumsum(SIZES)])
    return list(zip(e[:-1], e[1:]))


def _cut(lo, hi):
    """The ranges of batch [lo, hi) (frames) in its own samples, in GLOBAL's order."""
    a, b = lo * N, hi * N
    return [(ch, sh, max(g0, a) - a, min(g1, b) - a) for ch, sh, g0, g1 in GLOBAL if max(g0, a) < min(g1, b)]


def _engine(name, **kw):
    return pkg.SpectrumEngine(FS, CENTER, fft_size=N, decim=1, max_batch=MAX_BATCH, learn_ms=280, in_format=FORMATS[name][0], **kw)


def _same(got, want, what):
    (ga, grc), (wa, wrc) = got, want
    assert list(grc) == list(wrc) and sorted(ga) == sorted(wa), (what, list(grc), list(wrc))
    for k in ga:
        assert ga[k][0].tobytes() == wa[k][0].tobytes(), (what, k, "int8")
        assert (ga[k][1] is None) == (wa[k][1] is None), what
        if ga[k][1] is not None:
            assert ga[k][1].tobytes() == wa[k][1].tobytes(), (what, k, "cf32")


def _flat(batch):
    return batch.reshape(-1) if batch.dtype == np.complex64 else batch.reshape(-1, 2)


@pytest.mark.parametrize("tracked", [False, True], ids=["ss_feed_collect", "stf_collect"])
@pytest.mark.parametrize("name", list(FORMATS))
def test_record_equals_process_ranges_on_the_same_samples(name, tracked):
    iq = _frames(name)
    eng = _engine(name, flags=KEEP if tracked else 0)
    feed = eng.feed(depth=3, cand_cap=1 << 16)
    trk = feed.track(128) if tracked else None
    rec = feed.record(BW, channels=4, want_cf32=True)
    ref = Channelizer(FS, BW, in_format=FORMATS[name][0], channels=4, max_samples=MAX_BATCH * N)
    edges = _edges()
    t = (1_000 + 40 * np.arange(len(iq))).astype(np.int64)
    recorded = 0
    for k, (lo, hi) in enumerate(edges):  # one batch ahead of the collect: the held slot and the one being filled differ
        for j in ([0, 1] if k == 0 else [k + 1] if k + 1 < len(edges) else []):
            a, b = edges[j]
            buf = feed.acquire()
            buf[:b - a] = iq[a:b]
            feed.submit(b - a, t_ms=t[a:b], tag=j)
        got = trk.collect() if tracked else feed.collect()
        assert got["nframes"] == hi - lo and got["tag"] == k
        ranges = _cut(lo, hi)
        if not ranges:
            rec.release()
            continue
        out = rec.record(ranges)
        _same(out, ref.process_ranges(_flat(iq[lo:hi]), ranges), (name, k))
        recorded += int(sum(out[1]))
    assert recorded > (29_000 + 4_000 + 16_000 + 8_000) * BW // FS - 10 and feed.pending == 0
    rec.close()
    if trk:
        trk.close()
    feed.close()
    ref.close()


def test_the_hold_and_progress_at_depth_two():
    iq = _frames("cf32")
    eng = _engine("cf32")
    feed = eng.feed(depth=2, cand_cap=1 << 16)
    rec = feed.record(BW, channels=2)
    ref = Channelizer(FS, BW, channels=2, max_samples=MAX_BATCH * N)
    with pytest.raises(SpecscanError) as e:
        rec.release()  # nothing collected yet
    assert e.value.status == INVALID
    with pytest.raises(SpecscanError) as e:
        rec.record([(0, 0, 0, 10)])
    assert e.value.status == INVALID and "held" in str(e.value)

    def submit(j):
        buf = feed.acquire()
        buf[:32] = iq[32 * j:32 * j + 32]
        feed.submit(32, tag=j)

    submit(0)
    submit(1)
    for k in range(6):
        assert feed.collect()["tag"] == k
        if k < 5:  # slot k % 2 is held and it is the next to hand out (behind the last batch the other, free one is)
            with pytest.raises(SpecscanError) as e:
                feed.acquire()
            assert e.value.status == INVALID and "no free feed slot" in str(e.value)
        with pytest.raises(SpecscanError) as e:
            feed.collect()
        assert e.value.status == INVALID and "held" in str(e.value)
        ranges = [(1, 50_000, 3, 32 * N - k), (0, -100_000, 100 * k, 5_000)]
        if k == 2:
            with pytest.raises(SpecscanError) as e:  # a refused list keeps the batch held and changes nothing
                rec.record(ranges + [(1, 0, 0, 5)])
            assert e.value.status == INVALID
            with pytest.raises(SpecscanError):
                feed.acquire()
        if k == 4:
            rec.release()  # unrecorded: the reference sees nothing of this batch either
        elif k == 5:
            out = rec.record([])  # no ranges: a release
            assert out[0] == {} and len(out[1]) == 0
        else:
            _same(rec.record(ranges), ref.process_ranges(iq[32 * k:32 * k + 32].reshape(-1), ranges, want_cf32=False), k)
        with pytest.raises(SpecscanError):
            rec.release()  # let go already
        if k + 2 < 6:
            submit(k + 2)  # progress: the slot just let go is free again
    assert feed.pending == 0
    rec.close()
    buf = feed.acquire()  # without a recorder nothing is held
    buf[:8] = iq[:8]
    feed.submit(8)
    feed.collect()
    feed.acquire()
    feed.submit(8)
    feed.collect()
    feed.close()
    ref.close()


def test_producer_and_consumer_threads():
    name = "cs8"
    iq = _frames(name)
    eng = _engine(name)
    depth = 3
    feed = eng.feed(depth=depth, cand_cap=1 << 16)
    rec = feed.record(BW, channels=4, want_cf32=True)
    ref = Channelizer(FS, BW, in_format=FORMATS[name][0], channels=4, max_samples=MAX_BATCH * N)
    edges = _edges() * 3  # eighteen batches, the stream three times over
    free, submitted, errors = threading.Semaphore(depth), queue.Queue(), []

    def producer():
        try:
            for j, (a, b) in enumerate(edges):
                free.acquire()  # a slot that is neither pending nor held
                buf = feed.acquire()
                buf[:b - a] = iq[a:b]
                feed.submit(b - a, tag=j)
                submitted.put(j)
        except Exception as ex:  # noqa: BLE001
            errors.append(ex)
        submitted.put(None)

    th = threading.Thread(target=producer, daemon=True)
    th.start()
    results = []
    try:
        while True:
            j = submitted.get()
            if j is None:
                break
            got = feed.collect()
            assert got["tag"] == j
            lo, hi = edges[j]
            ranges = _cut(lo, hi)
            results.append((j, ranges, rec.record(ranges)))  # (no ranges: a release)
            free.release()
    finally:
        for _ in edges:  # (a failure above must not leave the producer waiting for a slot)
            free.release()
    th.join()
    assert not errors, errors
    assert len(results) == len(edges)
    for j, ranges, out in results:  # the reference afterwards, in the same order: the recording never waited for it
        if ranges:
            lo, hi = edges[j]
            _same(out, ref.process_ranges(_flat(iq[lo:hi]), ranges), j)
    rec.close()
    feed.close()
    ref.close()


def test_create_refusals():
    eng = _engine("cf32")
    feed = eng.feed(depth=2, cand_cap=1 << 10)
    for kw, word in ((dict(channels=17), "channels"), (dict(channels=0), "channels"), (dict(bandwidth=0), "bandwidth"), (dict(threshold=1), "threshold")):
        with pytest.raises(SpecscanError) as e:
            feed.record(kw.pop("bandwidth", BW), **kw)
        assert e.value.status == INVALID and word in str(e.value), (kw, str(e.value))
    feed.acquire()[:] = 0
    with pytest.raises(SpecscanError) as e:
        feed.record(BW)  # a slot is being filled
    assert e.value.status == INVALID and "pending" in str(e.value)
    feed.submit(4)
    with pytest.raises(SpecscanError) as e:
        feed.record(BW)
    assert e.value.status == INVALID and "pending" in str(e.value)
    feed.collect()
    rec = feed.record(BW)
    with pytest.raises(SpecscanError) as e:
        feed.record(BW)
    assert e.value.status == INVALID and "already has a recorder" in str(e.value)
    rec.close()
    rec = feed.record(BW)  # the place is free again
    rec.close()
    feed.close()
    dec = pkg.SpectrumEngine(FS, CENTER, fft_size=N, decim=2, max_batch=8)
    dfeed = dec.feed(depth=2, cand_cap=1 << 10)
    with pytest.raises(SpecscanError) as e:
        dfeed.record(BW)
    assert e.value.status == INVALID and "decim" in str(e.value)
    dfeed.close()


def test_feed_destroyed_first():
    iq = _frames("cf32")
    eng = _engine("cf32")
    feed = eng.feed(depth=2, cand_cap=1 << 10)
    rec = feed.record(BW, channels=2)
    buf = feed.acquire()
    buf[:16] = iq[:16]
    feed.submit(16)
    feed.collect()
    out, rc = rec.record([(0, 100_000, 0, 16 * N)])
    assert rc[0] == 16 * N * BW // FS and len(out[0][0]) == rc[0]
    feed.close()
    for call in (lambda: rec.record([(0, 0, 0, 10)]), rec.release):
        with pytest.raises(SpecscanError) as e:
            call()
        assert e.value.status == INVALID and "destroyed" in str(e.value)
    rec.close()


def test_track_plan_record_end_to_end():
    """A SyntheticBand stream through the tracked feed, the host tracker, RangePlanner and srf_record, against the classic route on
    the same samples: per range sc_start / sc_process / sc_stop at the frame boundaries the planner found. Both routes restart a
    channel's filter at the same samples, so the records (what a slot has gathered when a range ends with a flush) are compared as
    bytes, in order."""
    nframes, g = 150, 128
    iq = pkg.synth.SyntheticBand(N, seed=5, on_frame=30, off_frame=110).frames_cf32(nframes)
    t = (1_000 + 40 * np.arange(nframes)).astype(np.int64)
    eng = pkg.SpectrumEngine(FS, CENTER, fft_size=N, decim=1, max_batch=MAX_BATCH, learn_ms=280, flags=KEEP)
    feed = eng.feed(depth=3, cand_cap=1 << 20)
    trk = feed.track(g, max_watch=4096)
    rec = feed.record(BW, channels=2)
    tracker = pkg.tracker.SignalTracker(N, FS, group_size=g, min_time_ms=200, timeout_ms=400)
    planner = RangePlanner(2, N)
    classic = Channelizer(FS, BW, channels=2, max_samples=MAX_BATCH * N)
    cuts, at = [], 0
    for size in (7, 64, 1, 30) * 3:
        if at < nframes:
            cuts.append((at, min(nframes, at + size)))
            at = cuts[-1][1]

    def gather(store, records, ranges, ends, flushed, outs):
        """outs[i]: the int8 samples of ranges[i]. A range that ends with a flush publishes what the slot holds, a stop drops what
        is left (recorder.cpp:75-98)."""
        for (ch, shift, _b, _e), why, fl, y in zip(ranges, ends, flushed, outs):
            store[ch].append(y)
            if fl:
                records.append((ch, CENTER + shift, np.concatenate(store[ch]).tobytes()))
            if fl or why == "stop":
                store[ch] = []

    rec_a, rec_b, store_a, store_b = [], [], {0: [], 1: []}, {0: [], 1: []}
    kinds, nranges, spanning = set(), 0, 0
    for lo, hi in cuts:
        buf = feed.acquire()
        buf[:hi - lo] = iq[lo:hi]
        feed.submit(hi - lo, t_ms=t[lo:hi])
        got = trk.collect()
        tx = tracker.process_batch_digest(t[lo:hi], got)
        trk.post_keys(got["seq"], tracker.keys)
        ranges, ends, flushed = planner.plan([[(int(s), bool(f)) for s, f in frame[0]] for frame in tx])
        kinds |= set(ends)
        nranges += len(ranges)
        spanning += sum(1 for r, why in zip(ranges, ends) if why == "batch" and r[2] == 0 and hi - lo > 1)
        out, rc = rec.record(ranges)  # (no ranges: a release)
        used, outs = {0: 0, 1: 0}, []
        for (ch, *_), n in zip(ranges, rc):
            outs.append(out[ch][0][used[ch]:used[ch] + n])
            used[ch] += n
        gather(store_a, rec_a, ranges, ends, flushed, outs)
        x = iq[lo:hi].reshape(-1)
        outs = []
        for ch, shift, b, e in ranges:  # the classic route: one call per range, start and stop around it
            classic.start(ch, shift)
            outs.append(classic.process(x[b:e], want_cf32=False)[ch][0])
            classic.stop(ch)
        gather(store_b, rec_b, ranges, ends, flushed, outs)
    print(f"end to end: {nranges} ranges, ends {sorted(kinds)}, {spanning} whole-batch ranges, {len(rec_a)} records, "
          f"{sum(len(r[2]) for r in rec_a) // 2} samples published")
    # the band's transmissions last 80 frames, longer than any batch and than min_time: recordings span batches and flush
    assert nranges > 0 and kinds == {"stop", "batch"} and spanning > 0 and len(rec_a) > 0
    assert [(r[0], r[1], len(r[2])) for r in rec_a] == [(r[0], r[1], len(r[2])) for r in rec_b]
    assert rec_a == rec_b
    assert sum(len(r[2]) for r in rec_a) > 0
    rec.close()
    trk.close()
    feed.close()
    classic.close()
