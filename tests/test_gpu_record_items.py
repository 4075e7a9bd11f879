"""Recording from a decimated scan on the GPU: the whole-item feed (ss_feed_create_items), srf_record on it, and
sc_process_ranges_upload. Run with -m gpu.

An items feed keeps the stream's items of N * decim samples in its pinned slots and uploads their first N samples for the scan, so
the scan is an ordinary feed's, byte for byte; srf_record uploads only the union of the ranges it is given and must equal a plain
Channelizer.process_ranges on the batch's whole item stream, byte for byte. N = 256, fs 1 024 000, recording bandwidth 16 000,
max_batch 64, batches of (64, 40, 7, 33) items, CF32 and CS8, decim 2 and 5. The stream is SyntheticBand(N) frames taken decim at
a time as items. Every comparison is byte equality."""
import queue
import threading

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd.abi import SpecscanError
from rtl_sdr_scanner_cpp_amd.channelizer import Channelizer
from rtl_sdr_scanner_cpp_amd.recorder import RangePlanner

pytestmark = pytest.mark.gpu

A = pkg.abi
N, FS, BW, CENTER, MAX_BATCH = 256, 1_024_000, 16_000, 145_000_000, 64
KEEP, SPEC = A.SS_FLAG_KEEP_PLANES, A.SS_FLAG_SPECTROGRAM
INVALID = A.SS_ERR_INVALID
SIZES = (64, 40, 7, 33)  # items per batch
FORMATS = {"cf32": (A.SS_FMT_CF32, "frames_cf32"), "cs8": (A.SS_FMT_CS8, "frames_cs8"), "cu8": (A.SS_FMT_CU8, "frames_cu8"),
           "cs16": (A.SS_FMT_CS16, "frames_cs16")}
D5 = 5
ITEM = N * D5
# Per channel, in samples of the whole item stream at decim 5 (an item is 1280 samples, its frame the first 256); the batches end at
# 81 920, 133 120, 142 080 and 184 320. Channel 0 stays idle in front of the others.
GLOBAL = [
    (1, 100_000, 3 * ITEM + 300, 3 * ITEM + 1_200),              # wholly in the samples the scan drops, between two frames
    (2, -250_000, 59 * ITEM + 77, 66 * ITEM + 900),              # from an odd sample inside a frame, over a batch boundary, into an item's tail
    (1, 100_000, 80_000, 90_001),                                # overlaps channel 2 in time, another shift
    (3, 30_000, 100_000, 120_000),
    (3, -40_000, 120_000, 150_000),                              # a retune in place, over two batch boundaries
    (1, 7_000, 133_121, 133_122),                                # one sample
    (2, -250_000, 170_000, 184_320),                             # to the end of the stream
]

_streams = {}


def _items(name, decim, nitems=sum(SIZES)):
    """[nitems, N * decim] (CF32) or [nitems, N * decim, 2]: SyntheticBand(N) frames, decim at a time."""
    key = (name, decim, nitems)
    if key not in _streams:
        # (the combs come on at item 60 / decim: behind the 280 ms = 7 items of noise learning at every decim used here)
        iq = getattr(pkg.synth.SyntheticBand(N, seed=5, on_frame=60, off_frame=10_000), FORMATS[name][1])(nitems * decim)
        iq = iq.reshape((nitems, N * decim) + iq.shape[2:])
        iq.setflags(write=False)
        _streams[key] = iq
    return _streams[key]


def _edges(sizes=SIZES):
    e = np.concatenate([[0], np.cumsum(sizes)])
    return [(int(a), int(b)) for a, b in zip(e[:-1], e[1:])]


def _cut(lo, hi, ranges=GLOBAL, item=ITEM):
    """The ranges of batch [lo, hi) (items) in its own samples, in the list's order."""
    a, b = lo * item, hi * item
    return [(ch, sh, max(g0, a) - a, min(g1, b) - a) for ch, sh, g0, g1 in ranges if max(g0, a) < min(g1, b)]


def _union(ranges):
    """How many samples the ranges cover together."""
    if not ranges:
        return 0
    seen = np.zeros(max(r[3] for r in ranges), bool)
    for _ch, _sh, b, e in ranges:
        seen[b:e] = True
    return int(seen.sum())


def _engine(name, decim, **kw):
    return pkg.SpectrumEngine(FS, CENTER, fft_size=N, decim=decim, max_batch=MAX_BATCH, learn_ms=280, in_format=FORMATS[name][0], **kw)


def _flat(batch):
    return batch.reshape(-1) if batch.dtype == np.complex64 else batch.reshape(-1, 2)


def _same(got, want, what):
    (ga, grc), (wa, wrc) = got, want
    assert list(grc) == list(wrc) and sorted(ga) == sorted(wa), (what, list(grc), list(wrc))
    for k in ga:
        assert ga[k][0].tobytes() == wa[k][0].tobytes(), (what, k, "int8")
        assert (ga[k][1] is None) == (wa[k][1] is None), what
        if ga[k][1] is not None:
            assert ga[k][1].tobytes() == wa[k][1].tobytes(), (what, k, "cf32")


def _clock(n):
    return (1_000 + 40 * np.arange(n)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the scan does not change
# ---------------------------------------------------------------------------------------------------------------------------
def _scan(feed, fill, edges, t):
    out = []
    for j, (a, b) in enumerate(edges):
        buf = feed.acquire()
        fill(buf, a, b)
        feed.submit(b - a, t_ms=t[a:b], tag=j)
        r = feed.collect()
        assert r["nframes"] == b - a and r["tag"] == j
        out.append({k: np.array(r[k]) for k in ("cand_off", "cand_idx", "cand_avg", "psd")} | {"status": r["status"]})
    return out


def _scans_equal(a, b, what):
    assert a["status"] == b["status"], what
    for k in ("cand_off", "cand_idx", "cand_avg", "psd"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]) and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("decim", [2, 5])
@pytest.mark.parametrize("name", ["cf32", "cs8"])
def test_the_scan_of_an_items_feed_is_an_ordinary_feeds(name, decim):
    iq = _items(name, decim)
    t, edges, cap = _clock(len(iq)), _edges(), 1 << 16
    e_items, e_plain, e_proc = (_engine(name, decim) for _ in range(3))
    f_items = e_items.feed(depth=2, cand_cap=cap, want_psd=True, items=True)
    f_plain = e_plain.feed(depth=2, cand_cap=cap, want_psd=True)
    assert f_items.items and not f_plain.items
    buf = f_items.acquire()  # (acquiring twice hands out the same buffer)
    assert buf.shape == (MAX_BATCH, N * decim) + iq.shape[2:] and buf.dtype == iq.dtype
    assert f_plain.acquire().shape == (MAX_BATCH, N) + iq.shape[2:]

    def whole(buf, a, b):
        buf[:b - a] = iq[a:b]

    def first_n(buf, a, b):
        buf[:b - a] = iq[a:b, :N]

    got_items, got_plain = _scan(f_items, whole, edges, t), _scan(f_plain, first_n, edges, t)
    total = 0
    for k, (a, b) in enumerate(edges):
        _scans_equal(got_items[k], got_plain[k], (name, decim, k, "feeds"))
        p = e_proc.process(iq[a:b], t_ms=t[a:b], want=("psd",), cand_cap=cap)
        want = {"status": p["status"], "cand_off": p["cand_off"], "cand_idx": p["cand_idx"], "cand_avg": p["cand_avg"], "psd": p["psd"]}
        _scans_equal(got_items[k], want, (name, decim, k, "ss_process"))
        total += int(p["cand_off"][-1])
    assert total > 0  # the band's signals are found: the lists compared are not empty
    f_items.close()
    f_plain.close()


def test_an_items_feed_at_decim_one_is_an_ordinary_feed():
    iq = _items("cf32", 1)
    t, edges = _clock(len(iq)), _edges()
    e_items, e_plain = _engine("cf32", 1), _engine("cf32", 1)
    f_items = e_items.feed(depth=2, cand_cap=1 << 16, want_psd=True, items=True)
    f_plain = e_plain.feed(depth=2, cand_cap=1 << 16, want_psd=True)
    assert f_items.acquire().shape == (MAX_BATCH, N)

    def fill(buf, a, b):
        buf[:b - a] = iq[a:b]

    for k, (x, y) in enumerate(zip(_scan(f_items, fill, edges, t), _scan(f_plain, fill, edges, t))):
        _scans_equal(x, y, k)
    # and it records from the device upload, as an ordinary feed does: nothing is uploaded a second time
    rec = f_items.record(BW, channels=2)
    ref = Channelizer(FS, BW, channels=2, max_samples=MAX_BATCH * N)
    buf = f_items.acquire()
    buf[:40] = iq[:40]
    f_items.submit(40, t_ms=t[:40])
    f_items.collect()
    ranges = [(1, 50_000, 3, 40 * N - 1), (0, -100_000, 100, 5_000)]
    _same(rec.record(ranges), ref.process_ranges(iq[:40].reshape(-1), ranges, want_cf32=False), "decim 1")
    assert rec.last_h2d_bytes == 0
    rec.close()
    f_items.close()
    f_plain.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. and 3. record equals the whole-stream route, and uploads only the union of the ranges
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracked", [False, True], ids=["ss_feed_collect", "stf_collect"])
@pytest.mark.parametrize("name", ["cf32", "cs8"])
def test_record_equals_process_ranges_on_the_item_stream(name, tracked):
    iq = _items(name, D5)
    bps = A.SS_FMT_BYTES[FORMATS[name][0]]
    eng = _engine(name, D5, flags=KEEP if tracked else 0)
    feed = eng.feed(depth=3, cand_cap=1 << 16, items=True)
    trk = feed.track(128) if tracked else None
    rec = feed.record(BW, channels=4, want_cf32=True)
    ref = Channelizer(FS, BW, in_format=FORMATS[name][0], channels=4, max_samples=MAX_BATCH * ITEM)
    edges, t = _edges(), _clock(len(iq))
    recorded, uploaded = 0, 0
    for k, (lo, hi) in enumerate(edges):  # one batch ahead of the collect: the held slot and the one being filled differ
        for j in ([0, 1] if k == 0 else [k + 1] if k + 1 < len(edges) else []):
            a, b = edges[j]
            buf = feed.acquire()
            buf[:b - a] = iq[a:b]
            feed.submit(b - a, t_ms=t[a:b], tag=j)
        got = trk.collect() if tracked else feed.collect()
        assert got["nframes"] == hi - lo and got["tag"] == k
        ranges = _cut(lo, hi)
        assert ranges, k  # (every batch of this stream records something)
        out = rec.record(ranges)
        _same(out, ref.process_ranges(_flat(iq[lo:hi]), ranges), (name, k))
        assert rec.last_h2d_bytes == bps * _union(ranges), (name, k, rec.last_h2d_bytes, _union(ranges))
        uploaded += rec.last_h2d_bytes
        recorded += int(sum(out[1]))
    assert {len(_cut(lo, hi)) for lo, hi in edges} >= {2, 3, 4}
    assert uploaded == bps * _union(GLOBAL) < bps * len(iq) * ITEM // 2  # (the third batch is covered whole, the stream by far not)
    assert recorded > (900 + 9_700 + 10_000 + 50_000 + 1 + 14_000) * BW // FS - 12 and feed.pending == 0
    rec.close()
    if trk:
        trk.close()
    feed.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. what an earlier record left in the channeliser's input buffer is never read
# ---------------------------------------------------------------------------------------------------------------------------
def test_stale_staging_is_never_read():
    iq = _items("cf32", D5)
    eng = _engine("cf32", D5)
    feed = eng.feed(depth=2, cand_cap=1 << 16, items=True)
    rec = feed.record(BW, channels=3, want_cf32=True)
    ref = Channelizer(FS, BW, channels=3, max_samples=MAX_BATCH * ITEM)
    n = 40 * ITEM
    scattered = [(0, 100_000, 1, 2), (1, -250_000, 5 * ITEM + 255, 5 * ITEM + 258), (0, 100_000, 7 * ITEM + 600, 9 * ITEM + 3),
                 (2, 30_000, 9 * ITEM, 9 * ITEM + 4_001), (1, 7_000, 30 * ITEM + 1_279, n), (0, 100_000, n - 1, n)]
    plans = [[(0, 100_000, 0, n)], scattered, [(1, 7_000, 0, n)], scattered]
    for k, ranges in enumerate(plans):
        a = 40 * (k % 3)  # the batches differ: what the batch before left between the ranges is another stream's samples
        buf = feed.acquire()
        buf[:40] = iq[a:a + 40]
        feed.submit(40, tag=k)
        assert feed.collect()["tag"] == k
        _same(rec.record(ranges), ref.process_ranges(iq[a:a + 40].reshape(-1), ranges), k)
        assert rec.last_h2d_bytes == 8 * _union(ranges)
    rec.close()
    feed.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. sc_process_ranges_upload alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FORMATS))
def test_ranges_upload_equals_ranges_device_on_the_whole_stream(name):
    torch = pytest.importorskip("torch")
    iq = _flat(_items(name, D5, 24))
    n, nch = 24 * ITEM, 4
    bps = A.SS_FMT_BYTES[FORMATS[name][0]]
    a = Channelizer(FS, BW, in_format=FORMATS[name][0], channels=nch, max_samples=n)
    b = Channelizer(FS, BW, in_format=FORMATS[name][0], channels=nch, max_samples=n)
    cap = a.output_capacity(n)
    host = iq.view(np.float32).reshape(-1, 2) if iq.dtype == np.complex64 else iq
    d_iq = torch.from_numpy(np.array(host)).to("cuda:0")  # (a copy: the shared stream is read-only)
    calls = [
        [(1, 100_000, 0, n)],
        [(1, 100_000, 300, 1_200), (2, -250_000, 77, 3 * ITEM + 900), (3, 30_000, 4_000, 9_000), (3, -40_000, 9_000, 20_001), (1, 7_000, 25_001, 25_002),
         (2, -250_000, 30_000, n)],
        [],
        [(0, 50_000, n - 1, n), (2, 1_000, 5, 5), (1, 7_000, 11, 12)],
    ]
    for k, ranges in enumerate(calls):
        planes = []
        for _ in range(2):
            planes.append((torch.zeros((nch, cap, 2), dtype=torch.int8, device="cuda:0"), torch.zeros((nch, cap, 2), dtype=torch.float32, device="cuda:0")))
        torch.cuda.synchronize()
        ca, rca, up = a.process_ranges_upload(iq, ranges, planes[0][0], planes[0][1], cap)
        cb, rcb = b.process_ranges_device(d_iq, n, ranges, planes[1][0], planes[1][1], cap)
        b.sync()
        assert list(ca) == list(cb) and list(rca) == list(rcb), (name, k)
        assert up == bps * _union(ranges), (name, k, up)
        for p in range(2):  # the whole planes: nothing is written beyond a channel's count either
            assert planes[0][p].cpu().numpy().tobytes() == planes[1][p].cpu().numpy().tobytes(), (name, k, p)
        if ranges and k != 3:
            assert int(ca.sum()) > 0
    with pytest.raises(SpecscanError) as e:  # refused before anything is copied
        a.process_ranges_upload(iq, [(0, 0, 0, n + 1)], None, None, cap)
    assert e.value.status == INVALID
    a.start(1, 77_000)
    with pytest.raises(SpecscanError) as e:
        a.process_ranges_upload(iq, [(0, 0, 0, n)], None, None, cap)
    assert e.value.status == INVALID and a.is_recording(1)
    a.stop(1)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the hold, and a producer thread
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_hold_and_progress_at_depth_two():
    iq = _items("cf32", D5)
    eng = _engine("cf32", D5)
    feed = eng.feed(depth=2, cand_cap=1 << 16, items=True)
    rec = feed.record(BW, channels=2)
    ref = Channelizer(FS, BW, channels=2, max_samples=MAX_BATCH * ITEM)

    def submit(j):
        buf = feed.acquire()
        buf[:24] = iq[24 * j:24 * j + 24]
        feed.submit(24, tag=j)

    submit(0)
    submit(1)
    for k in range(6):
        assert feed.collect()["tag"] == k
        if k < 5:  # slot k % 2 is held and it is the next to hand out
            with pytest.raises(SpecscanError) as e:
                feed.acquire()
            assert e.value.status == INVALID and "no free feed slot" in str(e.value)
        with pytest.raises(SpecscanError) as e:
            feed.collect()
        assert e.value.status == INVALID and "held" in str(e.value)
        ranges = [(1, 50_000, 3, 24 * ITEM - k), (0, -100_000, 100 * k + 300, 5_000)]
        if k == 4:
            rec.release()  # unrecorded: nothing is uploaded
        elif k == 5:
            rec.last_h2d_bytes = -1
            out = rec.record([])  # no ranges: a release
            assert out[0] == {} and len(out[1]) == 0 and rec.last_h2d_bytes == 0
        else:
            _same(rec.record(ranges), ref.process_ranges(iq[24 * k:24 * k + 24].reshape(-1), ranges, want_cf32=False), k)
            assert rec.last_h2d_bytes == 8 * _union(ranges)
        with pytest.raises(SpecscanError):
            rec.release()  # let go already
        if k + 2 < 6:
            submit(k + 2)  # progress: the slot just let go is free again
    assert feed.pending == 0
    rec.close()
    feed.close()
    ref.close()


def test_producer_and_consumer_threads():
    name = "cs8"
    iq = _items(name, D5)
    eng = _engine(name, D5)
    depth = 3
    feed = eng.feed(depth=depth, cand_cap=1 << 16, items=True)
    rec = feed.record(BW, channels=4, want_cf32=True)
    ref = Channelizer(FS, BW, in_format=FORMATS[name][0], channels=4, max_samples=MAX_BATCH * ITEM)
    edges = _edges() * 3  # twelve batches, the stream three times over
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
            results.append((j, ranges, rec.record(ranges), rec.last_h2d_bytes))
            free.release()
    finally:
        for _ in edges:  # (a failure above must not leave the producer waiting for a slot)
            free.release()
    th.join()
    assert not errors, errors
    assert len(results) == len(edges)
    for j, ranges, out, up in results:  # the reference afterwards, in the same order: the recording never waited for it
        lo, hi = edges[j]
        _same(out, ref.process_ranges(_flat(iq[lo:hi]), ranges), j)
        assert up == 2 * _union(ranges)
    rec.close()
    feed.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    iq = _items("cf32", 2)
    dec = _engine("cf32", 2)
    plain = dec.feed(depth=2, cand_cap=1 << 10)
    with pytest.raises(SpecscanError) as e:
        plain.record(BW)
    assert e.value.status == INVALID and "decim" in str(e.value) and "ss_feed_create_items" in str(e.value)
    plain.close()
    feed = dec.feed(depth=2, cand_cap=1 << 10, items=True)
    feed.acquire()
    with pytest.raises(SpecscanError) as e:
        feed.record(BW)  # a slot is being filled
    assert e.value.status == INVALID and "pending" in str(e.value)
    feed.acquire()[:4] = iq[:4]
    feed.submit(4)
    with pytest.raises(SpecscanError) as e:
        feed.record(BW)
    assert e.value.status == INVALID and "pending" in str(e.value)
    feed.collect()
    rec = feed.record(BW, channels=2)
    with pytest.raises(SpecscanError) as e:
        feed.record(BW)
    assert e.value.status == INVALID and "already has a recorder" in str(e.value)
    ref = Channelizer(FS, BW, channels=2, max_samples=MAX_BATCH * N * 2)
    feed.acquire()[:7] = iq[4:11]
    feed.submit(7)
    feed.collect()
    n = 7 * N * 2
    rec.last_h2d_bytes = -1
    with pytest.raises(SpecscanError) as e:  # one sample beyond the batch's items: refused, held, nothing uploaded
        rec.record([(0, 100_000, 0, 100), (1, 0, n - 5, n + 1)])
    assert e.value.status == INVALID and "nsamples" in str(e.value) and rec.last_h2d_bytes == -1
    with pytest.raises(SpecscanError) as e:
        feed.collect()
    assert "held" in str(e.value)
    ranges = [(0, 100_000, 0, 100), (1, 0, n - 5, n)]  # the refused call changed nothing: the same state as the reference's
    _same(rec.record(ranges), ref.process_ranges(iq[4:11].reshape(-1), ranges, want_cf32=False), "after a refusal")
    assert rec.last_h2d_bytes == 8 * 105
    rec.close()
    feed.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. end to end at decim 5
# ---------------------------------------------------------------------------------------------------------------------------
def test_track_plan_record_end_to_end_at_decim_five():
    """test_gpu_record_feed.py's end-to-end run on an items feed: the tracker's frames are items, RangePlanner(channels, N * 5) turns
    them into ranges of the item stream, and srf_record must equal per range sc_start / sc_process / sc_stop on that stream."""
    nframes, g = 150, 128
    iq = pkg.synth.SyntheticBand(N, seed=5, on_frame=30 * D5, off_frame=110 * D5).frames_cf32(nframes * D5).reshape(nframes, ITEM)
    t = _clock(nframes)
    eng = pkg.SpectrumEngine(FS, CENTER, fft_size=N, decim=D5, max_batch=MAX_BATCH, learn_ms=280, flags=KEEP)
    feed = eng.feed(depth=3, cand_cap=1 << 20, items=True)
    trk = feed.track(g, max_watch=4096)
    rec = feed.record(BW, channels=2)
    tracker = pkg.tracker.SignalTracker(N, FS, group_size=g, min_time_ms=200, timeout_ms=400)
    planner = RangePlanner(2, ITEM)
    classic = Channelizer(FS, BW, channels=2, max_samples=MAX_BATCH * ITEM)
    cuts, at = [], 0
    for size in (7, 64, 1, 30) * 3:
        if at < nframes:
            cuts.append((at, min(nframes, at + size)))
            at = cuts[-1][1]

    def gather(store, records, ranges, ends, flushed, outs):
        for (ch, shift, _b, _e), why, fl, y in zip(ranges, ends, flushed, outs):
            store[ch].append(y)
            if fl:
                records.append((ch, CENTER + shift, np.concatenate(store[ch]).tobytes()))
            if fl or why == "stop":
                store[ch] = []

    rec_a, rec_b, store_a, store_b = [], [], {0: [], 1: []}, {0: [], 1: []}
    kinds, nranges, uploaded, streamed = set(), 0, 0, 0
    for lo, hi in cuts:
        buf = feed.acquire()
        buf[:hi - lo] = iq[lo:hi]
        feed.submit(hi - lo, t_ms=t[lo:hi])
        got = trk.collect()
        tx = tracker.process_batch_digest(t[lo:hi], got)
        trk.post_keys(got["seq"], tracker.keys)
        ranges, ends, flushed = planner.plan([[(int(s), bool(f)) for s, f in frame[0]] for frame in tx])
        assert all(b % ITEM == 0 and e % ITEM == 0 for _c, _s, b, e in ranges)  # whole items: the tails between the frames too
        kinds |= set(ends)
        nranges += len(ranges)
        out, rc = rec.record(ranges)  # (no ranges: a release)
        assert rec.last_h2d_bytes == 8 * _union(ranges)
        uploaded += rec.last_h2d_bytes
        streamed += 8 * (hi - lo) * ITEM
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
    print(f"end to end at decim {D5}: {nranges} ranges, ends {sorted(kinds)}, {len(rec_a)} records, "
          f"{sum(len(r[2]) for r in rec_a) // 2} samples published, {uploaded} of {streamed} bytes uploaded for recording")
    assert nranges > 0 and kinds == {"stop", "batch"} and len(rec_a) > 0
    assert [(r[0], r[1], len(r[2])) for r in rec_a] == [(r[0], r[1], len(r[2])) for r in rec_b]
    assert rec_a == rec_b
    assert sum(len(r[2]) for r in rec_a) > 0 and 0 < uploaded < streamed
    rec.close()
    trk.close()
    feed.close()
    classic.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the other riders of the feed
# ---------------------------------------------------------------------------------------------------------------------------
def test_spectrogram_rows_are_an_ordinary_feeds():
    iq = _items("cs8", D5)
    t = _clock(64)  # 2.5 s of clock in one batch: the per-frame gate closes rows inside it
    snaps = []
    for items in (True, False):
        eng = _engine("cs8", D5, flags=SPEC)
        feed = eng.feed(depth=2, cand_cap=1 << 16, items=items)
        sg = feed.spectrogram(max_rows=8, want_mean=True)
        buf = feed.acquire()
        buf[:64] = iq[:64] if items else iq[:64, :N]
        feed.submit(64, t_ms=t)
        feed.collect()
        r = sg.rows()
        snaps.append({k: (np.array(v).tobytes() if isinstance(v, np.ndarray) else v) for k, v in r.items() if k != "payloads"} | {"payloads": r["payloads"]()})
        sg.close()
        feed.close()
    assert snaps[0]["nrows"] >= 1 and snaps[0] == snaps[1]


# ---------------------------------------------------------------------------------------------------------------------------
# replay_file(items=True): the dump's whole items through an items feed
# ---------------------------------------------------------------------------------------------------------------------------
def test_replay_file_with_items_gives_the_same_candidates_and_rows(tmp_path):
    import time
    from rtl_sdr_scanner_cpp_amd import replay
    iq = _items("cs8", D5)  # 144 items of 1280 samples: the dump is the continuous stream
    name = replay.make_raw_file_name("full", "cs8", CENTER, FS, time.struct_time((2025, 3, 7, 9, 5, 1, 0, 0, -1)))
    path = str(tmp_path / name[2:])
    sink = replay.RawFileSink(2)
    sink.start_recording(path)
    sink.work(iq)
    sink.close()
    info = replay.parse_raw_file_name(path)
    runs = []
    for items in (False, True):
        eng = pkg.SpectrumEngine(FS, CENTER, fft_size=N, decim=D5, max_batch=MAX_BATCH, learn_ms=280, flags=SPEC, **replay.engine_overrides_for(info))
        chunks, stats = [], replay.ReplayStats()
        got = list(replay.replay_file(eng, path, batch=40, frame_period_ms=40.0, spectrogram=chunks.append, items=items, stats=stats))
        eng.close()
        assert stats.bytes_read == len(iq) * N * 2 * (D5 if items else 1)
        runs.append(([(r["nframes"], r["first_frame"], r["status"], r["cand_off"].tobytes(), r["cand_idx"].tobytes(), r["cand_avg"].tobytes()) for r in got],
                     b"".join(chunks)))
    assert [r[0] for r in runs[0][0]] == [40, 40, 40, 24] and sum(len(r[4]) for r in runs[0][0]) > 0 and len(runs[0][1]) > 0
    assert runs[0] == runs[1]
