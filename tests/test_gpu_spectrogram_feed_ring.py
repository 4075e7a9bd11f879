"""Spectrogram rows from batches that keep no dB plane (include/specscan_spectrogram_feed_ring.h: sgf_create_ring), on the GPU.

Tested: an engine WITHOUT SS_FLAG_SPECTROGRAM, feed.spectrogram(ring=True). The stream and the cuts are the ring tracker's smallest
(tests/test_gpu_track_feed_ring.py); the clock is 1000 + 40 f ms with learn_ms = 240 — the frame that finds
the time up still learns, and that is frame 6 — so the first 7-frame batch is exactly the learning phase (it keeps its plane), a row closes at frames 26, 52, 78 — inside batches — and the first row spans the plane batch,
a ring batch and the head of the next.

Two oracles. BYTES: a lock-step feed (one batch in flight) reads batch_db_rows() behind every collect; the reference's own Spectrogram +
DataController (oracle/_ref, RefSpectrogram) is fed those rows frame by frame with the frame's clock, and its payloads must equal the
feed's byte for byte — no tolerance, no mask. VALUES: so that reader and kernel cannot agree on a wrong permutation, the rows read
must pass parity.check_plane("psd", ...) against the CPU oracle's PSD of the same frames. Needs an MI355X: run with -m gpu."""
import json
import struct
import subprocess
import time

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import replay
from parity import check_plane, floor_tolerance
from test_gpu_track_feed import _batches
from test_gpu_track_digest_sparse import Runner, _stream, _tile_counters
from test_gpu_track_feed_ring import _restricted

pytestmark = pytest.mark.gpu

SPEC = pkg.abi.SS_FLAG_SPECTROGRAM
CF32, CS8 = pkg.abi.SS_FMT_CF32, pkg.abi.SS_FMT_CS8
CENTER = 145_000_000
INVALID = pkg.abi.SS_ERR_INVALID
G = 128
FIELDS = ("time_ms", "frame", "count", "rows", "mean")


def _engine(n, fs, fmt, max_batch, **cfg):
    return pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=max_batch, learn_ms=240, learn_frames=7, in_format=fmt, **cfg)


def _retune(eng, n, fs):
    eng.set_frequency_range(CENTER + fs - fs // 2, CENTER + fs + fs // 2)


def _run(n, fs, fmt, iq, t, sizes, in_flight=1, tracker=False, ring=True, flags=0, read_db=False, reset_after=None, before_batch=None, max_batch=None, **cfg):
    """The stream through a feed with the spectrogram object bound, `in_flight` batches in flight (depth 3). Per batch: the rows as
    copies, whether ss_read_window(SS_PLANE_PSD) was refused right behind the submit (the batch kept no plane), and — read_db, one
    batch in flight — batch_db_rows() behind the collect. reset_after: behind that batch drain, retune, ss_reset (and stf_reset).
    before_batch(k, eng, drain): in front of batch k; drain() collects what is in flight. Returns (batches, the scan's tile counters)."""
    eng = _engine(n, fs, fmt, max_batch or max(sizes), flags=flags, **cfg)
    feed = eng.feed(depth=3, cand_cap=1 << 20)
    trk = feed.track(G, max_watch=4096, sparse=True, ring=True) if tracker else None
    sg = feed.spectrogram(max_rows=8, want_mean=True, ring=ring)
    cuts, out, waiting = _batches(len(t), sizes), [], []

    def collect_one():
        k = waiting.pop(0)
        got = trk.collect() if trk else feed.collect()
        assert got["nframes"] == cuts[k][1] - cuts[k][0] and got["status"] == 0
        if trk:
            assert got["digest_status"] == 0
            trk.post_keys(got["seq"], np.zeros(0, np.int32))
        r = sg.rows()
        b = {f: np.array(r[f]) for f in FIELDS}
        b.update(nrows=r["nrows"], size=r["size"], frequency=r["frequency"], sample_rate=r["sample_rate"], open_count=r["open_count"], payloads=r["payloads"]())
        if read_db:
            b["db"] = sg.batch_db_rows()
        out.append(b)

    def drain():
        while waiting:
            collect_one()

    no_plane = []
    for k, (lo, hi) in enumerate(cuts):
        if before_batch:
            before_batch(k, eng, drain)
        buf = feed.acquire()
        buf[:hi - lo] = iq[lo:hi]
        feed.submit(hi - lo, t_ms=t[lo:hi], tag=k)
        try:  # (ss_read_window speaks of the batch submitted last, in flight or not)
            eng.read_window(pkg.abi.SS_PLANE_PSD, 0, 0, 64)
            no_plane.append(False)
        except pkg.abi.SpecscanError as e:
            assert e.status == INVALID and "kept no dB" in str(e), str(e)
            no_plane.append(True)
        waiting.append(k)
        if len(waiting) == in_flight:
            collect_one()
        if reset_after is not None and k == reset_after:
            while waiting:
                collect_one()
            _retune(eng, n, fs)
            if read_db:  # the retune settled the ring's dB rows: they are no longer what the batch's rows were formed from
                with pytest.raises(pkg.abi.SpecscanError) as e:
                    sg.batch_db_rows(0, 1)
                assert e.value.status == INVALID
            eng.reset()
            if trk:
                trk.reset()
    while waiting:
        collect_one()
    for b, flag in zip(out, no_plane):
        b["no_plane"] = flag
    tiles = _tile_counters(eng)
    for obj in (sg, trk, feed, eng):
        if obj:
            obj.close()
    return out, tiles


def _bare_tile_counters(n, fs, fmt, iq, t, sizes, reset_after=None, before_batch=None, **cfg):
    """The same cuts as device calls on an engine with nothing bound."""
    eng = _engine(n, fs, fmt, max(sizes), **cfg)
    run = Runner(eng, True, 8192)
    for k, (lo, hi) in enumerate(_batches(len(t), sizes)):
        if before_batch:
            before_batch(k, eng, lambda: None)
        run.batch(iq[lo:hi], t[lo:hi])
        if reset_after is not None and k == reset_after:
            _retune(eng, n, fs)
            eng.reset()
    tiles = _tile_counters(eng)
    eng.close()
    return tiles


def _reference_payloads(ref_mod, n, fs, batches, t, cuts, centres=None):
    """RefSpectrogram over the rows read, frame by frame with ref_set_time(t[f]): per batch, the payloads it published."""
    ref = ref_mod.RefSpectrogram(n, fs, CENTER if centres is None else centres[0])
    out = []
    for k, (a, b) in enumerate(cuts):
        if centres is not None and (k == 0 or centres[k] != centres[k - 1]):
            ref_mod.ref().ref_set_time(int(t[a]))  # (the shim creates a new centre's container at the retune: on the first frame's clock)
            ref.set_frequency(centres[k])
        got = []
        for f in range(a, b):
            ref.work(batches[k]["db"][f - a:f - a + 1], int(t[f]))
            while True:
                p = ref.pop()
                if p is None:
                    break
                got.append(p)
        out.append(got)
    size = ref.size
    ref.close()
    return out, size


def _check_bytes(ref_mod, n, fs, batches, t, cuts, centres=None):
    want, size = _reference_payloads(ref_mod, n, fs, batches, t, cuts, centres)
    total = 0
    for k, (b, w) in enumerate(zip(batches, want)):
        assert b["size"] == size and b["sample_rate"] == fs
        assert b["nrows"] == len(w) == len(b["payloads"]), (k, b["nrows"], len(w))
        for i, (gp, wp) in enumerate(zip(b["payloads"], w)):
            assert struct.unpack_from("<QiiiI", gp) == struct.unpack_from("<QiiiI", wp), (k, i)
            assert gp == wp, (k, i, int(np.count_nonzero(np.frombuffer(gp, np.int8) != np.frombuffer(wp, np.int8))))
            assert struct.unpack_from("<Q", gp)[0] == int(b["time_ms"][i]) == int(t[cuts[k][0] + int(b["frame"][i])])
        total += len(w)
    return total


def _same_rows(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x["nrows"], x["open_count"], x["frequency"], x["size"]) == (y["nrows"], y["open_count"], y["frequency"], y["size"]), (what, k)
        assert x["payloads"] == y["payloads"], (what, k)
        for f in FIELDS:
            assert x[f].shape == y[f].shape and x[f].tobytes() == y[f].tobytes(), (what, k, f)


def _no_plane_as_expected(batches, cuts, no_plane, learning):
    for b, (lo, hi), learns in zip(batches, cuts, learning):
        assert not (learns and b["no_plane"]) and not (not learns and hi - lo in no_plane and not b["no_plane"]), ([x["no_plane"] for x in batches], cuts, learning)


_lock = {}


def _lockstep(n, fs, fmt, sizes, restricted=False):
    """The lock-step run of a form case: (iq, t, cfg, batches, tile counters). The one two tests share is kept."""
    key = (n, fs, fmt, sizes, restricted)
    if key in _lock:
        return _lock[key]
    band, cfg = _restricted(n) if restricted else ({}, {})
    iq, t = _stream(n, fmt, sum(sizes), **band)
    batches, tiles = _run(n, fs, fmt, iq, t, sizes, read_db=True, **cfg)
    if key == (65536, 65536 * 250, CS8, (7, 16, 40, 9, 16), False):
        _lock[key] = (iq, t, cfg, batches, tiles)
    return iq, t, cfg, batches, tiles


def _form_case(ref_mod, n, fmt, sizes, no_plane, fs=None, m=None, restricted=False):
    fs = fs or n * 250
    iq, t, cfg, batches, tiles = _lockstep(n, fs, fmt, sizes, restricted)
    cuts = _batches(len(t), sizes)
    assert all(b["size"] == n // m for b in batches), (batches[0]["size"], n // m)
    _no_plane_as_expected(batches, cuts, no_plane, [k == 0 for k in range(len(cuts))])
    assert any(b["no_plane"] for b in batches)
    # bytes: the reference's own block on the rows read
    assert _check_bytes(ref_mod, n, fs, batches, t, cuts) == (len(t) - 1) // 26 >= 1
    assert batches[0]["nrows"] == 0 and not batches[0]["no_plane"] and batches[1]["no_plane"] and batches[2]["nrows"] >= 1  # the first row spans both kinds
    # values: the rows read are the PSD of those frames
    ref = ref_mod.oracle_chain(fs, CENTER, fft_size=n, decim=1, max_batch=len(t), learn_ms=240, learn_frames=7, in_format=fmt, **cfg).process(iq, t_ms=t, want=("psd",))
    got = np.concatenate([b["db"] for b in batches])
    worst = check_plane("psd", got, ref["psd"], floor_tolerance(ref["psd"]))
    # the scan is the one the same device calls run on a bare engine
    bare = _bare_tile_counters(n, fs, fmt, iq, t, sizes, **cfg)
    print(f"n {n} fs {fs} m {m}: rows {[b['nrows'] for b in batches]}, no plane {[b['no_plane'] for b in batches]}, worst |dB err| {worst:.2e}, scan {tiles}")
    assert tiles == bare, (tiles, bare)


@pytest.mark.parametrize("fs,m", [(65536 * 250, 4), (1_024_000, 64), (128_000, 512)])
def test_65536_cs8_the_radix_8_fold(ref_mod, fs, m):
    _form_case(ref_mod, 65536, CS8, (7, 16, 40, 9, 16), no_plane=(16, 40), fs=fs, m=m)


@pytest.mark.parametrize("fs,m", [(131072 * 250, 8), (128_000, 1024)])
def test_131072_cs8_the_radix_16_fold(ref_mod, fs, m):
    _form_case(ref_mod, 131072, CS8, (7, 16, 25), no_plane=(16, 25), fs=fs, m=m)


def test_65536_cf32_the_culled_chain(ref_mod):
    _form_case(ref_mod, 65536, CF32, (7, 16, 40, 9), no_plane=(16, 40), m=4)


def test_262144_cf32_range_restricted(ref_mod):
    _form_case(ref_mod, 262144, CF32, (7, 16, 25), no_plane=(16, 25), m=16, restricted=True)


def test_2_20_cf32_ring_only_range_restricted(ref_mod):
    _form_case(ref_mod, 1 << 20, CF32, (7, 16, 16, 9), no_plane=(16,), m=64, restricted=True)


def test_two_batches_in_flight_with_a_ring_tracker_beside():
    """Depth 3, two batches in flight, a ring tracker and the ring spectrogram on one feed: rows, means, times, frames and counts of
    every batch are the lock-step run's, byte for byte; and with no tracker too."""
    n, fs, sizes = 65536, 65536 * 250, (7, 16, 40, 9, 16)
    iq, t, cfg, lock, tiles = _lockstep(n, fs, CS8, sizes)
    both, tiles_both = _run(n, fs, CS8, iq, t, sizes, in_flight=2, tracker=True)
    _same_rows(both, lock, "tracker + spectrogram, two in flight")
    alone, tiles_alone = _run(n, fs, CS8, iq, t, sizes, in_flight=2)
    _same_rows(alone, lock, "spectrogram alone, two in flight")
    assert [b["no_plane"] for b in both] == [b["no_plane"] for b in alone] == [b["no_plane"] for b in lock] == [False, True, True, True, True]
    assert tiles_both == tiles_alone == tiles


def test_ring_wrap_with_two_batches_in_flight():
    """28 batches of 40 frames at 65536 points, CS8: the 1024-row ring's window reaches the buffer's end and is moved to the front
    while two rows kernels are still in the stream."""
    n, fs, nframes = 65536, 65536 * 250, 1120
    base, _ = _stream(n, CS8, 160, period=160)
    iq = np.concatenate([base] * 7)
    t = (1_000 + 40 * np.arange(nframes)).astype(np.int64)
    lock, tiles = _run(n, fs, CS8, iq, t, (40,))
    both, tiles_both = _run(n, fs, CS8, iq, t, (40,), in_flight=2, tracker=True)
    _same_rows(both, lock, "ring wrap")
    assert sum(b["nrows"] for b in lock) == (nframes - 1) // 26 and all(b["no_plane"] for b in both[1:]) and tiles == tiles_both


def test_retune_and_reset_behind_a_drain(ref_mod):
    """A retune and ss_reset in mid-run: a container per centre; the batch behind the retune learns (a plane batch), the next ones take
    the fold again; batch_db_rows is refused once the retune has settled the rows."""
    n, fs, sizes = 65536, 65536 * 250, (7, 16, 40, 9, 16)
    iq = pkg.synth.SyntheticBand(n, seed=5, on_frame=30, off_frame=70, period=80).frames_cs8(150)
    t = (1_000 + 40 * np.arange(150)).astype(np.int64)
    cuts = _batches(150, sizes)
    lock, tiles = _run(n, fs, CS8, iq, t, sizes, read_db=True, reset_after=3)
    centres = [CENTER if k <= 3 else CENTER + fs for k in range(len(cuts))]
    assert [b["frequency"] for b in lock] == centres
    assert _check_bytes(ref_mod, n, fs, lock, t, cuts, centres) >= 4
    learning = [k == 0 or k == 4 for k in range(len(cuts))]
    _no_plane_as_expected(lock, cuts, (16, 40), learning)
    both, tiles_both = _run(n, fs, CS8, iq, t, sizes, in_flight=2, tracker=True, reset_after=3)
    _same_rows(both, lock, "retune")
    assert tiles == tiles_both == _bare_tile_counters(n, fs, CS8, iq, t, sizes, reset_after=3)


def test_plane_and_no_plane_batches_alternate(ref_mod):
    """Cycles of 28 frames: ss_reset_noise, a 12-frame batch (seven learning frames: it keeps its plane), a 16-frame batch that keeps
    none. Rows span both kinds both ways. Lock-step against the reference's bytes; then with two batches in flight and a ring tracker
    beside — the plane batch's rows kernel (on the plane) and the ring batch's (on the ring's buffer) in the stream together, drained
    only where ss_reset_noise waits for the stream anyway — against the lock-step run, byte for byte."""
    n, fs, cycles = 65536, 65536 * 250, 4
    iq = pkg.synth.SyntheticBand(n, seed=5, on_frame=8, off_frame=28, period=28).frames_cs8(28 * cycles)
    t = (1_000 + 40 * np.arange(28 * cycles)).astype(np.int64)

    def before_batch(k, eng, drain):
        if k and k % 2 == 0:
            drain()
            eng.sync()
            eng.reset_noise()
    batches, tiles = _run(n, fs, CS8, iq, t, (12, 16), read_db=True, before_batch=before_batch, max_batch=16)
    assert [b["no_plane"] for b in batches] == [False, True] * cycles
    assert _check_bytes(ref_mod, n, fs, batches, t, _batches(len(t), (12, 16))) == 4
    assert tiles == _bare_tile_counters(n, fs, CS8, iq, t, (12, 16), before_batch=before_batch)
    both, tiles_both = _run(n, fs, CS8, iq, t, (12, 16), in_flight=2, tracker=True, before_batch=before_batch, max_batch=16)
    _same_rows(both, batches, "alternating, two in flight")
    assert [b["no_plane"] for b in both] == [False, True] * cycles and tiles_both == tiles


@pytest.mark.parametrize("n", [8192, 16384])
def test_small_sizes_equal_the_flagged_object(n):
    """Below 65536 points every batch keeps its plane: ring=True on a flag-less engine gives the bytes sgf_create gives on a flagged one."""
    fs, sizes = n * 250, (7, 64, 1, 100)
    iq, t = _stream(n, CF32, sum(sizes))
    ring, _ = _run(n, fs, CF32, iq, t, sizes, in_flight=2)
    flagged, _ = _run(n, fs, CF32, iq, t, sizes, in_flight=2, ring=False, flags=SPEC)
    _same_rows(ring, flagged, n)
    assert sum(b["nrows"] for b in ring) == (sum(sizes) - 1) // 26 and not any(b["no_plane"] for b in ring)


def test_refusals():
    def refused(call, word):
        with pytest.raises(pkg.abi.SpecscanError) as e:
            call()
        assert e.value.status == INVALID and word in str(e.value), str(e.value)
    n, fs = 65536, 65536 * 250
    flagged = _engine(n, fs, CS8, 16, flags=SPEC)
    ff = flagged.feed(depth=2, cand_cap=1 << 12)
    refused(lambda: ff.spectrogram(ring=True), "sgf_create")
    ff.close()
    flagged.close()
    eng = _engine(n, fs, CS8, 16)
    feed = eng.feed(depth=3, cand_cap=1 << 16)
    refused(lambda: feed.spectrogram(max_rows=0, ring=True), "max_rows")
    buf = feed.acquire()
    refused(lambda: feed.spectrogram(ring=True), "pending")  # a slot is acquired
    buf[:7] = 0
    buf[:7, ::97] = 5
    feed.submit(7)
    refused(lambda: feed.spectrogram(ring=True), "pending")  # a batch is pending
    feed.collect()
    sg = feed.spectrogram(ring=True)
    refused(lambda: feed.spectrogram(ring=True), "already")
    refused(lambda: feed.spectrogram(), "SS_FLAG_SPECTROGRAM")  # (sgf_create on a flag-less context: what it always said)
    refused(lambda: sg.batch_db_rows(0, 8), "outside")
    assert sg.batch_db_rows(0, 7).shape == (7, n)
    sg.close()
    feed.close()
    eng.close()


def test_replay_tool_spectrogram_ring(tmp_path):
    """specscan_replay --track-ring --spectrogram-out F --spectrogram-ring on the 65536-point CS8 dump of test_replay_tool_track_ring,
    made long enough for the rows: the Python route's payload bytes, and "spectrogram_ring": true. The rows close on the stream's
    own clock, 4 ms a frame, and with a clock the scan learns for its 2000 ms: 528 frames put a row at frame 251 (1004 ms), the end of
    learning at frame 500 and a second row at frame 502, so that row spans plane batches and fold batches."""
    n = 65536
    fs, nframes, batch, learn = n * 250, 528, 16, 7
    iq = pkg.synth.SyntheticBand(n, seed=21, on_frame=30, off_frame=120).frames_cs8(nframes)
    path = tmp_path / replay.make_raw_file_name("full", "cs8", CENTER, fs, time.struct_time((2025, 3, 7, 9, 5, 1, 0, 0, -1)))[2:]
    sink = replay.RawFileSink(2)
    sink.start_recording(str(path))
    sink.work(iq)
    sink.close()
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=batch, learn_frames=learn, **replay.engine_overrides_for(replay.parse_raw_file_name(str(path))))
    chunks = []
    got = list(replay.replay_file(eng, str(path), batch=batch, track="ring", track_group_size=128, spectrogram=chunks.append, spectrogram_ring=True))
    assert sum(b["nframes"] for b in got) == nframes
    with pytest.raises(pkg.abi.SpecscanError):  # the last batch kept no dB plane: the fold ran with the rows bound
        eng.read_window(pkg.abi.SS_PLANE_PSD, 0, 0, 64)
    eng.close()
    want = b"".join(chunks)
    assert len(chunks) == 2
    tool = pkg.build.build_replay_tool()
    out_file = tmp_path / "rows.bin"
    r = subprocess.run([tool, str(path), "--fft", str(n), "--decim", "1", "--batch", str(batch), "--learn-frames", str(learn), "--track-ring", "--bandwidth", "32000",
                        "--spectrogram-out", str(out_file), "--spectrogram-ring"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["spectrogram_ring"] is True and (rep["frames"], rep["spectrogram_rows"]) == (nframes, len(chunks)), rep
    assert out_file.read_bytes() == want
