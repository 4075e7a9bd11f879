"""specscan_replay --record-out on the GPU: the C++ host (host/replay_main.cpp: tracked feed -> SignalTracker -> FeedRecorder =
RangePlanner + srf_record + RecordingStore) records the transmissions of a raw dump, and its FILE must equal, byte for byte, what
the Python route gives on the same dump and the same cuts: SpectrumEngine with replay.engine_overrides_for, engine.feed(...).track
and .record, tracker.SignalTracker with the same min_time_ms / timeout_ms, recorder.RangePlanner, the store restatement of
tests/test_recording_store_host.py and channelizer.transmission_payload. The JSON counters are compared too. Run with -m gpu.

fs = 1 024 000, recording bandwidth 16 000: one item is 4096 outputs = 256 frames of 1 ms. Case 1: N = 1024, CF32, decim 1,
--track-sparse, batches of 64, two recorders for four combs. Case 2: the same band as .cs8 at N = 512, decim 2 — a whole-item feed —
--track, four recorders."""
import json
import struct
import subprocess
import time

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from rtl_sdr_scanner_cpp_amd import replay
from rtl_sdr_scanner_cpp_amd.channelizer import transmission_payload
from rtl_sdr_scanner_cpp_amd.recorder import RangePlanner
from test_recording_store_host import StoreModel

pytestmark = pytest.mark.gpu

FS, CENTER, BW, LEARN = 1_024_000, 145_000_000, 16_000, 25
KEEP = pkg.abi.SS_FLAG_KEEP_PLANES


def write_dump(tmp_path, iq, ext):
    name = replay.make_raw_file_name("full", ext, CENTER, FS, time.struct_time((2025, 3, 7, 9, 5, 1, 0, 0, -1)))
    path = str(tmp_path / name[2:])
    sink = replay.RawFileSink(8 if ext == "fc" else 2)
    sink.start_recording(path)
    sink.work(iq)
    sink.close()
    return path


def run_tool(path, out, n, decim, batch, extra):
    tool = pkg.build.build_replay_tool()
    r = subprocess.run([tool, path, "--fft", str(n), "--decim", str(decim), "--batch", str(batch), "--learn-frames", str(LEARN), "--bandwidth", str(BW),
                        "--record-out", str(out), *extra], capture_output=True, text=True, timeout=120)
    return r, (json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None)


def python_route(path, iq, n, decim, batch, recorders, min_time_ms, timeout_ms, sparse):
    """The dump's items through the tracked, recorded feed in the tool's cuts. Returns (FILE's bytes, counters, what the stream did)."""
    info = replay.parse_raw_file_name(path)
    items = decim != 1
    stride = n * decim
    g = pkg.tracker.index_step(BW, FS, n)
    eng = pkg.SpectrumEngine(FS, CENTER, fft_size=n, decim=decim, max_batch=batch, learn_frames=LEARN, flags=0 if sparse else KEEP,
                             **replay.engine_overrides_for(info))
    feed = eng.feed(depth=3, cand_cap=1 << 20, items=items)
    trk = feed.track(g, max_watch=4096, sparse=sparse)
    rec = feed.record(BW, channels=recorders)
    tracker = pkg.tracker.SignalTracker(n, FS, group_size=g, min_time_ms=min_time_ms, timeout_ms=timeout_ms)
    planner = RangePlanner(recorders, stride)
    frame_time = lambda frame: 1000 * frame * stride // FS  # noqa: E731  (the stream's own clock, as the tool's)
    store = StoreModel(recorders, CENTER, BW, stride, frame_time)
    c = {"recorded_ranges": 0, "recorded_samples": 0, "record_h2d_bytes": 0, "ignored_shifts_max": 0}
    did = {"stop": 0, "batch_from_zero": 0, "union_bytes": 0}
    bps = iq.itemsize * (1 if iq.dtype == np.complex64 else 2)
    for lo in range(0, len(iq), batch):
        hi = min(len(iq), lo + batch)
        buf = feed.acquire()
        buf[:hi - lo] = iq[lo:hi]  # (decim != 1: whole items into a whole-item feed)
        feed.submit(hi - lo)
        got = trk.collect()
        t = np.array([frame_time(f) for f in range(lo, hi)], np.int64)
        tx = tracker.process_batch_digest(t, got)
        trk.post_keys(got["seq"], tracker.keys)
        ranges, ends, flushes = planner.plan([[(int(s), bool(f)) for s, f in frame[0]] for frame in tx])
        c["ignored_shifts_max"] = max(c["ignored_shifts_max"], len(planner.ignored))
        if not ranges:
            rec.release()
            continue
        out, rc = rec.record(ranges)
        c["record_h2d_bytes"] += rec.last_h2d_bytes
        covered = np.zeros((hi - lo) * stride, bool)
        used = {}
        for r, why, fl, count in zip(ranges, ends, flushes, rc):
            ch, at = r[0], used.get(r[0], 0)
            store.feed(r, why, fl, out[ch][0][at:at + count], lo)
            used[ch] = at + int(count)
            covered[r[2]:r[3]] = True
            c["recorded_ranges"] += 1
            c["recorded_samples"] += r[3] - r[2]
            did["stop"] += why == "stop"
            did["batch_from_zero"] += why == "batch" and r[2] == 0
        did["union_bytes"] += bps * int(covered.sum())
    store.finish()
    c["published_items"], c["dropped_items"] = len(store.published), store.dropped
    data = b"".join(struct.pack("<I", len(p)) + p for p in (transmission_payload(t, f, rate, np.frombuffer(x, np.int8)) for t, f, rate, x in store.published))
    did.update(store.seen, stream_bytes=bps * len(iq) * stride)
    rec.close()
    trk.close()
    feed.close()
    eng.close()
    return data, c, did


def check_case(tmp_path, iq, ext, n, decim, batch, recorders, sparse, also):
    path = write_dump(tmp_path, iq, ext)
    want, counters, did = python_route(path, iq, n, decim, batch, recorders, 200, 300, sparse)
    print(counters, did)
    # what the stream must do, on the Python route alone
    assert counters["published_items"] >= 3 and did["stop"] >= 1 and did["batch_from_zero"] >= 1 and did["from_pending"] >= 1, (counters, did)
    assert also(counters, did), (counters, did)
    out = tmp_path / "tx.bin"
    r, rep = run_tool(path, out, n, decim, batch, ["--track-sparse" if sparse else "--track", "--recorders", str(recorders), "--min-time-ms", "200",
                                                   "--timeout-ms", "300"])
    assert r.returncode == 0, r.stderr
    print(rep)
    got = out.read_bytes()
    assert len(got) == len(want) == counters["published_items"] * (4 + 8 + 4 + 4 + 4 + 2 * 4096)
    assert got == want
    assert {k: rep[k] for k in counters} == counters
    assert rep["frames"] == rep["tracked_frames"] == len(iq) and rep["fft_size"] == n and rep["decim"] == decim


def test_case_1_cf32_sparse_two_recorders_for_four_combs(tmp_path):
    n, nframes = 1024, 1500
    iq = pkg.synth.SyntheticBand(n, seed=5, on_frame=30, off_frame=900).frames_cf32(nframes)
    # four combs, two slots: shifts are ignored; decim 1: recorded from the feed's own upload, nothing crosses PCIe twice
    check_case(tmp_path, iq, "fc", n, 1, 64, 2, True, lambda c, did: c["ignored_shifts_max"] >= 1 and c["record_h2d_bytes"] == 0)


def test_case_2_cs8_decim_2_whole_item_feed(tmp_path):
    n, decim, nframes = 512, 2, 1500
    iq = pkg.synth.SyntheticBand(n, decim=decim, seed=5, on_frame=30, off_frame=900).frames_cs8(nframes)
    # only the recorded union crosses PCIe a second time, and that is less than the stream
    check_case(tmp_path, iq, "cs8", n, decim, 64, 4, False, lambda c, did: 0 < c["record_h2d_bytes"] == did["union_bytes"] < did["stream_bytes"])


def test_usage_and_a_band_that_never_turns_on(tmp_path):
    n, nframes = 1024, 200
    iq = pkg.synth.SyntheticBand(n, seed=5, on_frame=10_000, off_frame=10_001).frames_cf32(nframes)
    path = write_dump(tmp_path, iq, "fc")
    out = tmp_path / "tx.bin"
    r, _ = run_tool(path, out, n, 1, 64, [])  # --record-out without --track / --track-sparse
    assert r.returncode == 2 and "usage" in r.stderr and not out.exists()
    r, rep = run_tool(path, out, n, 1, 64, ["--track-sparse", "--recorders", "2"])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == b""
    assert (rep["published_items"], rep["record_h2d_bytes"], rep["recorded_ranges"], rep["recorded_samples"], rep["dropped_items"]) == (0, 0, 0, 0, 0)
    assert rep["frames"] == nframes
