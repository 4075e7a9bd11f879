"""k_scan_step's stage pipelining (csrc/scan_step.h, 8192-point frames): the launch of call k carries the FFT + dB stage of
call k, the averaging / threshold stage of call k-1 and the candidate-list stage of call k-2. Results must be those of the
stages run back to back — bit for bit, whatever the call sizes, through learning, retunes, resets and reads in between.
Needs an MI355X: run with -m gpu."""
import os

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg

pytestmark = pytest.mark.gpu

N, FS, CENTER = 8192, 2_048_000, 145_000_000


def _device_outputs(torch, dev, s_, want_planes):
    """Result buffers pre-filled with values no result can have. torch fills them on its own stream: callers synchronise the
    device once after creating them, before an engine (which has its own streams) is asked to write there."""
    o = dict(psd=torch.full((s_, N), -7.0, dtype=torch.float32, device=dev), off=torch.full((s_ + 1,), -1, dtype=torch.int32, device=dev),
             idx=torch.full((s_ * 512,), -1, dtype=torch.int32, device=dev), cav=torch.full((s_ * 512,), -7.0, dtype=torch.float32, device=dev))
    o["rel"] = torch.full((s_, N), -7.0, dtype=torch.float32, device=dev) if want_planes else None
    o["avg"] = torch.full((s_, N), -7.0, dtype=torch.float32, device=dev) if want_planes else None
    return o


def _call(eng, d_iq, s_, o):
    eng.process_device(d_iq, s_, psd=o["psd"], rel=o["rel"], avg=o["avg"], cand_off=o["off"], cand_idx=o["idx"], cand_avg=o["cav"])


def _same(a, b, what):
    for k in ("psd", "off", "rel", "avg"):
        if a[k] is not None:
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=f"{what}: {k}")
    total = int(a["off"][-1])
    assert total == int(b["off"][-1])
    np.testing.assert_array_equal(a["idx"][:total].cpu().numpy(), b["idx"][:total].cpu().numpy(), err_msg=f"{what}: cand_idx")
    np.testing.assert_array_equal(a["cav"][:total].cpu().numpy(), b["cav"][:total].cpu().numpy(), err_msg=f"{what}: cand_avg")
    return total


@pytest.mark.parametrize("seed", range(8))
def test_overlapped_calls_equal_call_by_call(seed):
    """Engine A waits after every call (no stage ever overlaps another call), engine B is only synchronised at the very end
    (up to three calls in flight). Same stream, same random cut into calls, a retune with reset and a plain reset on the way,
    sometimes int8 IQ, the spectrogram branch or full planes."""
    import torch
    rng = np.random.default_rng(4200 + seed)
    dev = torch.device("cuda:0")
    fmt = [pkg.abi.SS_FMT_CF32, pkg.abi.SS_FMT_CS8, pkg.abi.SS_FMT_CU8][seed % 3]
    want_planes = seed % 4 == 1
    flags = pkg.abi.SS_FLAG_SPECTROGRAM if seed % 4 == 2 else 0
    nframes, learn, max_batch = 420, int(rng.integers(10, 40)), int(rng.choice([64, 100, 128]))
    band = pkg.synth.SyntheticBand(N, seed=70 + seed, on_frame=learn + 25, off_frame=250, period=300)
    iq = band.frames_cf32(nframes) if fmt == pkg.abi.SS_FMT_CF32 else (band.frames_cs8(nframes) if fmt == pkg.abi.SS_FMT_CS8 else band.frames_cu8(nframes))
    kw = dict(fft_size=N, decim=1, in_format=fmt, learn_frames=learn, max_batch=max_batch, flags=flags)
    a, b = pkg.SpectrumEngine(FS, CENTER, **kw), pkg.SpectrumEngine(FS, CENTER, **kw)
    sizes, pos = [], 0
    while pos < nframes:
        s_ = int(min(nframes - pos, rng.choice([1, 3, 16, 17, 40, max_batch, int(rng.integers(1, max_batch + 1))])))
        sizes.append(s_)
        pos += s_
    retune_at, reset_at = len(sizes) // 3, 2 * len(sizes) // 3
    outs_a = [_device_outputs(torch, dev, s_, want_planes) for s_ in sizes]
    outs_b = [_device_outputs(torch, dev, s_, want_planes) for s_ in sizes]
    torch.cuda.synchronize()  # (torch fills these on ITS stream: they must have landed before an engine writes on its own)
    keep, pos = [], 0
    for k, s_ in enumerate(sizes):
        if k == retune_at:  # SdrDevice::setFrequencyRange: new centre, buffers reset, noise learned afresh there
            for e in (a, b):
                e.set_frequency_range(CENTER + 1_000_000 - FS // 2, CENTER + 1_000_000 + FS // 2)
                e.reset()
        if k == reset_at:
            for e in (a, b):
                e.reset()
        chunk = iq[pos:pos + s_]
        d_iq = torch.from_numpy(np.ascontiguousarray(chunk).view(np.float32) if chunk.dtype == np.complex64 else np.ascontiguousarray(chunk)).to(dev)
        keep.append(d_iq)  # inputs stay untouched until the final sync
        _call(a, d_iq, s_, outs_a[k])
        a.sync()
        _call(b, d_iq, s_, outs_b[k])
        pos += s_
    b.sync()
    total = sum(_same(oa, ob, f"call {k} ({sizes[k]} frames)") for k, (oa, ob) in enumerate(zip(outs_a, outs_b)))
    assert total > 500
    if flags:
        ra, rb = a.spectrogram_read(), b.spectrogram_read()
        assert ra[2] == rb[2] > 0
        np.testing.assert_array_equal(ra[0], rb[0])
        np.testing.assert_array_equal(ra[1], rb[1])


@pytest.mark.parametrize("seed", range(int(os.environ.get("SS_TEST_DEEP_SEEDS", "6"))))
def test_long_runs_of_overlapped_calls_equal_call_by_call(seed):
    """Deep pipelining (specscan.hip): with calls of at least 35 frames and no learning in between, launch L carries FFT(L),
    detect(L - 2) and emit(L - 4) and launches alternate over two queues; five calls are in flight. Long runs of such calls —
    sizes that are and are not multiples of the 16-frame tiles, now and then a short call, a flush, a read or a producer on
    the public stream — against an engine that waits after every call. Plane sets rotate over `sets` buffers: fewer than
    five make the library drain instead of overlapping; the results are the same bits either way."""
    import torch
    rng = np.random.default_rng(9100 + seed)
    dev = torch.device("cuda:0")
    fmt = [pkg.abi.SS_FMT_CF32, pkg.abi.SS_FMT_CS8][seed % 2]
    want_planes = seed % 3 == 1
    sets = [8, 8, 5, 3, 2, 8, 6, 4, 7][seed % 9]
    flags = pkg.abi.SS_FLAG_SPECTROGRAM if seed % 4 == 3 else 0  # (the spectrogram branch rides in the detect stage: per-call partial sums, added at the next drain)
    decim = 3 if seed % 7 == 5 else 1  # (frame decimation: items of 3 x 8192 samples, the first 8192 scanned — also by the launch that transforms a call's last frames again)
    nframes, learn, max_batch = (1400 if decim == 1 else 700), 20, 128
    band = pkg.synth.SyntheticBand(N, decim=decim, seed=170 + seed, on_frame=60, off_frame=900 // decim, period=1000 // decim)
    iq = band.frames_cf32(nframes) if fmt == pkg.abi.SS_FMT_CF32 else band.frames_cs8(nframes)
    kw = dict(fft_size=N, decim=decim, in_format=fmt, learn_frames=learn, max_batch=max_batch, flags=flags)
    a, b = pkg.SpectrumEngine(FS, CENTER, **kw), pkg.SpectrumEngine(FS, CENTER, **kw)
    pub = torch.cuda.ExternalStream(b.stream_handle, device=dev)
    sizes, pos = [], 0
    while pos < nframes:
        s_ = int(min(nframes - pos, rng.choice([35, 37, 48, 64, 99, 128, int(rng.integers(35, 129)), int(rng.integers(35, 129)), int(rng.integers(1, 35))])))
        sizes.append(s_)
        pos += s_
    ring_b = [_device_outputs(torch, dev, max_batch, want_planes) for _ in range(sets)]
    outs_a = [_device_outputs(torch, dev, max_batch, want_planes) for _ in sizes]
    torch.cuda.synchronize()  # (torch fills these on ITS stream: they must have landed before an engine writes on its own)
    snap_b, keep, pos = [], [], 0
    pending = []  # (call index, set index) whose results of engine B have not been copied out yet
    def collect():
        b.sync()
        for k, j in pending:
            snap_b.append((k, {key: (v.clone() if v is not None else None) for key, v in ring_b[j].items()}))
        pending.clear()
    retune_at = len(sizes) // 2 if seed % 5 >= 3 else -1
    for k, s_ in enumerate(sizes):
        if k == retune_at:  # SdrDevice::setFrequencyRange in the middle of a run of overlapped calls: buffers reset, noise learned afresh
            for e in (a, b):
                e.set_frequency_range(CENTER + 1_000_000 - FS // 2, CENTER + 1_000_000 + FS // 2)
                e.reset()
        chunk = np.ascontiguousarray(iq[pos:pos + s_])
        host_t = torch.from_numpy(chunk.view(np.float32) if chunk.dtype == np.complex64 else chunk)
        d_iq = host_t.to(dev)
        keep.append(d_iq)
        _call(a, d_iq, s_, outs_a[k])
        a.sync()
        what = rng.integers(0, 12)
        if what == 0:
            b.flush()
        elif what == 1 and k > 3 and not (0 <= k - retune_at <= 3):  # (engine A is one call ahead here: equal once the learning frames are behind both)
            np.testing.assert_array_equal(b.read_noise()[0], a.read_noise()[0])
        elif what == 2:  # the caller produces this call's input on the public stream: the library's side queues must wait for it
            d_iq2 = torch.empty_like(d_iq)
            torch.cuda.synchronize()
            with torch.cuda.stream(pub):
                big = torch.ones(1 << 24, device=dev)
                for _ in range(6):
                    big = big * 1.0001 + 0.5  # a few hundred microseconds of work ahead of the copy
                d_iq2.copy_(d_iq)
            keep.append(d_iq2)
            keep.append(big)
            d_iq = d_iq2
        j = k % sets
        if any(jj == j for _, jj in pending):  # the caller is about to reuse a set it has not read yet: read first
            if sets >= 5 or rng.integers(0, 2):
                collect()
            else:  # ... or not: the library must notice the reuse itself; only the newest contents of the set can be compared
                pending[:] = [(kk, jj) for kk, jj in pending if jj != j]
        _call(b, d_iq, s_, ring_b[j])
        pending.append((k, j))
        pos += s_
    collect()
    if flags:
        ra, rb = a.spectrogram_read(), b.spectrogram_read()
        assert ra[2] == rb[2] == (nframes if retune_at < 0 else sum(sizes[retune_at:]))
        np.testing.assert_array_equal(ra[0], rb[0])
        np.testing.assert_array_equal(ra[1], rb[1])
    assert len(snap_b) >= len(sizes) // 2
    total = 0
    for k, ob in snap_b:
        s_ = sizes[k]
        cut = lambda o: {key: (v[:s_] if key in ("psd", "rel", "avg") and v is not None else (v[:s_ + 1] if key == "off" else v)) for key, v in o.items()}
        total += _same(cut(outs_a[k]), cut(ob), f"call {k} ({s_} frames)")
    assert total > (2000 if decim == 1 else 500)


def test_flush_then_stream_sync_completes_the_results():
    """ss_flush enqueues the deferred stages; after it any synchronisation of the stream (here: of the device) will do."""
    _flush_then_device_sync()


@pytest.mark.parametrize("env", [{"SS_DRAIN_TAIL_EVENT": "0"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_the_drains_join_in_its_measured_forms(monkeypatch, diag_lib, env):
    """drain_deep (specscan.hip): without the event behind the drain's last command — the barriers in front of it are the join either way.
    (The one-wave waiter in front of the join, round 6's other measured form, is removed: profiles/r06/s19_summary.txt.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _flush_then_device_sync()


def _flush_then_device_sync():
    import torch
    dev = torch.device("cuda:0")
    band = pkg.synth.SyntheticBand(N, seed=5, on_frame=40, off_frame=10_000)
    iq = band.frames_cf32(192)
    kw = dict(fft_size=N, decim=1, learn_frames=16, max_batch=64)
    host = pkg.SpectrumEngine(FS, CENTER, **kw)
    eng = pkg.SpectrumEngine(FS, CENTER, **kw)
    outs, keep = [], []
    for k in range(3):
        d_iq = torch.from_numpy(iq[64 * k:64 * k + 64].view(np.float32).copy()).to(dev)
        keep.append(d_iq)
        o = _device_outputs(torch, dev, 64, False)
        torch.cuda.synchronize()
        _call(eng, d_iq, 64, o)
        outs.append(o)
    if os.environ.get("SS_PIPELINE") != "0":  # (the whole suite can be run on the diagnostics build without stage pipelining)
        assert int(outs[2]["off"][0]) == -1  # (the last call's candidate stage has not even been launched yet)
    eng.flush()
    torch.cuda.synchronize()
    for k in range(3):
        h = host.process(iq[64 * k:64 * k + 64])
        np.testing.assert_array_equal(outs[k]["off"].cpu().numpy(), h["cand_off"])
        np.testing.assert_array_equal(outs[k]["psd"].cpu().numpy(), h["psd"])
        t = int(h["cand_off"][-1])
        np.testing.assert_array_equal(outs[k]["idx"][:t].cpu().numpy(), h["cand_idx"])
        np.testing.assert_array_equal(outs[k]["cav"][:t].cpu().numpy(), h["cand_avg"])
    assert int(outs[2]["off"][-1]) > 100


def test_reads_between_overlapped_calls_see_finished_state():
    """ss_read_window / ss_read_noise in the middle of a run of device calls drain the deferred stages first."""
    import torch
    dev = torch.device("cuda:0")
    band = pkg.synth.SyntheticBand(N, seed=6, on_frame=30, off_frame=10_000)
    iq = band.frames_cf32(160)
    kw = dict(fft_size=N, decim=1, learn_frames=12, max_batch=32, flags=pkg.abi.SS_FLAG_KEEP_PLANES)
    host = pkg.SpectrumEngine(FS, CENTER, **kw)
    eng = pkg.SpectrumEngine(FS, CENTER, **kw)
    keep = []
    for k in range(5):
        chunk = iq[32 * k:32 * k + 32]
        h = host.process(chunk)
        d_iq = torch.from_numpy(chunk.view(np.float32).copy()).to(dev)
        keep.append(d_iq)
        o = _device_outputs(torch, dev, 32, False)
        torch.cuda.synchronize()
        _call(eng, d_iq, 32, o)
        keep.append(o)
        if k >= 2:
            for plane, key in ((pkg.abi.SS_PLANE_PSD, "psd"), (pkg.abi.SS_PLANE_REL, "rel"), (pkg.abi.SS_PLANE_AVG, "avg")):
                np.testing.assert_array_equal(eng.read_window(plane, 7, 100, 900), h[key][7, 100:900])
            np.testing.assert_array_equal(eng.read_window(pkg.abi.SS_PLANE_REL, -3, 0, N), host.read_window(pkg.abi.SS_PLANE_REL, -3, 0, N))
    np.testing.assert_array_equal(eng.read_noise()[0], host.read_noise()[0])


def test_caller_reusing_its_planes_every_call_is_safe():
    """The same PSD / avg planes handed to every call, never synchronised in between: the library notices that this call's
    stages would overwrite what a deferred stage of the previous call still reads, and drains first."""
    import torch
    dev = torch.device("cuda:0")
    band = pkg.synth.SyntheticBand(N, seed=9, on_frame=40, off_frame=10_000)
    iq = band.frames_cf32(320)
    kw = dict(fft_size=N, decim=1, learn_frames=16, max_batch=64)
    host = pkg.SpectrumEngine(FS, CENTER, **kw)
    eng = pkg.SpectrumEngine(FS, CENTER, **kw)
    o = _device_outputs(torch, dev, 64, True)
    torch.cuda.synchronize()
    keep = []
    for k in range(5):
        chunk = iq[64 * k:64 * k + 64]
        h = host.process(chunk)
        d_iq = torch.from_numpy(chunk.view(np.float32).copy()).to(dev)
        keep.append(d_iq)
        _call(eng, d_iq, 64, o)
    eng.sync()
    for key, name in (("psd", "psd"), ("rel", "rel"), ("avg", "avg")):
        np.testing.assert_array_equal(o[key].cpu().numpy(), h[name])
    np.testing.assert_array_equal(o["off"].cpu().numpy(), h["cand_off"])
    t = int(h["cand_off"][-1])
    assert t > 1000
    np.testing.assert_array_equal(o["idx"][:t].cpu().numpy(), h["cand_idx"])
    np.testing.assert_array_equal(o["cav"][:t].cpu().numpy(), h["cand_avg"])


@pytest.mark.parametrize("n,fs,max_batch,fmt", [(65536, 20_000_000, 64, "cs8"), (4096, 1_024_000, 1024, "cf32"), (1 << 18, 61_440_000, 16, "cf32")])
def test_other_sizes_asynchronous_calls_equal_call_by_call(n, fs, max_batch, fmt):
    """FFT sizes other than 8192 (three to six launches per call, no stage pipelining): an engine that is synchronised after
    every call against one that is synchronised once at the end; a retune with reset and a short call on the way. (A two-stream
    form — FFT kernels of call k beside detect + emit of call k-1, ordered by events — was built against this test and
    measured: 65536 x 128 int8 119.9 vs 121.2 GS/s, 2^20 x 16 77.3 vs 77.5: kernels of two streams do not overlap here; dropped.)"""
    import torch
    dev = torch.device("cuda:0")
    in_format = pkg.abi.SS_FMT_CS8 if fmt == "cs8" else pkg.abi.SS_FMT_CF32
    ncalls = 7
    band = pkg.synth.SyntheticBand(n, seed=31, on_frame=max_batch + max_batch // 2, off_frame=10_000_000)
    kw = dict(fft_size=n, decim=1, in_format=in_format, learn_frames=max_batch // 2, max_batch=max_batch)
    a, b = pkg.SpectrumEngine(fs, CENTER, **kw), pkg.SpectrumEngine(fs, CENTER, **kw)
    sizes = [max_batch, max_batch, max_batch, 3, max_batch, max_batch, max_batch][:ncalls]
    outs_a, outs_b, keep = [], [], []
    for k, s_ in enumerate(sizes):
        if k == 4:
            for e in (a, b):
                e.set_frequency_range(CENTER + fs - fs // 2, CENTER + fs + fs // 2)
                e.reset()
        chunk = band.frames_cs8(s_) if fmt == "cs8" else band.frames_cf32(s_)
        d_iq = torch.from_numpy(np.ascontiguousarray(chunk).view(np.float32) if chunk.dtype == np.complex64 else np.ascontiguousarray(chunk)).to(dev)
        keep.append(d_iq)

        def outputs():
            return dict(psd=torch.full((s_, n), -7.0, dtype=torch.float32, device=dev), off=torch.full((s_ + 1,), -1, dtype=torch.int32, device=dev),
                        idx=torch.full((s_ * 2048,), -1, dtype=torch.int32, device=dev), cav=torch.full((s_ * 2048,), -7.0, dtype=torch.float32, device=dev), rel=None, avg=None)
        oa, ob = outputs(), outputs()
        torch.cuda.synchronize()  # (torch's fills first: the engines write from their own streams)
        _call(a, d_iq, s_, oa)
        a.sync()
        _call(b, d_iq, s_, ob)
        outs_a.append(oa)
        outs_b.append(ob)
    b.sync()
    total = sum(_same(oa, ob, f"call {k}") for k, (oa, ob) in enumerate(zip(outs_a, outs_b)))
    assert total > 200


def test_diag_canary_catches_an_input_buffer_refilled_in_flight(monkeypatch, diag_lib):
    """The launch of call k + 1 reads the last frames of call k's input once more; include/specscan.h asks callers to leave
    every buffer alone until ss_sync. The diagnostics build can check that (SS_CANARY=1): a checksum of those frames right
    behind launch k and again right before launch k + 1, compared by ss_sync. A clean run passes; a producer on the context's
    stream that refills the previous call's buffer between two calls is reported."""
    import torch
    if os.environ.get("SS_DEEP") == "0" or os.environ.get("SS_PIPELINE") == "0":
        pytest.skip("launches in order: no call reads another call's input")
    monkeypatch.setenv("SS_CANARY", "1")
    dev = torch.device("cuda", 0)
    nb = 64
    band = pkg.synth.SyntheticBand(N, seed=91, on_frame=40, off_frame=10_000)
    iq = band.frames_cf32(nb * 5)
    eng = pkg.SpectrumEngine(FS, CENTER, fft_size=N, decim=1, max_batch=nb, learn_frames=8)
    bufs = [torch.from_numpy(iq[k * nb:(k + 1) * nb].view(np.float32)).to(dev) for k in range(5)]
    outs = [dict(off=torch.zeros(nb + 1, dtype=torch.int32, device=dev), idx=torch.empty(nb * 512, dtype=torch.int32, device=dev)) for _ in range(5)]

    def call(k):
        eng.process_device(bufs[k], nb, cand_off=outs[k]["off"], cand_idx=outs[k]["idx"])

    call(0)  # the learning frames: not overlapped
    eng.sync()
    for k in range(1, 5):  # (the first call after a single-call sync still runs in order; from the second on launches overlap)
        call(k)
    eng.sync()  # nothing was touched: passes
    ss_stream = torch.cuda.ExternalStream(eng.stream_handle)
    for k in range(1, 4):
        call(k)
    with torch.cuda.stream(ss_stream):  # a producer on the context's stream, behind call 3: refills ITS buffer while call 4's launch still has to read its tail
        bufs[3][-1].add_(1.0)
    call(4)
    with pytest.raises(pkg.abi.SpecscanError, match="input canary"):
        eng.sync()
