"""CS16 input (SS_FMT_CS16: interleaved little-endian int16 I,Q) on every scan path. CS16 takes CF32's path at every size and under
every flag and differs from it in the load stage alone; its default scale 1/32768 is a power of two, so (float)v * scale is exact and
an engine fed CS16 must hand out, bit for bit, what an engine fed the CF32 conversion hands out: planes, candidate lists, candidate
powers, noise ceilings, spectrogram rows. The reference side (the oracle, oracle/_ref) is fed that conversion. Run with -m gpu."""
import os

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from parity import check_all, check_plane, dont_care_limit

pytestmark = pytest.mark.gpu

A = pkg.abi
CENTER = 145_000_000
KEYS = ("psd", "rel", "avg", "cand_off", "cand_idx", "cand_avg")


def _to_cf32(iq16, scale=1.0 / 32768):
    """[F, M, 2] int16 -> [F, M] complex64, exactly (the scale is a power of two)."""
    x = iq16.astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(x).view(np.complex64)[..., 0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a


def _same(tag, a, b):
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    ba, bb = _bits(a), _bits(b)
    bad = np.flatnonzero(ba.reshape(-1) != bb.reshape(-1))
    assert bad.size == 0, (tag, bad.size, bad[:5], a.reshape(-1)[bad[:5]], b.reshape(-1)[bad[:5]])


def _engines(fs, n, decim, scale=None, **kw):
    kw16 = dict(kw, fft_size=n, decim=decim, in_format=A.SS_FMT_CS16)
    if scale is not None:
        kw16["int_scale"] = scale
    e16 = pkg.SpectrumEngine(fs, CENTER, **kw16)
    e32 = pkg.SpectrumEngine(fs, CENTER, **dict(kw, fft_size=n, decim=decim, in_format=A.SS_FMT_CF32))
    return e16, e32


def _session(e16, e32, iq16, cf, chunks, want, hooks=None, t_ms=None):
    """The same calls on both engines; every output compared bitwise call by call."""
    pos = 0
    for k, size in enumerate(chunks):
        if hooks and k in hooks:
            for e in (e16, e32):
                hooks[k](e)
        t = None if t_ms is None else t_ms[pos:pos + size]
        g16 = e16.process(iq16[pos:pos + size], t_ms=t, want=want)
        g32 = e32.process(cf[pos:pos + size], t_ms=t, want=want)
        for key in KEYS:
            if key in g32:
                _same(f"call {k} {key}", g16[key], g32[key])
        pos += size
    assert pos == iq16.shape[0]
    t16, r16 = e16.read_noise()
    t32, r32 = e32.read_noise()
    assert r16 == r32
    _same("noise", t16, t32)
    return r16


def _ragged(total, max_batch, rng):
    out = []
    while sum(out) < total:
        out.append(int(min(total - sum(out), rng.integers(1, max_batch + 1))))
    return out


def _retune(fs):
    return lambda e: (e.set_frequency_range(CENTER + fs // 2, CENTER + fs + fs // 2), e.reset())


BIT_CASES = [
    # n, fs, decim, nframes, max_batch, want (() = detect mode), learn
    (64, 16_000, 1, 120, 17, ("psd", "rel", "avg"), 20),
    (512, 128_000, 3, 100, 40, ("psd", "rel", "avg"), 15),
    (2048, 512_000, 1, 90, 32, ("psd", "rel", "avg"), 12),
    (8192, 2_048_000, 1, 96, 48, ("psd", "rel", "avg"), 12),
    (8192, 2_048_000, 5, 70, 30, ("psd", "rel", "avg"), 12),
    (32768, 6_000_000, 1, 60, 24, ("psd", "rel", "avg"), 8),
    (65536, 20_000_000, 1, 56, 25, (), 6),
    (65536, 20_000_000, 1, 40, 16, ("psd", "rel", "avg"), 6),
    (131072, 20_000_000, 1, 40, 20, (), 4),
    (262144, 61_440_000, 1, 24, 12, (), 4),
    (1 << 20, 61_440_000, 1, 24, 16, (), 3),
]


@pytest.mark.parametrize("n,fs,decim,nframes,max_batch,want,learn", BIT_CASES)
def test_cs16_is_bit_identical_to_cf32(n, fs, decim, nframes, max_batch, want, learn):
    band = pkg.synth.SyntheticBand(n, decim=decim, seed=n % 97 + decim, on_frame=learn + 3, off_frame=nframes - 3)
    iq16 = band.frames_cs16(nframes)
    cf = _to_cf32(iq16)
    e16, e32 = _engines(fs, n, decim, learn_frames=learn, max_batch=max_batch)
    rng = np.random.default_rng(n + decim)
    chunks = _ragged(nframes, max_batch, rng)
    mid = len(chunks) // 2
    hooks = {mid: _retune(fs), mid + 1: lambda e: e.reset()} if len(chunks) > 2 else None
    _session(e16, e32, iq16, cf, chunks, want, hooks)


@pytest.mark.parametrize("decim", [1, 5])
@pytest.mark.parametrize("flags", [A.SS_FLAG_STREAM_ORDERED, A.SS_FLAG_REFERENCE_NAN, A.SS_FLAG_SPECTROGRAM])
def test_cs16_8192_under_flags(decim, flags):
    n, fs, nframes, learn = 8192, 2_048_000, 80, 10
    band = pkg.synth.SyntheticBand(n, decim=decim, seed=40 + decim + flags, on_frame=learn + 3, off_frame=nframes - 3)
    iq16 = band.frames_cs16(nframes)
    cf = _to_cf32(iq16)
    e16, e32 = _engines(fs, n, decim, learn_frames=learn, max_batch=32, flags=flags)
    chunks = [7, 32, 1, 19, 21]
    _session(e16, e32, iq16, cf, chunks, ("psd", "rel", "avg"), hooks={3: _retune(fs)})
    if flags & A.SS_FLAG_SPECTROGRAM:
        r16, m16, c16 = e16.spectrogram_read()
        r32, m32, c32 = e32.spectrogram_read()
        assert c16 == c32 > 0
        _same("spectrogram row", r16, r32)
        _same("spectrogram means", m16, m32)


@pytest.mark.parametrize("decim", [1, 5])
def test_cs16_8192_pipelined_device_entry_point(decim):
    """ss_process_device from a torch int16 tensor, consecutive calls overlapping on the library's queues (the default contract)."""
    import torch
    n, fs, learn = 8192, 2_048_000, 10
    calls = [37, 64, 5, 64, 30]
    nframes = sum(calls)
    band = pkg.synth.SyntheticBand(n, decim=decim, seed=60 + decim, on_frame=learn + 3, off_frame=nframes - 3)
    iq16 = band.frames_cs16(nframes)
    cf = _to_cf32(iq16)
    e16, e32 = _engines(fs, n, decim, learn_frames=learn, max_batch=64)
    dev = torch.device("cuda:0")
    src = {16: torch.from_numpy(iq16).to(dev), 32: torch.from_numpy(cf.view(np.float32)).to(dev)}
    outs = {16: [], 32: []}
    torch.cuda.synchronize()
    pos = 0
    for size in calls:
        for bits, e in ((16, e16), (32, e32)):
            planes = [torch.empty((size, n), dtype=torch.float32, device=dev) for _ in range(3)]
            off = torch.zeros(size + 1, dtype=torch.int32, device=dev)
            idx = torch.empty(size * n, dtype=torch.int32, device=dev)
            cav = torch.empty(size * n, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            e.process_device(src[bits][pos:pos + size], size, *planes, off, idx, cav)
            outs[bits].append((planes, off, idx, cav))
        pos += size
    e16.sync()
    e32.sync()
    e16.input_wait(None, 1)  # ss_input_wait on a CS16 context: the ranges it waits for are CS16-sized
    e16.sync()
    seen = 0
    for k, (a, b) in enumerate(zip(outs[16], outs[32])):
        for name, x, y in zip(("psd", "rel", "avg"), a[0], b[0]):
            _same(f"call {k} {name}", x.cpu().numpy(), y.cpu().numpy())
        _same(f"call {k} cand_off", a[1].cpu().numpy(), b[1].cpu().numpy())
        total = int(b[1][-1])
        seen += total
        _same(f"call {k} cand_idx", a[2][:total].cpu().numpy(), b[2][:total].cpu().numpy())
        _same(f"call {k} cand_avg", a[3][:total].cpu().numpy(), b[3][:total].cpu().numpy())
    assert seen > 0


CASES = [  # the sizes of test_gpu_parity.CASES: n, fs, decim, nframes, chunk, learn, seed
    (64, 16_000, 1, 120, 17, 20, 1),
    (1024, 256_000, 1, 150, 64, 30, 2),
    (2048, 512_000, 3, 90, 32, 25, 3),
    (512, 128_000, 1, 5000, 5000, 40, 12),
    (4096, 1_024_000, 1, 80, 80, 22, 4),
    (8192, 2_048_000, 1, 96, 48, 24, 5),
    (8192, 2_048_000, 5, 70, 70, 21, 6),
    (16384, 4_096_000, 1, 64, 30, 10, 7),
    (32768, 6_000_000, 1, 60, 24, 8, 10),
    (65536, 20_000_000, 1, 56, 25, 6, 8),
    (131072, 20_000_000, 1, 40, 20, 4, 9),
]


def _run(chain, iq, chunk):
    outs = [chain.process(iq[a:a + chunk]) for a in range(0, iq.shape[0], chunk)]
    res = {k: np.concatenate([o[k] for o in outs]) for k in ("psd", "rel", "avg", "cand_idx", "cand_avg")}
    counts = np.concatenate([np.diff(o["cand_off"]) for o in outs])
    res["cand_off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return res


@pytest.mark.parametrize("n,fs,decim,nframes,chunk,learn,seed", CASES)
def test_cs16_matches_oracle(oracle_mod, n, fs, decim, nframes, chunk, learn, seed):
    band = pkg.synth.SyntheticBand(n, decim=decim, seed=seed, on_frame=learn + 5, off_frame=nframes - 3)
    iq16 = band.frames_cs16(nframes)
    kw = dict(fft_size=n, decim=decim, learn_frames=learn, max_batch=max(chunk, 8))
    eng = pkg.SpectrumEngine(fs, CENTER, in_format=A.SS_FMT_CS16, **kw)
    orc = oracle_mod.oracle_chain(fs, CENTER, in_format=A.SS_FMT_CF32, **kw)  # (the oracle reads no CS16: it gets the exact conversion)
    got, ref = _run(eng, iq16, chunk), _run(orc, _to_cf32(iq16), chunk)
    errs, ncand, ndc = check_all(got, ref)
    assert ncand > (50 if n >= 256 else 5), "the test vector must produce detections"
    assert ndc <= dont_care_limit(ncand), (ncand, ndc)
    thr_g, ready_g = eng.read_noise()
    thr_o, ready_o = orc.read_noise()
    assert ready_g and ready_o
    check_plane("noise ceiling", thr_g[None], thr_o[None])


def test_cs16_matches_the_reference(ref_mod):
    """Against the reference's own sources compiled in place (oracle/_ref), as smoke() checks CF32."""
    n, fs = 8192, 2_048_000
    band = pkg.synth.SyntheticBand(n, seed=0, on_frame=12, off_frame=40)
    iq16 = band.frames_cs16(48)
    t = (1_000 + 250 * np.arange(48)).astype(np.int64)
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=64, in_format=A.SS_FMT_CS16)
    got = eng.process(iq16, t_ms=t)
    ref_mod.ref().orc_set_fft_backend(0)
    r = ref_mod.RefChain(n, fs, CENTER - fs // 2, CENTER + fs // 2).process(_to_cf32(iq16), t)
    off = np.zeros(49, np.int32)
    off[1:] = np.cumsum([len(c) for c in r["cands"]])
    want = {"psd": r["psd"], "rel": r["rel"], "avg": r["avg"], "cand_off": off, "cand_idx": np.concatenate(r["cands"]).astype(np.int32)}
    errs, ncand, ndc = check_all(got, want)
    assert ncand > 100 and ndc <= dont_care_limit(ncand), (ncand, ndc)


@pytest.mark.parametrize("n,fs", [(512, 128_000), (8192, 2_048_000), (65536, 20_000_000), (1 << 20, 61_440_000)])
def test_cs16_edge_values(n, fs):
    """Full-scale values (-32768, 32767) and all-zero frames (the -inf of log2(0)), with and without SS_FLAG_REFERENCE_NAN."""
    nframes = 24 if n < (1 << 20) else 12
    rng = np.random.default_rng(n)
    iq16 = rng.integers(-300, 300, size=(nframes, n, 2)).astype(np.int16)
    iq16[2] = np.where(rng.random((n, 2)) < 0.5, -32768, 32767).astype(np.int16)
    iq16[3, :, 0], iq16[3, :, 1] = -32768, 32767
    iq16[5] = 0
    iq16[6, : n // 2] = 0
    cf = _to_cf32(iq16)
    for flags in (0, A.SS_FLAG_REFERENCE_NAN):
        e16, e32 = _engines(fs, n, 1, learn_frames=4, max_batch=8, flags=flags)
        _session(e16, e32, iq16, cf, [3, 8, 1, 8, 4] if nframes == 24 else [3, 8, 1], ("psd", "rel", "avg"))
        if not flags:
            assert np.isneginf(e16.process(iq16[5:6])["psd"]).all()  # an all-zero frame: -inf in every bin, as for CF32 zeros


@pytest.mark.parametrize("n,fs", [(2048, 512_000), (8192, 2_048_000), (65536, 20_000_000), (1 << 20, 61_440_000)])
def test_cs16_tone_lands_in_its_own_bin(n, fs):
    """A complex exponential at +f must peak in +f's bin: I is the low half of each 32-bit word (swapped halves give -f)."""
    k = n // 8 + 3
    ph = 2 * np.pi * k * np.arange(n) / n
    iq16 = np.stack([np.rint(12000 * np.cos(ph)), np.rint(12000 * np.sin(ph))], axis=-1).astype(np.int16)[None].repeat(2, 0)
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=2, learn_frames=1, in_format=A.SS_FMT_CS16)
    psd = eng.process(iq16)["psd"]
    x = iq16[0, :, 0].astype(np.float64) + 1j * iq16[0, :, 1]
    plus = int(np.argmax(np.abs(np.fft.fftshift(np.fft.fft(x)))))  # the dB row is in the reference's shifted order
    minus = int(np.argmax(np.abs(np.fft.fftshift(np.fft.fft(np.conj(x))))))
    assert plus != minus
    assert int(np.argmax(psd[0])) == plus
    assert psd[0, plus] > psd[0, minus] + 60


@pytest.mark.parametrize("n,fs", [(8192, 2_048_000), (65536, 20_000_000)])
def test_cs16_custom_scale_12_bit(n, fs):
    """int_scale = 1/2048 (a 12-bit device, PlutoSDR): bit-identical to CF32 of x / 2048."""
    band = pkg.synth.SyntheticBand(n, seed=77, on_frame=9, off_frame=40)
    iq16 = (band.frames_cs16(44) >> 4).astype(np.int16)  # 12-bit values in int16
    assert np.abs(iq16.astype(np.int64)).max() <= 2048
    e16, e32 = _engines(fs, n, 1, scale=1.0 / 2048, learn_frames=6, max_batch=16)
    _session(e16, e32, iq16, _to_cf32(iq16, 1.0 / 2048), [16, 5, 16, 7], ("psd", "rel", "avg"))


def test_cs16_feed_equals_process():
    n, fs, nframes, batch = 8192, 2_048_000, 100, 32
    band = pkg.synth.SyntheticBand(n, seed=9, on_frame=15, off_frame=90)
    iq16 = band.frames_cs16(nframes)
    kw = dict(fft_size=n, decim=1, learn_frames=10, max_batch=batch, in_format=A.SS_FMT_CS16)
    sync = pkg.SpectrumEngine(fs, CENTER, **kw)
    eng = pkg.SpectrumEngine(fs, CENTER, **kw)
    feed = eng.feed(depth=3, cand_cap=1 << 20, want_psd=True)
    pos = 0
    while pos < nframes:
        size = min(batch, nframes - pos)
        buf = feed.acquire()
        assert buf.dtype == np.int16 and buf.shape == (batch, n, 2)
        buf[:size] = iq16[pos:pos + size]
        feed.submit(size, tag=pos)
        r = feed.collect()
        want = sync.process(iq16[pos:pos + size])
        assert r["tag"] == pos and r["nframes"] == size
        _same("feed psd", r["psd"], want["psd"])
        _same("feed cand_off", r["cand_off"], want["cand_off"])
        _same("feed cand_idx", r["cand_idx"], want["cand_idx"])
        _same("feed cand_avg", r["cand_avg"], want["cand_avg"])
        pos += size
    feed.close()


def test_cs16_replay_file_equals_process(tmp_path):
    from rtl_sdr_scanner_cpp_amd import replay
    import time
    n, fs, decim, nframes = 8192, 2_048_000, 2, 90
    band = pkg.synth.SyntheticBand(n, decim=decim, seed=11, on_frame=15, off_frame=80)
    iq16 = band.frames_cs16(nframes)
    name = replay.make_raw_file_name("full", "cs16", CENTER, fs, time.struct_time((2025, 3, 7, 9, 5, 1, 0, 0, -1)))
    path = tmp_path / name[2:]
    iq16.tofile(path)
    info = replay.parse_raw_file_name(str(path))
    kw = dict(fft_size=n, decim=decim, learn_frames=10, max_batch=32, **replay.engine_overrides_for(info))
    res = list(replay.replay_file(pkg.SpectrumEngine(fs, CENTER, **kw), str(path), batch=32, want_psd=True))
    want = pkg.SpectrumEngine(fs, CENTER, **kw)
    pos = 0
    for r in res:
        size = r["nframes"]
        assert r["first_frame"] == pos
        w = want.process(iq16[pos:pos + size])  # (whole N*D items: the chain keeps the first N of each)
        _same("replay psd", r["psd"], w["psd"])
        _same("replay cand_idx", r["cand_idx"], w["cand_idx"])
        _same("replay cand_avg", r["cand_avg"], w["cand_avg"])
        pos += size
    assert pos == nframes


@pytest.mark.parametrize("seed", range(int(os.environ.get("SS_CS16_FUZZ_SEEDS", "12"))))
def test_cs16_random_session(seed):
    rng = np.random.default_rng(7000 + seed)
    sizes = [64, 256, 1024, 4096, 8192, 8192, 16384, 65536] if seed % 3 else [8192, 32768, 65536, 131072]
    n = int(rng.choice(sizes))
    decim = int(rng.choice([1, 1, 2, 5])) if n <= 16384 else 1
    fs = int(n * rng.choice([200, 250, 125]))
    nframes = int(rng.integers(60, 160)) if n <= 8192 else int(rng.integers(30, 70))
    learn = int(rng.integers(3, 20))
    max_batch = int(rng.choice([8, 16, 64]))
    ign = []
    if rng.random() < 0.5:
        lo = CENTER + int(rng.integers(-fs // 3, fs // 4))
        ign = [lo, lo + fs // 20]
    want = ("psd", "rel", "avg") if rng.random() < 0.6 else ()
    band = pkg.synth.SyntheticBand(n, decim=decim, seed=300 + seed, on_frame=learn + 3, off_frame=nframes - 4)
    iq16 = band.frames_cs16(nframes, full_scale=float(rng.choice([0.05, 0.5, 2.0])))
    e16, e32 = _engines(fs, n, decim, learn_frames=learn, max_batch=max_batch, ignored=ign)
    chunks = _ragged(nframes, max_batch, rng)
    hooks = {}
    for k in rng.choice(len(chunks), size=min(2, len(chunks)), replace=False):
        hooks[int(k)] = _retune(fs) if rng.random() < 0.5 else (lambda e: e.reset())
    _session(e16, e32, iq16, _to_cf32(iq16), chunks, want, hooks)
