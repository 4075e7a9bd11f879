"""Caller-supplied window taps (ss_config.window) on every transform family, against the CPU oracle under the same taps, against an
fp64 FFT of the same windowed frames, and against the engine's own default-window results where those must be bit-identical.

With a caller's window the product library launches what the default never reaches: the table branch of the 65536-point column
tiles (fft256_kernels.h), k_fft_cols1024<FMT, 4, false> / k_fft_cols1024_plan<FMT, false> reading the permuted tap table of
fft1024_window_order at 2^20 points, and the four-step forms for int8 IQ at 65536 / 131072 points (the fold needs the default taps,
ss_create: fold_ok). The taps are windows.rough — asymmetric and not smooth, so a mirrored, shifted or locally permuted tap table
leaves the contract in > 99 % of the bins (tests/test_window_oracle.py pins that on the CPU) — plus a 4-term Blackman-Harris window
(taps down to 6e-5) and the rectangle. Run with -m gpu."""
import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from parity import all_bins_vs_fp64, check_all, check_plane, dont_care_limit, error_quantiles, excess_vs_fp64, format_all_bins, format_quantiles, hamming_f32
from test_gpu_cs16 import BIT_CASES, KEYS, _ragged, _retune, _same, _to_cf32
from windows import WINDOWS, rough

pytestmark = pytest.mark.gpu

A = pkg.abi
CENTER = 145_000_000
ALL = ("psd", "rel", "avg")

CASES = {  # n: fs, decim, nframes, max_batch, learn — the frame counts of test_gpu_cs16.BIT_CASES
    64: (16_000, 1, 120, 17, 20), 512: (128_000, 3, 100, 40, 15),                                              # generic
    1024: (256_000, 1, 90, 32, 12), 2048: (512_000, 1, 90, 32, 12), 4096: (1_024_000, 1, 80, 32, 12),          # 256-point register kernels
    8192: (2_048_000, 1, 96, 48, 12),                                                                          # fft8192_v2
    16384: (4_096_000, 1, 64, 30, 10), 32768: (6_000_000, 1, 60, 24, 8),                                       # four-step
    65536: (20_000_000, 1, 56, 25, 6), 131072: (20_000_000, 1, 40, 20, 4), 262144: (61_440_000, 1, 24, 12, 3),
    1 << 20: (61_440_000, 1, 24, 16, 3),                                                                       # two passes of 1024
}


def _cat(outs):
    res = {k: np.concatenate([o[k] for o in outs]) for k in ALL + ("cand_idx", "cand_avg") if k in outs[0]}
    res["cand_off"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(o["cand_off"]) for o in outs]))]).astype(np.int32)
    return res


def _frames(n, decim, nframes, learn, fmt, seed=None):
    band = pkg.synth.SyntheticBand(n, decim=decim, seed=n % 97 + decim if seed is None else seed, on_frame=learn + 3, off_frame=nframes - 3)
    if fmt == "cf32":
        x = band.frames_cf32(nframes)
        return x, x, A.SS_FMT_CF32, A.SS_FMT_CF32
    if fmt == "cs16":  # (the oracle reads no CS16: it gets the exact conversion, as in tests/test_gpu_cs16.py)
        x = band.frames_cs16(nframes)
        return x, _to_cf32(x), A.SS_FMT_CS16, A.SS_FMT_CF32
    x = band.frames_cs8(nframes) if fmt == "cs8" else band.frames_cu8(nframes)
    f = A.SS_FMT_CS8 if fmt == "cs8" else A.SS_FMT_CU8
    return x, x, f, f


def _against_oracle(oracle_mod, tag, n, w, fmt="cf32", want=ALL, decim=None, w_engine=None, retune=True):
    """One session — ragged call sizes, a retune with an Averager reset once the first detections are in — on an engine and on the
    oracle under the taps w; check_all, the detection counts, the noise ceiling. Returns what both handed out."""
    fs, d, nframes, max_batch, learn = CASES[n]
    decim = d if decim is None else decim
    raw, cf, f_eng, f_orc = _frames(n, decim, nframes, learn, fmt)
    kw = dict(fft_size=n, decim=decim, learn_frames=learn, max_batch=max_batch)
    eng = pkg.SpectrumEngine(fs, CENTER, in_format=f_eng, window=w if w_engine is None else w_engine, **kw)
    orc = oracle_mod.oracle_chain(fs, CENTER, in_format=f_orc, window=w, **kw)
    outs_e, outs_o, pos, retuned = [], [], 0, not retune
    for size in _ragged(nframes, max_batch, np.random.default_rng(n + decim)):
        if not retuned and pos >= learn + 26 and nframes - pos >= 8:
            for c in (eng, orc):
                _retune(fs)(c)
            retuned = True
        outs_e.append(eng.process(raw[pos:pos + size], want=want))
        outs_o.append(orc.process(cf[pos:pos + size]))
        pos += size
    got, ref = _cat(outs_e), _cat(outs_o)
    errs, ncand, ndc = check_all(got, ref)
    print(f"\n[{tag}: {n} points, {fmt}, {'planes' if want else 'detect mode'}] {ncand} reference candidates, {ndc} inside the band; |err| dB: {format_quantiles(error_quantiles(got, ref))}")
    assert ncand > (50 if n >= 256 else 5), "the test vector must produce detections"
    assert ndc <= dont_care_limit(ncand), (ncand, ndc)
    thr_g, ready_g = eng.read_noise()
    thr_o, ready_o = orc.read_noise()
    assert ready_g and ready_o
    check_plane("noise ceiling", thr_g[None], thr_o[None])
    return got, ref, cf


@pytest.mark.parametrize("n,decim,want", [(n, None, ALL) for n in CASES] + [(8192, 5, ALL)] + [(n, None, ()) for n in (65536, 262144, 1 << 20)])
def test_rough_window_matches_oracle(oracle_mod, n, decim, want):
    _against_oracle(oracle_mod, "rough", n, rough(n), want=want, decim=decim)


@pytest.mark.parametrize("name", ["bh4", "rect"])
@pytest.mark.parametrize("n", [2048, 8192, 65536, 1 << 20])
def test_blackman_harris_and_rectangle_match_oracle(oracle_mod, name, n):
    _against_oracle(oracle_mod, name, n, WINDOWS[name](n))


@pytest.mark.parametrize("n,fmt", [(8192, "cs8"), (65536, "cu8"), (131072, "cs8"), (1 << 20, "cu8"), (8192, "cs16"), (1 << 20, "cs16")])
def test_rough_window_integer_formats_match_oracle(oracle_mod, n, fmt):
    """int8 IQ under a caller's window: the sizes that leave the fold for the four-step forms, and the int8 x table-tap column tiles."""
    _against_oracle(oracle_mod, "rough", n, rough(n, seed=1), fmt=fmt)


@pytest.mark.parametrize("n,fmt", [(65536, "cs8"), (131072, "cu8"), (1 << 20, "cf32")])
def test_rough_window_device_calls_that_keep_no_plane(oracle_mod, n, fmt):
    """ss_process_device calls back to back that hand out no plane (the calls the fold would take with the default taps; at 2^20 points
    the call whose column launch carries the plan of the call before: k_fft_cols1024_plan<FMT, false>), the learning frames as a call of
    their own: candidate lists against the oracle's."""
    import torch
    fs, _, nframes, max_batch, learn = CASES[n]
    w = rough(n, seed=2)
    raw, cf, f_eng, f_orc = _frames(n, 1, nframes, learn, fmt)
    kw = dict(fft_size=n, decim=1, learn_frames=learn, max_batch=max_batch)
    ref = oracle_mod.oracle_chain(fs, CENTER, in_format=f_orc, window=w, **dict(kw, max_batch=nframes)).process(cf)
    eng = pkg.SpectrumEngine(fs, CENTER, in_format=f_eng, window=w, **kw)
    cuts = [0, learn] + list(range(learn + max_batch // 2, nframes, max_batch // 2)) + [nframes]
    dev = torch.device("cuda", 0)
    d_iq = [torch.from_numpy(raw[a:b].view(np.float32) if raw.dtype == np.complex64 else raw[a:b]).to(dev) for a, b in zip(cuts, cuts[1:])]
    outs = [dict(off=torch.zeros(b - a + 1, dtype=torch.int32, device=dev), idx=torch.empty((b - a) * 2048, dtype=torch.int32, device=dev),
                 avg=torch.empty((b - a) * 2048, dtype=torch.float32, device=dev)) for a, b in zip(cuts, cuts[1:])]
    torch.cuda.synchronize()
    for d, o in zip(d_iq, outs):
        eng.process_device(d, d.shape[0], cand_off=o["off"], cand_idx=o["idx"], cand_avg=o["avg"])
    eng.sync()
    res = []
    for o in outs:
        off = o["off"].cpu().numpy()
        res.append({"cand_off": off, "cand_idx": o["idx"].cpu().numpy()[:off[-1]], "cand_avg": o["avg"].cpu().numpy()[:off[-1]]})
    errs, ncand, ndc = check_all(_cat(res), ref)
    assert ncand > 50 and ndc <= dont_care_limit(ncand), (ncand, ndc)


@pytest.mark.parametrize("n", [2048, 8192, 65536, 1 << 20])
def test_rough_window_against_fp64(oracle_mod, n):
    """Engine and oracle PSD against the fp64 FFT of the same windowed frames; the engine held to the project's rule (parity._arbitrate):
    rms distance at most 1.5 x the oracle's + 1e-6, over all bins and on the bins where the two part."""
    fs = CASES[n][0]
    nframes = 8 if n <= 65536 else 4
    w = rough(n, seed=3)
    iq = pkg.synth.SyntheticBand(n, seed=n % 89, on_frame=2, off_frame=nframes).frames_cf32(nframes)
    kw = dict(fft_size=n, decim=1, learn_frames=2, max_batch=nframes, window=w)
    got = pkg.SpectrumEngine(fs, CENTER, **kw).process(iq)["psd"]
    ref = oracle_mod.oracle_chain(fs, CENTER, **kw).process(iq)["psd"]
    v = all_bins_vs_fp64(iq, got, ref, fs, window=w)
    print(f"\n[rough window, {n} points] {format_all_bins(v)}")
    assert v["engine"]["rms"] <= 1.5 * v["reference"]["rms"] + 1e-6, v
    excess_vs_fp64(iq, got, ref, fs, window=w)  # (asserts the same rule on the bins outside the bare 1e-4 tolerance)


@pytest.mark.parametrize("n,fs,decim,nframes,max_batch,want,learn", [c for c in BIT_CASES if c[0] not in (65536, 1 << 20)] + [(16384, 4_096_000, 1, 64, 30, ALL, 10)])
def test_explicit_hamming_is_bit_identical_where_the_default_loads_its_taps(n, fs, decim, nframes, max_batch, want, learn):
    """window = hamming(N) against window = NULL: the same tap table, so the same bits — planes, lists, cand_avg, noise ceiling —
    at every size but the two whose default forms its taps in the kernel (65536, 2^20: below)."""
    iq = pkg.synth.SyntheticBand(n, decim=decim, seed=n % 97 + decim, on_frame=learn + 3, off_frame=nframes - 3).frames_cf32(nframes)
    kw = dict(fft_size=n, decim=decim, learn_frames=learn, max_batch=max_batch)
    ea, eb = pkg.SpectrumEngine(fs, CENTER, window=hamming_f32(n), **kw), pkg.SpectrumEngine(fs, CENTER, **kw)
    chunks = _ragged(nframes, max_batch, np.random.default_rng(n + decim))
    pos = 0
    for k, size in enumerate(chunks):
        if len(chunks) > 2 and k == len(chunks) // 2:
            for e in (ea, eb):
                _retune(fs)(e)
        ga, gb = ea.process(iq[pos:pos + size], want=want), eb.process(iq[pos:pos + size], want=want)
        for key in KEYS:
            if key in gb:
                _same(f"call {k} {key}", ga[key], gb[key])
        pos += size
    (ta, ra), (tb, rb) = ea.read_noise(), eb.read_noise()
    assert ra == rb
    _same("noise", ta, tb)


@pytest.mark.parametrize("n", [65536, 1 << 20])
def test_explicit_hamming_at_the_tap_forming_sizes_matches_oracle(oracle_mod, n):
    """The table-tap column tiles under Hamming taps against the oracle (the default there forms its taps: within 1.2e-7 of these, not equal)."""
    _against_oracle(oracle_mod, "explicit Hamming", n, hamming_f32(n))


@pytest.mark.parametrize("n", [8192, 1 << 20])
def test_taps_times_two_and_samples_halved_give_the_same_bits(n):
    """Powers of two commute with every rounding in front of the FFT: window = 2 w on iq / 2 == window = w on iq, bit for bit."""
    fs, _, nframes, max_batch, learn = CASES[n]
    iq = pkg.synth.SyntheticBand(n, seed=21, on_frame=learn + 3, off_frame=nframes - 3).frames_cf32(nframes)
    w = rough(n, seed=4)
    kw = dict(fft_size=n, decim=1, learn_frames=learn, max_batch=max_batch)
    ea, eb = pkg.SpectrumEngine(fs, CENTER, window=w, **kw), pkg.SpectrumEngine(fs, CENTER, window=(2.0 * w).astype(np.float32), **kw)
    half = (iq * np.float32(0.5)).astype(np.complex64)
    total = 0
    for a in range(0, nframes, max_batch):
        ga, gb = ea.process(iq[a:a + max_batch]), eb.process(half[a:a + max_batch])
        for key in KEYS:
            _same(f"{a} {key}", ga[key], gb[key])
        total += len(ga["cand_idx"])
    assert total > 50


@pytest.mark.parametrize("n", [8192, 65536])
def test_device_entry_point_matches_host_entry_point_under_a_window(n):
    import torch
    fs, nframes = CASES[n][0], 100 if n == 8192 else 40
    iq = pkg.synth.SyntheticBand(n, seed=16, on_frame=20, off_frame=nframes - 5).frames_cf32(nframes)
    kw = dict(fft_size=n, decim=1, learn_frames=10, max_batch=128, window=rough(n, seed=5))
    host = pkg.SpectrumEngine(fs, CENTER, **kw).process(iq)
    eng = pkg.SpectrumEngine(fs, CENTER, **kw)
    dev = torch.device("cuda:0")
    d_iq = torch.from_numpy(iq.view(np.float32)).to(dev)
    planes = [torch.empty((nframes, n), dtype=torch.float32, device=dev) for _ in range(3)]
    off = torch.zeros(nframes + 1, dtype=torch.int32, device=dev)
    idx = torch.empty(nframes * 2048, dtype=torch.int32, device=dev)
    cav = torch.empty(nframes * 2048, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    eng.process_device(d_iq, nframes, *planes, off, idx, cav)
    eng.sync()
    for t, k in zip(planes, ALL):
        np.testing.assert_array_equal(t.cpu().numpy(), host[k])
    np.testing.assert_array_equal(off.cpu().numpy(), host["cand_off"])
    total = int(off[-1])
    assert total > 50
    np.testing.assert_array_equal(idx[:total].cpu().numpy(), host["cand_idx"])
    np.testing.assert_array_equal(cav[:total].cpu().numpy(), host["cand_avg"])


@pytest.mark.parametrize("n", [8192, 65536])
def test_taps_are_copied_at_create(n):
    fs, _, nframes, max_batch, learn = CASES[n]
    iq = pkg.synth.SyntheticBand(n, seed=22, on_frame=learn + 3, off_frame=nframes - 3).frames_cf32(max_batch)
    kw = dict(fft_size=n, decim=1, learn_frames=learn, max_batch=max_batch)
    w = rough(n, seed=6)
    want = pkg.SpectrumEngine(fs, CENTER, window=w.copy(), **kw).process(iq)
    eng = pkg.SpectrumEngine(fs, CENTER, window=w, **kw)  # (float32 and contiguous: ss_config.window points at this very array)
    w[:] = np.nan
    got = eng.process(iq)
    for key in KEYS:
        _same(key, got[key], want[key])


def test_two_contexts_with_different_windows(oracle_mod):
    n, fs = 2048, 512_000
    iq = pkg.synth.SyntheticBand(n, seed=23, on_frame=15, off_frame=87).frames_cf32(90)
    kw = dict(fft_size=n, decim=1, learn_frames=12, max_batch=32)
    wins = [rough(n, seed=7), WINDOWS["bh4"](n)]
    engs = [pkg.SpectrumEngine(fs, CENTER, window=w, **kw) for w in wins]
    outs = [[], []]
    for a in range(0, 90, 30):
        for e, o in zip(engs, outs):
            o.append(e.process(iq[a:a + 30]))
    for w, o in zip(wins, outs):
        ref = oracle_mod.oracle_chain(fs, CENTER, window=w, **dict(kw, max_batch=90)).process(iq)
        errs, ncand, ndc = check_all(_cat(o), ref)
        assert ncand > 50 and ndc <= dont_care_limit(ncand)
