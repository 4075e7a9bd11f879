"""The oracle's handling of ss_config.window and ss_config.int_scale, on the CPU (oracle/liboracle.so alone): the GPU tests
(tests/test_gpu_window.py, tests/test_gpu_int8_scale.py) compare the engine with the oracle under caller-supplied taps and integer
scales, so the oracle's own reading of the two fields is anchored here against fp64 numpy — and the choice of the test windows
(tests/windows.py) is pinned: a wrong tap order must be visible through the parity contract."""
import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from parity import TOL, check_all, check_plane, floor_tolerance, fp64_psd_rows, hamming_f32
from windows import WINDOWS, mirrored, pair_swapped, rolled, rough

A = pkg.abi
CENTER = 145_000_000
PLANES = ("psd", "rel", "avg", "cand_off", "cand_idx", "cand_avg")


def _bitwise(a, b):
    for k in PLANES:
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)), k


@pytest.mark.parametrize("name", ["rough", "bh4", "rect"])
@pytest.mark.parametrize("n,fs,nframes", [(64, 16_000, 16), (2048, 512_000, 8), (8192, 2_048_000, 8), (131072, 20_000_000, 3)])
def test_oracle_psd_under_a_window_against_fp64(oracle_mod, name, n, fs, nframes):
    """Oracle PSD with the caller's taps against an fp64 FFT of the same fp32 products: every bin within the contract's
    1e-4 max(1, |truth|) plus HALF the floor allowance (floor_tolerance is the distance of TWO fp32 FFTs; one of them against the
    truth gets half)."""
    w = WINDOWS[name](n)
    iq = pkg.synth.SyntheticBand(n, seed=n % 89, on_frame=2, off_frame=nframes).frames_cf32(nframes)
    got = oracle_mod.oracle_chain(fs, CENTER, fft_size=n, decim=1, learn_frames=2, max_batch=nframes, window=w).process(iq)["psd"]
    truth = fp64_psd_rows(iq, fs, window=w)
    err = np.abs(got.astype(np.float64) - truth)
    bad = ~(err <= TOL * np.maximum(1.0, np.abs(truth)) + 0.5 * floor_tolerance(truth))
    assert not bad.any(), (int(bad.sum()), float(err[bad].max()))


@pytest.mark.parametrize("n,fs", [(64, 16_000), (2048, 512_000), (8192, 2_048_000)])
def test_oracle_explicit_hamming_is_the_default(oracle_mod, n, fs):
    iq = pkg.synth.SyntheticBand(n, seed=3, on_frame=8, off_frame=40).frames_cf32(44)
    kw = dict(fft_size=n, decim=1, learn_frames=5, max_batch=44)
    _bitwise(oracle_mod.oracle_chain(fs, CENTER, window=hamming_f32(n), **kw).process(iq), oracle_mod.oracle_chain(fs, CENTER, **kw).process(iq))


def test_a_wrong_tap_order_is_visible_with_the_rough_window_and_not_with_hamming(oracle_mod):
    """Why the GPU tests use windows.rough: the oracle under the rough taps against the oracle under the same taps mirrored, rolled by
    one and pair-swapped fails check_plane with most bins outside (measured: ~61 000 of 61 440 bins, the worst by 44 dB), while
    mirrored Hamming taps — exactly symmetric — give the same bits, so a mirrored tap table in a kernel would pass every Hamming test.
    (At 65536 and 2^20 points a table rolled by one or pair-swapped moves < 0.3 % of the bins under Hamming: smooth taps hide local
    permutations too.) Do not swap the rough window for a smooth or symmetric one."""
    n, fs, nframes = 2048, 512_000, 30
    iq = pkg.synth.SyntheticBand(n, seed=5, on_frame=8, off_frame=27).frames_cf32(nframes)
    kw = dict(fft_size=n, decim=1, learn_frames=5, max_batch=nframes)
    w = rough(n)
    ref = oracle_mod.oracle_chain(fs, CENTER, window=w, **kw).process(iq)
    floor = floor_tolerance(ref["psd"])
    for wrong in (mirrored, rolled, pair_swapped):
        got = oracle_mod.oracle_chain(fs, CENTER, window=wrong(w), **kw).process(iq)
        with pytest.raises(AssertionError, match="bins outside tolerance"):
            check_plane(wrong.__name__, got["psd"], ref["psd"], floor)
        outside = ~(np.abs(got["psd"] - ref["psd"]) <= TOL * np.maximum(1.0, np.abs(ref["psd"])) + floor)
        assert outside.mean() > 0.9, (wrong.__name__, float(outside.mean()))
    h = hamming_f32(n)
    assert np.array_equal(h, mirrored(h))
    _bitwise(oracle_mod.oracle_chain(fs, CENTER, window=mirrored(h), **kw).process(iq), oracle_mod.oracle_chain(fs, CENTER, **kw).process(iq))


@pytest.mark.parametrize("scale", [1.0, 1.0 / 100, 0.0123])
@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_oracle_int_scale_is_the_cf32_conversion(oracle_mod, fmt, scale):
    """CS8 / CU8 with a caller's int_scale == the oracle fed CF32 ((float)p - offset) * (float)scale, bit for bit."""
    n, fs, nframes = 2048, 512_000, 44
    band = pkg.synth.SyntheticBand(n, seed=7, on_frame=8, off_frame=40)
    raw = band.frames_cs8(nframes) if fmt == "cs8" else band.frames_cu8(nframes)
    off = np.float32(0.0 if fmt == "cs8" else 127.5)
    cf = np.ascontiguousarray((raw.astype(np.float32) - off) * np.float32(scale)).view(np.complex64)[..., 0]
    kw = dict(fft_size=n, decim=1, learn_frames=5, max_batch=nframes)
    a = oracle_mod.oracle_chain(fs, CENTER, in_format=A.SS_FMT_CS8 if fmt == "cs8" else A.SS_FMT_CU8, int_scale=scale, **kw).process(raw)
    b = oracle_mod.oracle_chain(fs, CENTER, **kw).process(cf)
    _bitwise(a, b)
    assert check_all(a, b)[1] > 500
