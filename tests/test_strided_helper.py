"""tests/strided.py on the CPU: the helper itself, and the oracle under it — oracle_chain(decim=D) on the strided items hands out,
bit for bit, what oracle_chain(decim=1) hands out on the compact frames (it reads the first N samples of every item and nothing
else), while a chain that took the same bytes at a stride of N does not (the poison shows)."""
import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from strided import FORMATS, poison, strided_items

A = pkg.abi
IN_FORMAT = {"cf32": A.SS_FMT_CF32, "cs8": A.SS_FMT_CS8, "cu8": A.SS_FMT_CU8, "cs16": A.SS_FMT_CS16}
KEYS = ("psd", "rel", "avg", "cand_off", "cand_idx", "cand_avg")


def _frames(n, nframes, fmt, seed, learn=6):
    band = pkg.synth.SyntheticBand(n, seed=seed, on_frame=learn + 3, off_frame=nframes - 3)
    return {"cf32": band.frames_cf32, "cs8": band.frames_cs8, "cu8": band.frames_cu8, "cs16": band.frames_cs16}[fmt](nframes)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind in "fc" else a


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("n,nframes,decim", [(64, 5, 3), (256, 3, 2), (1000, 2, 5), (16, 1, 1)])
def test_items_hold_the_frames_then_poison(fmt, n, nframes, decim):
    dtype, pair = FORMATS[fmt]
    rng = np.random.default_rng(n + decim)
    if pair is None:  # any bit pattern must come through as it is: signed zeros, infinities, NaNs with a payload among them
        x = rng.integers(0, 1 << 32, size=(nframes, n, 2), dtype=np.uint32).view(np.complex64)[..., 0]
    else:
        x = rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max + 1, size=(nframes, n, 2)).astype(dtype)
    y = strided_items(x, decim, fmt)
    assert y.dtype == x.dtype == dtype and y.flags["C_CONTIGUOUS"]
    assert y.shape == (nframes, n * decim) + ((2,) if pair else ())
    assert y.nbytes == nframes * n * decim * A.SS_FMT_BYTES[IN_FORMAT[fmt]]  # the whole buffer, the last item included
    np.testing.assert_array_equal(_bits(y[:, :n]), _bits(x))
    gap = y[:, n:]
    assert gap.shape[1] == n * (decim - 1)
    if pair is None:
        assert np.isnan(gap.real).all() and np.isnan(gap.imag).all()
        quiet = gap.view(np.uint32) & 0x7FC00000
        assert (quiet == 0x7FC00000).all()
    else:
        flat = gap.reshape(nframes, -1).astype(np.int64)
        assert (flat[:, 0::2] == pair[0]).all() and (flat[:, 1::2] == pair[1]).all()
        info = np.iinfo(dtype)
        assert set(pair) == {info.min, info.max}
    for f in range(nframes):
        np.testing.assert_array_equal(_bits(gap[f]), _bits(poison(fmt, n * (decim - 1))))


def test_wrong_frames_are_refused():
    with pytest.raises(ValueError):
        strided_items(np.zeros((2, 64), np.complex64), 2, "cs8")
    with pytest.raises(ValueError):
        strided_items(np.zeros((2, 64, 2), np.int16), 2, "cs8")
    with pytest.raises(ValueError):
        strided_items(np.zeros((2, 64, 2), np.int8), 0, "cs8")


def _session(chain, iq, cuts):
    return [chain.process(iq[a:b]) for a, b in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("fmt", ["cf32", "cs8"])
@pytest.mark.parametrize("n,fs", [(256, 64_000), (1024, 256_000)])
def test_oracle_reads_the_first_n_of_every_item_and_nothing_else(oracle_mod, n, fs, fmt):
    decim, nframes, learn = 3, 48, 6
    x = _frames(n, nframes, fmt, seed=n % 97 + decim, learn=learn)
    y = strided_items(x, decim, fmt)
    kw = dict(fft_size=n, in_format=IN_FORMAT[fmt], learn_frames=learn, max_batch=32)
    cuts = [0, 17, 18, nframes]
    compact = _session(oracle_mod.oracle_chain(fs, 145_000_000, decim=1, **kw), x, cuts)
    strided = _session(oracle_mod.oracle_chain(fs, 145_000_000, decim=decim, **kw), y, cuts)
    total = 0
    for k, (a, b) in enumerate(zip(compact, strided)):
        for key in KEYS:
            np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=f"call {k} {key}")
        assert np.isfinite(b["psd"]).all()
        total += len(a["cand_idx"])
    assert total > 50, "equal lists say little when they are empty"
    # control: the same bytes at a stride of N — every (decim)th row is a frame, the rows between are poison, and it shows
    rows = y.reshape((nframes * decim, n) + y.shape[2:])
    wrong = oracle_mod.oracle_chain(fs, 145_000_000, decim=1, **dict(kw, max_batch=nframes * decim)).process(rows)
    right = np.concatenate([a["psd"] for a in compact])
    assert _bits(wrong["psd"][0]).tolist() == _bits(right[0]).tolist()  # (row 0 is frame 0 either way)
    for f in range(1, nframes):
        if f % decim:
            if fmt == "cf32":
                assert np.isnan(wrong["psd"][f]).all(), f
            else:  # a full-scale constant: its line at the centre bin stands above every bin of every frame (16 dB here)
                assert wrong["psd"][f, n // 2] == wrong["psd"][f].max() > right.max() + 10.0, f
        assert not np.array_equal(_bits(wrong["psd"][f]), _bits(right[f])), f
