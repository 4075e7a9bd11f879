"""An fp64 model of one recording slot of the channeliser (csrc/channelizer.hip), in plain numpy / scipy: nothing from csrc/,
nothing from the oracle's arithmetic. TEST INFRASTRUCTURE, anchored against the oracle by tests/test_chan_ref.py and pointed at
the GPU by tests/test_gpu_channelizer_fp64.py.

  increment  the angle of the rotator's fp32 increment as sc_start forms it (recorder.cpp:64 -> rotator::set_phase_incr): the
             ratio in double over a float rate, the angle as a float, cosf / sinf / hypotf of the C library (through ctypes, as
             the library itself calls them; numpy's float32 cos / sin are other functions and differ by an ulp at some shifts),
             normalised in fp32, then atan2 in double.
  phase      of the n-th sample a slot has seen: the running sum of the increment in force, mod 1, in fp64. It advances only
             while the slot records; a restart on another shift changes the increment and keeps the phase.
  cascade    scipy.signal.upfirdn in fp64 per stage over everything the slot recorded, each stage cut to the length a streaming
             resampler produces (output m's window ends at input sample m * D // I: ceil(n * I / D) outputs for n samples).
"""
import ctypes as C
import ctypes.util
import math
from collections import namedtuple

import numpy as np
from scipy import signal

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _name in ("cosf", "sinf"):
    getattr(_libm, _name).argtypes = [C.c_float]
    getattr(_libm, _name).restype = C.c_float
_libm.hypotf.argtypes = [C.c_float, C.c_float]
_libm.hypotf.restype = C.c_float

# (fs, bw, threshold, stages (interp, decim), first-stage form): every first-stage form of sc_create's dispatch, its range
# edges, the workgroup-size switch (four waves up to D = 85, two from 86) and the ways into the generic kernel
CASCADES = [
    (16_000, 16_000, 125, [(1, 1)], "<3,1>"),
    (48_000, 16_000, 125, [(1, 3)], "<3,1>"),
    (128_000, 16_000, 125, [(1, 8)], "<3,1>"),  # top of <3,1>
    (144_000, 16_000, 125, [(1, 9)], "<4,1>"),  # bottom of <4,1>
    (250_000, 25_000, 125, [(1, 10)], "<4,1>"),
    (272_000, 16_000, 125, [(1, 17)], "<5,1>"),  # bottom of <5,1>
    (1_024_000, 32_000, 125, [(1, 32)], "<5,1>"),  # top of <5,1>
    (528_000, 16_000, 125, [(1, 33)], "<6,1>"),  # bottom of <6,1>
    (2_048_000, 32_000, 125, [(1, 64)], "<6,1>"),  # top of <6,1>: the straight span == U * TPB staging
    (1_040_000, 16_000, 125, [(1, 65)], "<6,2>"),  # bottom of <6,2>: one live branch in pass 2
    (2_400_000, 32_000, 125, [(1, 75)], "<6,2>"),
    (1_360_000, 16_000, 125, [(1, 85)], "<6,2>"),  # the last D with four waves
    (1_376_000, 16_000, 125, [(1, 86)], "<6,2>"),  # the first D with two waves
    (2_032_000, 16_000, 125, [(1, 127)], "<6,2>"),
    (2_048_000, 16_000, 128, [(1, 128)], "<6,2>"),  # top of <6,2>
    (2_096_000, 16_000, 125, [(1, 131)], "generic"),  # D > 128
    (1_000_000, 16_000, 125, [(2, 125)], "generic"),  # interpolation at the input
    (2_048_000, 16_000, 125, [(1, 8), (1, 16)], "<3,1>"),  # feeding next_buf
    (1_024_000, 20_000, 125, [(1, 16), (5, 16)], "<4,1>"),  # interpolating second stage
    (61_440_000, 32_000, 125, [(1, 40), (1, 48)], "<6,1>"),  # feeding next_buf
]
WAVES = {85: 4, 86: 2, 127: 2, 128: 2}  # decimation -> waves per workgroup where the table pins it; every other row: 4


def cascade_id(row):
    return f"{row[0]}-{row[1]}-" + "x".join(f"{i}_{d}" for i, d in row[3])


FirstStage = namedtuple("FirstStage", "form waves tile")  # tile: outputs per workgroup


def first_stage(stages):
    """Which first-stage kernel a cascade [(interp, decim, ntaps), ...] takes, by sc_create's rule: the polyphase-by-branch
    k_chan_dec<LOGG, PASSES> for interpolation 1, decimation <= 128 and <= 33 taps per branch, with as many waves (4, 2, 1) as
    keep the staged span of a tile within 64 KiB of LDS; else the generic k_chan_stage<true> (256 threads)."""
    i, d, ntaps = stages[0]
    nt = (ntaps + i - 1) // i
    tile = 64
    while True:
        span = (tile - 1) * d // i + 1 + nt
        cols = (span + d) // d + 2
        if (cols | 1) * d * 8 <= 64 * 1024 or tile == 1:
            break
        tile //= 2
    if i != 1 or d > 128 or ntaps > 33 * d:
        return FirstStage("generic", 4, tile)
    logg = 3
    while (1 << logg) < d and logg < 6:
        logg += 1
    for waves in (4, 2, 1):
        t = waves * (64 >> logg) * 16
        if ((t - 1) * d + 33 * d) * 8 <= 64 * 1024:
            return FirstStage(f"<{logg},{2 if d > 64 else 1}>", waves, t)
    return FirstStage("generic", 4, tile)


def increment(fs, shift):
    """Revolutions per sample of the rotator's fp32 increment for this shift (sc_start)."""
    ratio = float(-shift) / float(np.float32(fs))
    ang = np.float32(float(np.longdouble(2.0) * np.longdouble("3.141592653589793238462643383279502884") * np.longdouble(ratio)))
    re, im = np.float32(_libm.cosf(float(ang))), np.float32(_libm.sinf(float(ang)))
    mag = np.float32(_libm.hypotf(float(re), float(im)))
    return math.atan2(float(np.float32(im / mag)), float(np.float32(re / mag))) / (2.0 * math.pi)


def produced(n, interp, decim):
    """Outputs of a streaming rational resampler that starts from rest, for n input samples."""
    return -((-n * interp) // decim)


class SlotModel:
    """One slot: start(shift), feed(x) for every call it records in, output() for all it should have produced so far."""

    def __init__(self, fs, stages, taps):
        self.fs = fs
        self.stages = [(int(i), int(d)) for i, d, *_ in stages]
        self.taps = [np.asarray(t, np.float64) for t in taps]
        assert len(self.taps) == len(self.stages)
        self.df = 0.0
        self.f0 = 0.0  # phase of the next sample, revolutions
        self._rot, self._phi = [], []

    def start(self, shift):
        self.df = increment(self.fs, shift)

    def feed(self, x):
        x = np.asarray(x).astype(np.complex128)
        phi = (self.f0 + np.arange(len(x), dtype=np.float64) * self.df) % 1.0
        self.f0 = (self.f0 + len(x) * self.df) % 1.0
        self._phi.append(phi)
        self._rot.append(x * np.exp(2j * np.pi * phi))

    def phase(self):
        """Rotator phase (revolutions) of every sample recorded so far."""
        return np.concatenate(self._phi) if self._phi else np.zeros(0)

    def output(self):
        y = np.concatenate(self._rot) if self._rot else np.zeros(0, np.complex128)
        for (i, d), t in zip(self.stages, self.taps):
            n = len(y)
            y = signal.upfirdn(t, y, up=i, down=d)[:produced(n, i, d)] if n else y
        return y


def decreep(got, ref, in_per_out):
    """Remove the best-fit linear phase ramp between got and ref: (residual max |error| / max |ref|, slope per input sample)."""
    w = np.abs(ref) ** 2
    d = np.angle(got * np.conj(ref))
    k = np.arange(len(ref), dtype=np.float64)
    slope = float((w * k) @ d / ((w * k) @ k))
    return float(np.abs(got * np.exp(-1j * slope * k) - ref).max() / np.abs(ref).max()), slope / in_per_out


# ---------------------------------------------------------------------------------------------------------------------------
# impulse trains: a FIR's impulse response is its taps. With one non-zero sample per filter length every output of a
# single-stage cascade is one product taps[k] * x0 (k = m * D - n0 * I for the impulse at n0), or zero.
# ---------------------------------------------------------------------------------------------------------------------------
X0 = np.complex64(1.0 - 0.5j)  # both products with a float are exact


def impulse_spacing(ntaps, decim):
    """The smallest spacing >= the filter length that is coprime to the decimation: consecutive impulses walk every residue."""
    s = ntaps
    while math.gcd(s, decim) != 1:
        s += 1
    return s


def impulse_train(n_impulses, spacing, first=0):
    """(stream complex64, impulse positions): X0 at first + j * spacing, zeros elsewhere; the stream ends one spacing after the
    last impulse, so every response is complete."""
    pos = first + spacing * np.arange(n_impulses, dtype=np.int64)
    x = np.zeros(int(pos[-1]) + spacing, np.complex64)
    x[pos] = X0
    return x, pos


def impulse_hits(pos, n, interp, decim, ntaps):
    """For a stream of n samples with impulses at pos: (m, k, j), the outputs m that impulse j reaches and the tap k each sees."""
    nout = produced(n, interp, decim)
    ms, ks, js = [], [], []
    for j, n0 in enumerate(np.asarray(pos, np.int64)):
        lo = -((-n0 * interp) // decim)
        hi = min((n0 * interp + ntaps - 1) // decim, nout - 1)
        m = np.arange(lo, hi + 1, dtype=np.int64)
        ms.append(m)
        ks.append(m * decim - n0 * interp)
        js.append(np.full(len(m), j, np.int64))
    return np.concatenate(ms), np.concatenate(ks), np.concatenate(js)


def impulse_response_exact(pos, n, interp, decim, taps):
    """The response at shift 0 as fp32 bits: taps[k] * X0 where an impulse reaches, +0 elsewhere. Returns (complex64, hit mask)."""
    taps = np.asarray(taps, np.float32)
    m, k, _ = impulse_hits(pos, n, interp, decim, len(taps))
    out = np.zeros((produced(n, interp, decim), 2), np.float32)
    out[m, 0] = taps[k] * np.float32(X0.real) + np.float32(0.0)  # (+0: a zero tap gives +0, as an accumulator that starts at +0 does)
    out[m, 1] = taps[k] * np.float32(X0.imag) + np.float32(0.0)
    hit = np.zeros(len(out), bool)
    hit[m] = True
    return out.view(np.complex64).reshape(-1), hit


def impulse_response_rotated(pos, n, interp, decim, taps, phase):
    """The response under rotation in fp64: taps[k] * X0 * exp(2 pi i phase[n0]). Returns (complex128, hit mask)."""
    taps = np.asarray(taps, np.float64)
    m, k, j = impulse_hits(pos, n, interp, decim, len(taps))
    out = np.zeros(produced(n, interp, decim), np.complex128)
    out[m] = taps[k] * complex(X0) * np.exp(2j * np.pi * np.asarray(phase)[np.asarray(pos, np.int64)[j]])
    hit = np.zeros(len(out), bool)
    hit[m] = True
    return out, hit


def to_i8(y):
    """volk_32f_s32f_convert_8i after x127 on a complex64 array: saturate to [-128, 127], rint (ties to even) -> int8 [n, 2]."""
    r = np.ascontiguousarray(y, np.complex64).view(np.float32).reshape(-1, 2) * np.float32(127.0)
    return np.clip(np.rint(r), -128, 127).astype(np.int8)
