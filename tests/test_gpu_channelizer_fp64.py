"""Every first-stage form of the recorder channeliser (csrc/channelizer.hip) against the fp64 slot model (tests/chan_ref.py)
and against its own taps, CF32 input (the integer formats are tied bit for bit to CF32 by test_gpu_channelizer_int_iq.py).
Run with -m gpu. Nothing is fitted: the engine evaluates the rotator in closed form, so the model's phase is its phase.

  a  impulse trains at shift 0: every output is taps[k] * x0 bit for bit or exactly zero — a dropped, zeroed or misplaced tap
     of any branch, in full tiles, edge tiles, short calls and across call boundaries (hist0), changes bits;
  b  the same trains under rotation: every non-zero output is taps[k] * x0 * exp(2 pi i phase(n0)) of the model to 2e-6 of its
     own magnitude — a one-sample phase slip at a tile, table or call boundary is 2 pi df >= 1e-3 rad;
  c  noise and carriers on four slots of six: the whole stream within margin * e0 (+ 2e-6 where the rotator turns), e0 being
     the CPU oracle's own fp32 floor against the same model on the same stream;
  d  start / stop / restart sessions, e sixteen slots, both with the bound of c; a.slot[s] != s in c, d, e and f;
  f  sentinels: nothing is written beyond counts[k], beyond cap, or into an idle slot's plane.
The cascades are chan_ref.CASCADES; tests/test_chan_ref.py anchors model and table without a GPU."""
import math

import numpy as np
import pytest

import chan_ref as R
from oracle import oracle
from rtl_sdr_scanner_cpp_amd.channelizer import Channelizer

pytestmark = pytest.mark.gpu

CALL = 1 << 16
# Rotated slots: three phase evaluations (P0, T[tid], T[u * TPB]), each at most 2^-25 revolution of argument rounding plus
# 2 ulp of sincospif (<= 3.1e-7 rad), two table products and the rotation at 1.7e-7 each: 1.5e-6, rounded up.
P_ROT = 2e-6
# The engine forms the oracle's fp32 products in another order (33 sequential FMAs and a log2 D tree against 33 D sequential
# terms), so it should sit at or below the oracle's floor e0; 2 covers the spread of a maximum over ~1e4 outputs.
# Measured on an MI355X, largest e_gpu / e0 over the rows and the four shifts of c (largest RMS ratio in brackets):
#   <3,1> 1.02 (1.29) at (1,1), 0.62 at (1,3), 0.27 at (1,8), 0.62 feeding a second stage;  <4,1> 0.40 (0.54);
#   <5,1> 0.26 (0.40);  <6,1> 0.17 (0.33) single stage, 0.77 (0.78) at (1,40),(1,48) over its 157 outputs;
#   <6,2> four waves 0.17 (0.28), two waves 0.13 (0.22);  generic 0.63 (0.90).
# No form needs a margin of its own. The RMS error is held to MARGIN * the oracle's RMS error with no allowance for the rotator.
MARGIN = 2.0


def _context(row, channels, max_samples=CALL):
    """A context for a row of the table, having checked that it takes the stages, the first-stage form and the wave count
    the table says (so every form is reached, not assumed)."""
    fs, bw, thr, stages, form = row
    ch = Channelizer(fs, bw, threshold=thr, channels=channels, max_samples=max_samples)
    assert [(i, d) for i, d, _ in ch.stages] == stages
    fst = R.first_stage(ch.stages)
    assert fst.form == form and fst.waves == R.WAVES.get(stages[0][1], 4)
    for s, (i, d, _n) in enumerate(ch.stages):
        np.testing.assert_array_equal(ch.stage_taps(s), oracle.design_taps(i, d))
    return ch, fst


def _model(ch, fs):
    return R.SlotModel(fs, ch.stages, [ch.stage_taps(s) for s in range(len(ch.stages))])


def _row(fs, bw):
    return next(r for r in R.CASCADES if r[0] == fs and r[1] == bw and r[2] == 125)


# ---------------------------------------------------------------------------------------------------------------------------
# a, b: impulse trains
# ---------------------------------------------------------------------------------------------------------------------------
SINGLE = [r for r in R.CASCADES if len(r[3]) == 1]  # (1,131) and (2,125) included: the generic kernel's partial sums add zeros


def _impulse_case(interp, decim, ntaps):
    """The stream, its impulse positions and the call sizes: short calls at the start (zero history) and in mid-stream (live
    history), a call that ends just behind an impulse, full calls, a ragged end."""
    nt = (ntaps + interp - 1) // interp
    spacing = R.impulse_spacing(ntaps, decim)
    n_imp = max(decim, 8, -(-(3 * CALL) // spacing))
    x, pos = R.impulse_train(n_imp, spacing, first=5)
    n = len(x)
    short = [c for c in (1, 7, decim - 1, decim, decim + 1) if c > 0]
    sizes = list(short)
    at = sum(sizes)
    j = int(np.searchsorted(pos, at + 20_000))
    end = int(pos[j]) + max(1, nt // 3)  # the impulse lies in the last nt samples: its response spills into the next call
    sizes.append(end - at)
    sizes += [CALL] + short
    at = sum(sizes)
    while n - at > CALL:
        sizes.append(CALL)
        at += CALL
    if n > at:
        sizes.append(n - at)
    assert sum(sizes) == n and max(sizes) <= CALL
    return x, pos, sizes, nt


def _check_coverage(pos, sizes, nt, interp, decim, tile, hit):
    """The stream really contains what the cases are about (stated, not assumed)."""
    ends = np.cumsum(sizes)
    starts = ends - np.asarray(sizes)
    assert len(set(int(p) % decim for p in pos)) == decim  # every branch residue
    assert len(pos) >= max(decim, 8)
    for c in (1, 7, decim - 1, decim, decim + 1):
        assert c <= 0 or (c in sizes and c < nt)  # shorter than the filter
    spills = [bool(np.any((pos >= e - nt) & (pos < e))) for e in ends[:-1]]
    assert any(spills)
    first3 = interior = ragged = False
    for a, b, size in zip(starts, ends, sizes):
        o0, o1 = R.produced(int(a), interp, decim), R.produced(int(b), interp, decim)
        ntiles = -(-(o1 - o0) // tile)
        if size == CALL:
            assert ntiles >= 6
        if ntiles < 5:
            continue
        t = lambda k: bool(hit[o0 + k * tile:min(o0 + (k + 1) * tile, o1)].any())  # noqa: E731
        first3 |= t(0) and t(1) and t(2)
        interior |= any(t(k) for k in range(3, ntiles - 1))
        ragged |= (o1 - o0) % tile != 0 and t(ntiles - 1)
    assert first3 and interior and ragged


def _run(ch, x, sizes, slots):
    got = {k: ([], []) for k in slots}
    at = 0
    for size in sizes:
        out = ch.process(x[at:at + size])
        assert sorted(out) == sorted(slots)  # idle slots report nothing
        for k in slots:
            got[k][0].append(out[k][0])
            got[k][1].append(out[k][1])
        at += size
    assert at == len(x)
    return {k: (np.concatenate(v[0]), np.concatenate(v[1])) for k, v in got.items()}


@pytest.mark.parametrize("row", SINGLE, ids=R.cascade_id)
def test_impulse_response_is_the_taps_bit_for_bit(row):
    ch, fst = _context(row, channels=3)
    interp, decim, ntaps = ch.stages[0]
    taps = ch.stage_taps(0)
    x, pos, sizes, nt = _impulse_case(interp, decim, ntaps)
    want, hit = R.impulse_response_exact(pos, len(x), interp, decim, taps)
    _check_coverage(pos, sizes, nt, interp, decim, fst.tile, hit)
    assert np.unique(R.impulse_hits(pos, len(x), interp, decim, ntaps)[1]).size == ntaps  # every tap of every branch is seen
    ch.start(1, 0)  # slots 0 and 2 idle
    g8, gy = _run(ch, x, sizes, [1])[1]
    ch.close()
    assert len(gy) == len(want)
    bad = np.flatnonzero(gy.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (len(bad), bad[:8], gy[bad[:8]], want[bad[:8]])
    assert gy.tobytes() == want.tobytes()
    assert not gy[~hit].view(np.uint64).any()  # exact +0 outside the responses
    assert g8.tobytes() == R.to_i8(want).tobytes()
    assert np.abs(g8).max() > 0


@pytest.mark.parametrize("row", SINGLE, ids=R.cascade_id)
def test_impulse_response_under_rotation(row):
    fs = row[0]
    ch, fst = _context(row, channels=3)
    interp, decim, ntaps = ch.stages[0]
    taps = ch.stage_taps(0)
    x, pos, sizes, _nt = _impulse_case(interp, decim, ntaps)
    shifts = {1: int(fs / 7), 2: -int(fs / 5)}  # slot 0 idle
    models = {}
    for k, sh in shifts.items():
        ch.start(k, sh)
        models[k] = _model(ch, fs)
        models[k].start(sh)
    at = 0
    for size in sizes:  # the model's phase is kept call by call, as the engine keeps f0
        for m in models.values():
            m.feed(x[at:at + size])
        at += size
    got = _run(ch, x, sizes, [1, 2])
    ch.close()
    worst = 0.0
    for k in shifts:
        assert abs(models[k].df) * 2 * math.pi > 1e-3  # what a slip of one sample would show as
        want, hit = R.impulse_response_rotated(pos, len(x), interp, decim, taps, models[k].phase())
        gy = got[k][1].astype(np.complex128)
        assert len(gy) == len(want)
        assert not np.any(gy[~hit] != 0)
        mag = np.abs(want[hit])
        rel = np.abs(gy[hit] - want[hit])[mag > 0] / mag[mag > 0]
        worst = max(worst, float(rel.max()))
        assert np.all(gy[hit][mag == 0] == 0)
        r = got[k][1].view(np.float32).reshape(-1, 2) * np.float32(127.0)
        np.testing.assert_array_equal(got[k][0], np.clip(np.rint(r), -128, 127).astype(np.int8))
    print(f"CHANFIG b {R.cascade_id(row)} {fst.form} waves {fst.waves}: max relative error {worst:.3g}")
    assert worst <= P_ROT


# ---------------------------------------------------------------------------------------------------------------------------
# c, d, e: noise and carriers against the model, bound margin * e0 + p
# ---------------------------------------------------------------------------------------------------------------------------
N_NOISE = 300_000
_noise_cache = {}


def _stream(n, fs, bw, seed=1):
    """The CPU test's noise (0.2 sigma complex) plus two carriers that the slots on fs/7 and -fs/5 pull into their passband."""
    if seed not in _noise_cache:
        rng = np.random.default_rng(seed)
        z = (rng.standard_normal(N_NOISE) + 1j * rng.standard_normal(N_NOISE)) * 0.2
        z.setflags(write=False)
        _noise_cache[seed] = z
    t = np.arange(n, dtype=np.float64)
    x = _noise_cache[seed][:n].copy()
    for k, f in enumerate((int(fs / 7) + bw / 8.0, -int(fs / 5) - bw / 10.0)):
        x += 0.15 * np.exp(2j * np.pi * ((f / fs) * t + 0.1 * k))
    return x.astype(np.complex64)


def _floor(row, ch, recorded):
    """The oracle's fp32 floor on these samples: shift 0 through oracle and model. Returns (e0, rms0), both relative to
    the model's maximum."""
    fs, bw, thr = row[:3]
    o = oracle.ChannelizerOracle(fs, bw, thr)
    o.set_shift(0)
    m = _model(ch, fs)
    ys = []
    for part in recorded:
        ys.append(o.process(part)[0])
        m.feed(part)
    y, ref = np.concatenate(ys), m.output()
    assert len(y) == len(ref)
    scale = np.abs(ref).max()
    err = np.abs(y - ref)
    return float(err.max() / scale), float(np.sqrt(np.mean(err ** 2)) / scale)


def _hold(tag, got, model, e0, rms0, rotated):
    """got (complex64) against the model's output with the bound of c; prints the figures first."""
    ref = model.output()
    assert len(got) == len(ref), (tag, len(got), len(ref))
    scale = np.abs(ref).max()
    err = np.abs(got.astype(np.complex128) - ref)
    e, rms = float(err.max() / scale), float(np.sqrt(np.mean(err ** 2)) / scale)
    p = P_ROT if rotated else 0.0
    print(f"CHANFIG {tag}: e_gpu {e:.3g} e0 {e0:.3g} ratio {e / e0:.3g} | rms_gpu {rms:.3g} rms0 {rms0:.3g} ratio {rms / rms0:.3g} | p {p:g}")
    return e <= MARGIN * e0 + p and rms <= MARGIN * rms0, (tag, e, e0, rms, rms0)


@pytest.mark.parametrize("row", R.CASCADES, ids=R.cascade_id)
def test_noise_against_the_model_nothing_fitted(row):
    fs, bw = row[:2]
    ch, fst = _context(row, channels=6)
    x = _stream(N_NOISE, fs, bw)
    shifts = {1: 0, 2: int(fs / 7), 4: -int(fs / 5), 5: fs // 2}  # slots 0 and 3 idle: a.slot[s] != s for every s
    models = {}
    for k, sh in shifts.items():
        ch.start(k, sh)
        models[k] = _model(ch, fs)
        models[k].start(sh)
    sizes = [1, 7, CALL, 40_001, CALL, 3, CALL, 12_345]
    sizes.append(N_NOISE - sum(sizes))
    at, parts = 0, []
    for size in sizes:
        parts.append(x[at:at + size])
        for m in models.values():
            m.feed(parts[-1])
        at += size
    got = _run(ch, x, sizes, list(shifts))
    e0, rms0 = _floor(row, ch, parts)
    ch.close()
    assert e0 <= 3e-6
    results = []
    for k, sh in shifts.items():
        gy = got[k][1]
        results.append(_hold(f"c {R.cascade_id(row)} {fst.form} waves {fst.waves} slot {k} shift {sh}", gy, models[k], e0, rms0,
                             rotated=sh not in (0, fs // 2)))
        np.testing.assert_array_equal(got[k][0], R.to_i8(gy))
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]


SESSIONS = [(2_048_000, 32_000), (1_024_000, 32_000), (2_000_000, 20_000), (1_024_000, 20_000)]  # (1,64) (1,32) (1,100) (1,16),(5,16)


@pytest.mark.parametrize("fs,bw", SESSIONS)
def test_sessions_against_the_model_nothing_fitted(fs, bw):
    """Start on shift a, three calls, stop, two idle calls, start on shift b, three calls: phase and histories carry over the
    gap, the increment changes at the restart, and the model is fed exactly the recorded samples."""
    row = (fs, bw, 125, oracle.resampler_factors(fs, bw), None)
    ch = Channelizer(fs, bw, channels=2, max_samples=CALL)
    assert [(i, d) for i, d, _ in ch.stages] == row[3]
    fst = R.first_stage(ch.stages)
    assert fst.form == {64: "<6,1>", 32: "<5,1>", 100: "<6,2>", 16: "<4,1>"}[ch.stages[0][1]]
    sizes = [30_001, CALL, 17, 5_000, 33_333, CALL, 1, 41_234]
    x = _stream(sum(sizes), fs, bw, seed=2)
    model = _model(ch, fs)
    got, parts, at = [], [], 0
    for c, size in enumerate(sizes):
        if c == 0:
            ch.start(1, int(fs / 7))
            model.start(int(fs / 7))
        if c == 3:
            ch.stop(1)
        if c == 5:
            ch.start(1, -int(fs / 5))
            model.start(-int(fs / 5))
        out = ch.process(x[at:at + size])
        if 3 <= c < 5:
            assert out == {} and not ch.is_recording(1)
        else:
            assert list(out) == [1]
            got.append(out[1][1])
            parts.append(x[at:at + size])
            model.feed(parts[-1])
        at += size
    e0, rms0 = _floor(row, ch, parts)
    ch.close()
    ok, info = _hold(f"d {fs}-{bw} {fst.form} waves {fst.waves}", np.concatenate(got), model, e0, rms0, rotated=True)
    assert ok, info


@pytest.mark.parametrize("fs,bw", [(2_048_000, 32_000), (250_000, 25_000)])  # (1,64), (1,10)
def test_sixteen_slots(fs, bw):
    """SC_MAX_CHANNELS slots, fourteen recording on distinct shifts, slots 0 and 9 idle: every slot against its own model."""
    row = _row(fs, bw)
    ch, fst = _context(row, channels=16)
    sizes = [CALL, 50_001]
    x = _stream(sum(sizes), fs, bw, seed=3)
    slots = [k for k in range(16) if k not in (0, 9)]
    shifts = {k: int(fs * (k - 7.5) / 16.3) for k in slots}
    assert len(set(shifts.values())) == 14 and 0 not in shifts.values()
    models = {}
    for k in slots:
        ch.start(k, shifts[k])
        models[k] = _model(ch, fs)
        models[k].start(shifts[k])
    parts = [x[:sizes[0]], x[sizes[0]:]]
    for m in models.values():
        for part in parts:
            m.feed(part)
    got = _run(ch, x, sizes, slots)
    e0, rms0 = _floor(row, ch, parts)
    ch.close()
    results = [_hold(f"e {fs}-{bw} {fst.form} slot {k} shift {shifts[k]}", got[k][1], models[k], e0, rms0, rotated=True) for k in slots]
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]


# ---------------------------------------------------------------------------------------------------------------------------
# f: nothing written out of place
# ---------------------------------------------------------------------------------------------------------------------------
I8_SENTINEL = 0x5A
F32_SENTINEL = 0x7FC05A5A  # a quiet NaN with a payload
GUARD = 4096


class _Planes:
    """Output planes for `channels` slots of `cap` samples and a guard region behind each, all filled with sentinels."""

    def __init__(self, torch, dev, channels, cap):
        self.channels, self.cap = channels, cap
        self.i8 = torch.full((channels * cap * 2 + GUARD,), I8_SENTINEL, dtype=torch.int8, device=dev)
        self.f32 = torch.full((channels * cap * 2 + GUARD,), F32_SENTINEL, dtype=torch.int32, device=dev)

    def host(self):
        """(int8 [channels, cap, 2], uint32 [channels, cap, 2], int8 guard, uint32 guard)"""
        n = self.channels * self.cap * 2
        i8 = self.i8.cpu().numpy()
        f32 = self.f32.cpu().numpy().view(np.uint32)
        return i8[:n].reshape(self.channels, self.cap, 2), f32[:n].reshape(self.channels, self.cap, 2), i8[n:], f32[n:]


@pytest.mark.parametrize("fs,bw,thr", [(2_048_000, 32_000, 125), (2_032_000, 16_000, 125), (2_048_000, 16_000, 125)])  # (1,64) (1,127) (1,8),(1,16)
def test_nothing_is_written_out_of_place(fs, bw, thr):
    import torch
    row = next(r for r in R.CASCADES if r[:3] == (fs, bw, thr))
    dev = torch.device("cuda:0")
    n1, n2 = 30_001, 70_000
    x = _stream(n1 + n2, fs, bw, seed=4)
    d_iq = torch.from_numpy(x.view(np.float32).copy()).to(dev)
    recording, idle = {1: int(fs / 7), 3: -int(fs / 5)}, (0, 2)

    def run(cap_of):
        ch, _fst = _context(row, channels=4, max_samples=n2)
        for k, sh in recording.items():
            ch.start(k, sh)
        warm = _Planes(torch, dev, 4, ch.output_capacity(n1))
        torch.cuda.synchronize()  # torch's fills run on torch's stream, the library writes from its own
        c1 = ch.process_device(d_iq, n1, warm.i8, warm.f32.view(torch.float32), warm.cap)
        ch.sync()
        cap = cap_of(ch, c1)
        planes = _Planes(torch, dev, 4, cap)
        torch.cuda.synchronize()
        counts = ch.process_device(d_iq[2 * n1:], n2, planes.i8, planes.f32.view(torch.float32), cap)
        ch.sync()
        ch.close()
        return counts, planes

    counts, full = run(lambda ch, c1: ch.output_capacity(n2))
    i8, f32, g8, g32 = full.host()
    assert counts[1] == counts[3] > 100 and counts[0] == counts[2] == 0 and counts[1] <= full.cap
    for k in recording:
        assert np.all(i8[k, counts[k]:] == I8_SENTINEL) and np.all(f32[k, counts[k]:] == F32_SENTINEL)
        assert not np.any(f32[k, :counts[k]] == F32_SENTINEL)  # and everything below counts[k] was written
    for k in idle:
        assert np.all(i8[k] == I8_SENTINEL) and np.all(f32[k] == F32_SENTINEL)
    assert np.all(g8 == I8_SENTINEL) and np.all(g32 == F32_SENTINEL)

    counts_half, half = run(lambda ch, c1: int(counts[1]) // 2)
    h8, h32, g8, g32 = half.host()
    cap = half.cap
    assert cap == counts[1] // 2 and list(counts_half) == list(counts)
    for k in recording:
        assert h8[k].tobytes() == i8[k, :cap].tobytes() and h32[k].tobytes() == f32[k, :cap].tobytes()
    for k in idle:
        assert np.all(h8[k] == I8_SENTINEL) and np.all(h32[k] == F32_SENTINEL)
    assert np.all(g8 == I8_SENTINEL) and np.all(g32 == F32_SENTINEL)
