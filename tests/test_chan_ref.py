"""The fp64 slot model (tests/chan_ref.py) against the CPU oracle (oracle/channelizer_oracle.c), on every cascade of
chan_ref.CASCADES: the model is what tests/test_gpu_channelizer_fp64.py holds the HIP kernels to, so it is anchored here first,
without a GPU.
  * shift 0: the oracle's fp32 floor e0 against the model, per cascade, within the 3e-6 the oracle is already held to
    (test_channelizer_oracle.py::test_resampler_cascade_against_fp64_upfirdn);
  * shift fs/7: the oracle's rotator recurrence against the model's closed form, modulo its creep — whose slope is bounded at
    3e-9 rad per input sample, a tenth of what one fp32 ulp in the increment gives (2^-24 * 0.5 rad), so that the model's
    increment is the oracle's;
  * impulse trains at shift 0 through single-stage cascades: the oracle's every output is taps[k] * x0 bit for bit, which pins
    the impulse builder's indexing before it meets the GPU."""
import numpy as np
import pytest

import chan_ref as R
from oracle import oracle

N = 200_000


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.2).astype(np.complex64)


@pytest.fixture(scope="module")
def noise():
    x = _noise(N, 1)
    x.setflags(write=False)
    return x


def _pair(fs, bw, thr, shift):
    o = oracle.ChannelizerOracle(fs, bw, thr)
    o.set_shift(shift)
    m = R.SlotModel(fs, o.stages, [oracle.design_taps(i, d) for i, d, _ in o.stages])
    m.start(shift)
    return o, m


@pytest.mark.parametrize("row", R.CASCADES, ids=R.cascade_id)
def test_table_stages_and_first_stage_form(row):
    """The table states what sc_create does with each row: a change of the factor split or of the dispatch rule shows up here."""
    fs, bw, thr, stages, form = row
    got = oracle.ChannelizerOracle(fs, bw, thr).stages
    assert [(i, d) for i, d, _ in got] == stages
    assert oracle.resampler_factors(fs, bw, thr) == stages
    fst = R.first_stage(got)
    assert fst.form == form
    assert fst.waves == R.WAVES.get(stages[0][1], 4)
    assert got[0][2] <= 33 * stages[0][1] or form == "generic"


def test_first_stage_rule_over_every_decimation():
    """Form and wave count as a function of the decimation alone (GNU Radio's default design: ntaps = 32.8 D, made odd)."""
    for d in range(1, 140):
        ntaps = len(oracle.design_taps(1, d))
        fst = R.first_stage([(1, d, ntaps)])
        if d > 128:
            assert fst.form == "generic", d
            continue
        logg = 3 if d <= 8 else 4 if d <= 16 else 5 if d <= 32 else 6
        assert fst == (f"<{logg},{2 if d > 64 else 1}>", 4 if d <= 85 else 2, (4 if d <= 85 else 2) * (64 >> logg) * 16), d
        assert (fst.tile + 32) * d * 8 <= 64 * 1024


@pytest.mark.parametrize("row", R.CASCADES, ids=R.cascade_id)
def test_shift_0_floor_of_the_oracle(row, noise):
    fs, bw, thr, _stages, _form = row
    o, m = _pair(fs, bw, thr, 0)
    y, _ = o.process(noise)
    m.feed(noise)
    ref = m.output()
    assert len(y) == len(ref) >= N * bw // fs - 2
    e0 = float(np.abs(y - ref).max() / np.abs(ref).max())
    print(f"{R.cascade_id(row)}: e0 = {e0:.3g}")
    assert e0 <= 3e-6


@pytest.mark.parametrize("row", R.CASCADES, ids=R.cascade_id)
def test_shifted_oracle_follows_the_model_increment(row, noise):
    fs, bw, thr, _stages, _form = row
    shift = int(fs / 7)
    o, m = _pair(fs, bw, thr, shift)
    y, _ = o.process(noise)
    m.feed(noise)
    ref = m.output()
    assert len(y) == len(ref)
    resid, slope = R.decreep(y, ref, fs / bw)
    print(f"{R.cascade_id(row)}: residual {resid:.3g}, slope {slope:.3g} rad/sample")
    assert resid < 1.5e-4
    assert abs(slope) < 3e-9


def test_increment_is_the_c_library_s():
    """The increment must come from the C library's cosf / sinf / hypotf: an ulp in the increment is 3e-8 rad per sample, ten
    times the slope bound above. Shift 0 and fs/2 are exact: 0 and -1/2 revolution."""
    assert R.increment(2_048_000, 0) == 0.0
    assert abs(abs(R.increment(2_048_000, 1_024_000)) - 0.5) < 1e-7
    for fs in (2_400_000, 2_000_000, 1_000_000, 272_000):
        df = R.increment(fs, int(fs / 7))
        assert abs(df + int(fs / 7) / fs) < 2.0 ** -24  # the fp32 angle's rounding, in revolutions
        assert R.increment(fs, -int(fs / 7)) == -df


def test_model_phase_carries_over_a_restart():
    m = R.SlotModel(1_000_000, [(1, 1, 1)], [np.ones(1)])
    m.start(100_000)
    m.feed(np.ones(1000, np.complex64))
    d1 = m.df
    m.start(-250_000)
    m.feed(np.ones(10, np.complex64))
    phi = m.phase()
    assert len(phi) == 1010 and phi[0] == 0.0
    want = (1000 * d1 + np.arange(10) * m.df) % 1.0
    assert np.abs((phi[1000:] - want + 0.5) % 1.0 - 0.5).max() < 1e-12
    np.testing.assert_allclose(m.output(), np.exp(2j * np.pi * phi), atol=1e-12)


SINGLE = [r for r in R.CASCADES if len(r[3]) == 1 and r[3][0][0] == 1]


@pytest.mark.parametrize("row", SINGLE, ids=R.cascade_id)
def test_oracle_impulse_response_is_its_taps_bit_for_bit(row):
    fs, bw, thr, stages, _form = row
    d = stages[0][1]
    o, _ = _pair(fs, bw, thr, 0)
    taps = oracle.design_taps(1, d)
    s = R.impulse_spacing(len(taps), d)
    x, pos = R.impulse_train(max(d, 8), s, first=3)
    want, hit = R.impulse_response_exact(pos, len(x), 1, d, taps)
    parts, at = [], 0
    for size in (1, 7, d + 1, len(x) // 3, len(x)):  # a stream: the cut does not matter
        parts.append(o.process(x[at:at + size])[0])
        at += size
    got = np.concatenate(parts)
    assert len(got) == len(want)
    assert got.tobytes() == want.tobytes()
    per_impulse = np.bincount(R.impulse_hits(pos, len(x), 1, d, len(taps))[2])
    assert set(per_impulse) <= {32, 33} and per_impulse.max() == 33
    assert len(set(int(p) % d for p in pos)) == d  # every residue mod D
    assert hit.sum() == per_impulse.sum()


def test_impulse_indexing_with_interpolation():
    """(2,125): the tap index follows total % I; the oracle's outputs are still single products."""
    fs, bw = 1_000_000, 16_000
    o, _ = _pair(fs, bw, 125, 0)
    assert o.stages[0][:2] == (2, 125)
    taps = oracle.design_taps(2, 125)
    s = R.impulse_spacing(len(taps), 125)
    x, pos = R.impulse_train(125, s, first=1)
    want, hit = R.impulse_response_exact(pos, len(x), 2, 125, taps)
    got = o.process(x)[0]
    assert len(got) == len(want) and got.tobytes() == want.tobytes()
    m, k, _ = R.impulse_hits(pos, len(x), 2, 125, len(taps))
    assert set(k % 2) == {0, 1} and hit.sum() == len(m)
