"""Per-slot sample ranges in one channeliser call (sc_process_ranges / sc_process_ranges_device) on the GPU. Run with -m gpu.

The call is DEFINED by the older entry points: per channel, its ranges in order, each as sc_start(shift) / sc_process_device of
d_iq + begin, end - begin samples / sc_stop. So context A makes one ranges call per chunk, twin context B runs that sequence, and
every range must give B's bytes (int8 and cf32), counts and range_counts: for the six first-stage forms and the four input
formats, over three consecutive calls so that phase, histories and counters carry. Then sixteen channels, cap below a channel's
total with sentinel planes, every refusal (with the state proven untouched), the host-pointer form, and the fp64 slot model fed
only the ranges' samples with the bounds test_gpu_channelizer_fp64.py holds the same cascades to."""
import numpy as np
import pytest

import chan_ref as R
from oracle import oracle
from rtl_sdr_scanner_cpp_amd import abi as A
from rtl_sdr_scanner_cpp_amd.abi import SpecscanError
from rtl_sdr_scanner_cpp_amd.channelizer import SC_MAX_RANGES, Channelizer
from test_gpu_channelizer_fp64 import F32_SENTINEL, I8_SENTINEL, SESSIONS, _floor, _hold, _model, _Planes, _stream
from test_gpu_channelizer_int_iq import CASES, FORMATS, _ints, _to_cf32

pytestmark = pytest.mark.gpu

FORMS = CASES[:6]  # <6,1>, <3,1> two-stage, <4,1>, <5,1>, <6,2>, generic
CHUNKS = (40_000, 33_333, 25_001)  # three calls: every form has full tiles, edge tiles and a ragged last tile in the long ranges
NCH = 4


def _range_sets(stages, fs):
    """The three calls' range lists [(channel, shift, begin, end)]. D, nt: the first stage's decimation and taps per arm.
    Channel 0 never has a range (an idle channel in front of active ones); channels are interleaved in the lists."""
    i0, d, ntaps = stages[0]
    nt = (ntaps + i0 - 1) // i0
    a, a2, b, b2, c = int(fs / 7), -int(fs / 9), -int(fs / 5), int(fs / 11), 12_500
    n0, n1, n2 = CHUNKS
    p = 7 + nt - 2  # (nt is about 33 D at interpolation 1)
    assert nt - 2 >= 1 and p + 1_000 < n0 - 5 * 64 * d // i0 and 20_001 > 11 + 2 * d + 1 and 9_001 + nt - 2 <= n2
    return [
        [  # three ranges on channel 1 beside one each on 2 and 3: later rounds have fewer slots
            (1, a, 0, 1),  # from 0, length 1
            (3, c, 5_000, 25_001),
            (1, a, 7, 7 + nt - 2),  # odd begin, shorter than the history
            (2, b, 3, 3 + d - 1),  # D - 1
            (1, a, p + 1_000, n0),  # to nsamples
        ],
        [
            (2, b, 0, 12_345),
            (1, a, 11, 11 + d),  # D
            (1, a, 11 + d, 11 + 2 * d + 1),  # abuts, D + 1
            (3, c, 777, 777 + d + 1),
            (1, a2, 20_001, n1),  # retuned
        ],
        [
            (3, c, n2 - 1, n2),  # length 1, to nsamples
            (2, b, 1, 1 + d),
            (1, a2, 0, n2),  # the whole call
            (2, b2, 1 + d, 9_000),  # abuts and retunes
            (2, b2, 9_001, 9_001 + nt - 2),
            (3, c, n2, n2),  # empty: a no-op behind the range that ends there
        ],
    ]


def _dev_stream(torch, q):
    """The stream as a device tensor [n, 2] of its own dtype (CF32: float32)."""
    host = q.view(np.float32).reshape(-1, 2) if q.dtype == np.complex64 else q
    return torch.from_numpy(np.ascontiguousarray(host)).to("cuda:0")


def _twin(torch, ch, d_iq, ranges, cap):
    """The defining sequence on ch: ({channel: (int8 bytes, cf32 bytes)}, counts, range_counts)."""
    nch = ch.cfg.channels
    i8 = torch.zeros((nch, cap, 2), dtype=torch.int8, device="cuda:0")
    cf = torch.zeros((nch, cap, 2), dtype=torch.float32, device="cuda:0")
    out = {}
    counts, rc = np.zeros(nch, np.int64), []
    for k in sorted({r[0] for r in ranges}):
        out[k] = ([], [])
        for i, (chan, shift, begin, end) in enumerate(ranges):
            if chan != k:
                continue
            ch.start(k, shift)
            torch.cuda.synchronize()
            got = ch.process_device(d_iq[begin:], end - begin, i8, cf, cap)
            ch.sync()
            ch.stop(k)
            assert all(got[j] == 0 for j in range(nch) if j != k)
            out[k][0].append(i8[k, :got[k]].cpu().numpy().tobytes())
            out[k][1].append(cf[k, :got[k]].cpu().numpy().tobytes())
            counts[k] += got[k]
            rc.append((i, int(got[k])))
    return {k: (b"".join(v[0]), b"".join(v[1])) for k, v in out.items()}, counts, [n for _i, n in sorted(rc)]


def _ranges_call(torch, ch, d_iq, nsamples, ranges, cap):
    nch = ch.cfg.channels
    i8 = torch.zeros((nch, cap, 2), dtype=torch.int8, device="cuda:0")
    cf = torch.zeros((nch, cap, 2), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    counts, rc = ch.process_ranges_device(d_iq, nsamples, ranges, i8, cf, cap)
    ch.sync()
    assert not any(ch.is_recording(k) for k in range(nch))
    out = {k: (i8[k, :counts[k]].cpu().numpy().tobytes(), cf[k, :counts[k]].cpu().numpy().tobytes()) for k in sorted({r[0] for r in ranges})}
    return out, counts, list(rc)


def _compare(got, want, tag):
    (ga, gc, gr), (wa, wc, wr) = got, want
    assert list(gc) == list(wc) and gr == wr, (tag, list(gc), list(wc), gr, wr)
    assert sorted(ga) == sorted(wa), tag
    for k in ga:
        assert ga[k][0] == wa[k][0], (tag, k, "int8")
        assert ga[k][1] == wa[k][1], (tag, k, "cf32")


@pytest.mark.parametrize("name", ["cf32", "cs8", "cu8", "cs16"])
@pytest.mark.parametrize("fs,bw,stages,form", FORMS, ids=[c[3] + f"-{c[0]}-{c[1]}" for c in FORMS])
def test_ranges_equal_the_defining_sequence_bit_for_bit(fs, bw, stages, form, name):
    import torch
    n = sum(CHUNKS)
    q = _ints(n, fs, "cs16" if name == "cf32" else name, seed=fs // 1000 + bw // 1000)
    kw = {}
    if name == "cf32":
        q = _to_cf32(q, "cs16")
    else:
        kw = dict(in_format=FORMATS[name][0], int_scale=FORMATS[name][1])
    a = Channelizer(fs, bw, channels=NCH, max_samples=max(CHUNKS), **kw)
    b = Channelizer(fs, bw, channels=NCH, max_samples=max(CHUNKS), **kw)
    assert [(i, d) for i, d, _ in a.stages] == stages and R.first_stage(a.stages).form == form
    d_iq = _dev_stream(torch, q)
    cap = a.output_capacity(max(CHUNKS))
    pos, produced = 0, 0
    for size, ranges in zip(CHUNKS, _range_sets(a.stages, fs)):
        assert len(ranges) <= SC_MAX_RANGES and any(r[2] % 2 for r in ranges) and all(r[0] != 0 for r in ranges)
        chunk = d_iq[pos:pos + size]
        got = _ranges_call(torch, a, chunk, size, ranges, cap)
        want = _twin(torch, b, chunk, ranges, cap)
        _compare(got, want, (name, form, pos))
        assert got[1][0] == 0 and sum(got[2]) == sum(got[1])
        produced += int(sum(got[1]))
        pos += size
    assert produced > 500
    a.close()
    b.close()


def test_sixteen_channels_one_range_each():
    import torch
    fs, bw, n = 2_048_000, 32_000, 50_000
    x = _stream(n, fs, bw, seed=6)
    d_iq = _dev_stream(torch, x)
    a = Channelizer(fs, bw, channels=16, max_samples=n)
    b = Channelizer(fs, bw, channels=16, max_samples=n)
    cap = a.output_capacity(n)
    for call in range(2):
        ranges = [(k, int(fs * (k - 7.5) / 16.3), (37 * k + call) % 5_000, n - 1_000 * ((k + call) % 7) - k) for k in (5, 0, 15, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14)]
        got = _ranges_call(torch, a, d_iq, n, ranges, cap)
        _compare(got, _twin(torch, b, d_iq, ranges, cap), call)
        assert min(got[1]) > 600
    a.close()
    b.close()


def test_host_form_equals_device_form():
    import torch
    fs, bw, stages, _form = FORMS[1]
    n = CHUNKS[0]
    q = _ints(n, fs, "cs8", seed=9)
    h = Channelizer(fs, bw, in_format=A.SS_FMT_CS8, channels=NCH, max_samples=n)
    d = Channelizer(fs, bw, in_format=A.SS_FMT_CS8, channels=NCH, max_samples=n)
    d_iq = _dev_stream(torch, q)
    for ranges in _range_sets(h.stages, fs)[:2]:
        ranges = [r for r in ranges if r[3] <= n]
        out, rc = h.process_ranges(q, ranges)
        want, counts, wrc = _ranges_call(torch, d, d_iq, n, ranges, d.output_capacity(n))
        assert list(rc) == wrc and sorted(out) == sorted(want)
        for k in out:
            assert len(out[k][0]) == counts[k] and out[k][0].tobytes() == want[k][0] and out[k][1].tobytes() == want[k][1]
    h.close()
    d.close()


def test_cap_below_a_channels_total_and_nothing_out_of_place():
    """Planes of sentinels: with the full cap nothing beyond counts, in idle channels or behind the planes is written; with cap in
    the middle of channel 1's SECOND range (out0 + m < cap, not m < cap) the planes hold the first cap outputs and nothing else,
    and counts are still the true totals."""
    import torch
    fs, bw, n = 2_048_000, 32_000, 70_000
    x = _stream(n, fs, bw, seed=4)
    d_iq = _dev_stream(torch, x)
    ranges = [(1, int(fs / 7), 3, 20_000), (3, -int(fs / 5), 0, n), (1, int(fs / 7), 30_001, n)]

    def run(cap):
        ch = Channelizer(fs, bw, channels=4, max_samples=n)
        planes = _Planes(torch, "cuda:0", 4, cap or ch.output_capacity(n))
        torch.cuda.synchronize()
        counts, rc = ch.process_ranges_device(d_iq, n, ranges, planes.i8, planes.f32.view(torch.float32), planes.cap)
        ch.sync()
        ch.close()
        return counts, rc, planes

    counts, rc, full = run(0)
    i8, f32, g8, g32 = full.host()
    assert counts[0] == counts[2] == 0 and counts[1] == rc[0] + rc[2] and counts[3] == rc[1] and rc[0] > 300 and rc[2] > 600
    for k in (1, 3):
        assert np.all(i8[k, counts[k]:] == I8_SENTINEL) and np.all(f32[k, counts[k]:] == F32_SENTINEL)
        assert not np.any(f32[k, :counts[k]] == F32_SENTINEL)
    for k in (0, 2):
        assert np.all(i8[k] == I8_SENTINEL) and np.all(f32[k] == F32_SENTINEL)
    assert np.all(g8 == I8_SENTINEL) and np.all(g32 == F32_SENTINEL)

    cap = int(rc[0]) + int(rc[2]) // 2
    counts_cut, rc_cut, cut = run(cap)
    h8, h32, g8, g32 = cut.host()
    assert list(counts_cut) == list(counts) and list(rc_cut) == list(rc) and cap < counts[1] < counts[3]
    for k in (1, 3):
        assert h8[k].tobytes() == i8[k, :cap].tobytes() and h32[k].tobytes() == f32[k, :cap].tobytes()
    for k in (0, 2):
        assert np.all(h8[k] == I8_SENTINEL) and np.all(h32[k] == F32_SENTINEL)
    assert np.all(g8 == I8_SENTINEL) and np.all(g32 == F32_SENTINEL)


def test_refusals_change_nothing():
    import torch
    fs, bw, n = 1_024_000, 32_000, 30_000
    q = _ints(2 * n, fs, "cs16", seed=13)
    d_iq = _dev_stream(torch, q)
    a = Channelizer(fs, bw, in_format=A.SS_FMT_CS16, channels=3, max_samples=n)
    b = Channelizer(fs, bw, in_format=A.SS_FMT_CS16, channels=3, max_samples=n)
    cap = a.output_capacity(n)
    first = [(0, 100_000, 5, 9_999), (2, -200_000, 0, n), (0, 150_000, 10_000, 29_001)]
    _compare(_ranges_call(torch, a, d_iq[:n], n, first, cap), _twin(torch, b, d_iq[:n], first, cap), "first")
    i8 = torch.zeros((3, cap, 2), dtype=torch.int8, device="cuda:0")
    good = (1, 50_000, 0, n)
    refused = {
        "too many": [(1, 50_000, k, k + 1) for k in range(SC_MAX_RANGES + 1)],
        "channel -1": [good, (-1, 0, 0, 10)],
        "channel 3": [good, (3, 0, 0, 10)],
        "begin > end": [good, (0, 0, 11, 10)],
        "begin < 0": [good, (0, 0, -1, 10)],
        "end > nsamples": [good, (0, 0, 0, n + 1)],
        "overlap": [(0, 0, 0, 100), good, (0, 0, 99, 200)],
        "descending": [(0, 0, 500, 600), (0, 0, 0, 100)],
    }
    for what, ranges in refused.items():
        with pytest.raises(SpecscanError) as e:
            a.process_ranges_device(d_iq[:n], n, ranges, i8, None, cap)
        assert e.value.status == A.SS_ERR_INVALID, what
        with pytest.raises(SpecscanError) as e:  # the host form refuses the same lists
            a.process_ranges(q[:n], ranges)
        assert e.value.status == A.SS_ERR_INVALID, what
    with pytest.raises(SpecscanError) as e:
        a.process_ranges_device(d_iq[:n + 1], n + 1, [good], i8, None, cap)
    assert e.value.status == A.SS_ERR_BATCH
    with pytest.raises(SpecscanError) as e:
        a.process_ranges_device(d_iq.reshape(-1)[1:], n, [good], i8, None, cap)  # 2 bytes off the 4-byte sample
    assert e.value.status == A.SS_ERR_INVALID
    a.start(1, 77_000)  # the two ways of driving a context are not mixed
    with pytest.raises(SpecscanError) as e:
        a.process_ranges_device(d_iq[:n], n, [(0, 100_000, 0, n)], i8, None, cap)
    assert e.value.status == A.SS_ERR_INVALID and a.is_recording(1)
    a.stop(1)
    counts, rc = a.process_ranges_device(d_iq[:n], n, [], i8, None, cap)  # no ranges: a call that does nothing
    assert not counts.any() and len(rc) == 0
    second = [(2, -200_000, 1, 12_345), (0, 150_000, 0, n), (1, 50_000, 29_999, n), (2, 300_000, 12_345, n - 1)]
    _compare(_ranges_call(torch, a, d_iq[n:], n, second, cap), _twin(torch, b, d_iq[n:], second, cap), "second")
    a.close()
    b.close()


@pytest.mark.parametrize("fs,bw", SESSIONS)
def test_ranges_against_the_fp64_model(fs, bw):
    """The model is fed only the ranges' samples, start(shift) at each retune. Abutting ranges, a gap, a retune at an abutment and a
    retune behind a gap, over three calls: a merged call has no bit-for-bit twin, the model covers it."""
    row = (fs, bw, 125, oracle.resampler_factors(fs, bw), None)
    sizes = [50_001, 1 << 16, 41_234]
    ch = Channelizer(fs, bw, channels=2, max_samples=max(sizes))
    assert [(i, d) for i, d, _ in ch.stages] == row[3]
    fst = R.first_stage(ch.stages)
    d = ch.stages[0][1]
    a, b = int(fs / 7), -int(fs / 5)
    calls = [
        [(1, a, 0, 10_000), (1, a, 10_000, 10_000 + d + 1), (1, a, 10_001 + d, 30_001), (1, a, 33_333, sizes[0])],
        [(1, a, 1, 20_000), (1, b, 20_000, 40_000), (1, b, 40_007, sizes[1])],
        [(1, b, 0, 17), (1, a, 5_001, sizes[2])],
    ]
    x = _stream(sum(sizes), fs, bw, seed=2)
    model = _model(ch, fs)
    got, parts, at, shift = [], [], 0, None
    for size, ranges in zip(sizes, calls):
        out, rc = ch.process_ranges(x[at:at + size], ranges)
        assert list(out) == [1] and sum(rc) == len(out[1][1])
        got.append(out[1][1])
        for _k, sh, begin, end in ranges:
            if sh != shift:
                model.start(sh)
                shift = sh
            parts.append(x[at + begin:at + end])
            model.feed(parts[-1])
        at += size
    e0, rms0 = _floor(row, ch, parts)
    ch.close()
    ok, info = _hold(f"ranges {fs}-{bw} {fst.form} waves {fst.waves}", np.concatenate(got), model, e0, rms0, rotated=True)
    assert ok, info
