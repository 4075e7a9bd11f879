"""SS_FLAG_FOLD_CS16: CS16 contexts of 65536 / 131072 points on the work-buffer-free radix-8 / radix-16 fold (csrc/fft65536_dif8.h,
FMT_CS16; csrc/fold_cs16_staging.h), on the GPU. Calls are ss_process_device calls that hand out no plane, the learning frames a call
of their own (it takes the four-step form on every engine), as in test_gpu_int8_scale.test_int8_scale_on_the_fold_matches_oracle.

The fold's arithmetic behind the conversion is the int8 fold's, operation for operation, and the format's scale rides on the table wt:
int8 samples shifted left by eight bits under 1/32768 = (1/128) / 256 give fp32 values that are the int8 run's times 256 — exactly, no
overflow or underflow at these magnitudes — until wt divides it out. So a flagged CS16 engine fed frames_cs8 << 8 equals a CS8 engine
fed frames_cs8 BIT FOR BIT: lists, candidate powers, noise ceiling, tile counters, and the riders' digests. (On the parent commit the
flag is ignored, CS16 takes the four-step form, and none of that holds.) Real 16-bit values are held to the oracle; 12-bit values
under 1/2048 to the same values shifted under the default scale; decimated items to compact frames; and a flag that cannot take
effect to the unflagged engine. Run with -m gpu."""
import functools

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from digest_ref import assert_digest_equal
from parity import check_all, dont_care_limit
from strided import strided_items
from test_gpu_cs16 import _same, _to_cf32

pytestmark = pytest.mark.gpu

A = pkg.abi
CENTER = 145_000_000
FOLD = A.SS_FLAG_FOLD_CS16
CS8, CS16, CF32 = A.SS_FMT_CS8, A.SS_FMT_CS16, A.SS_FMT_CF32
# n: sample rate, learning frames, frames, the calls behind the learning call — fewer than 8 frames, exactly 8, whole groups of eight plus
# a remainder (both branches of dif8_item), and a call longer than the 35-frame reach of the averager
VECTORS = {65536: (20_000_000, 6, 75, [25, 3, 8, 33]), 131072: (20_000_000, 21, 128, [32, 5, 8, 62])}
G = 128


def _band(n):
    fs, learn, nframes, _ = VECTORS[n]
    return pkg.synth.SyntheticBand(n, seed=46, on_frame=learn + 24, off_frame=nframes - 12)


@functools.lru_cache(maxsize=None)
def _frames_cs8(n):
    v = _band(n).frames_cs8(VECTORS[n][2])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _frames_cs8_shifted(n):
    v = (_frames_cs8(n).astype(np.int16) << 8).astype(np.int16)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _frames_cs16(n):
    v = _band(n).frames_cs16(VECTORS[n][2])
    v.setflags(write=False)
    return v


def _cuts(n):
    _, learn, nframes, calls = VECTORS[n]
    cuts = np.concatenate([[0, learn], learn + np.cumsum(calls)]).astype(int)
    assert cuts[-1] == nframes
    return list(zip(cuts[:-1], cuts[1:]))


def _engine(n, fmt, max_batch, **cfg):
    fs, learn, _, _ = VECTORS.get(n, (n * 250, 6, 0, None))
    return pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=cfg.pop("decim", 1), learn_frames=learn, max_batch=max_batch, in_format=fmt, **cfg)


def _device_calls(eng, frames, cuts, cap_per_frame=2048):
    """The calls [a, b) of `cuts` as ss_process_device calls with no plane handed out, one ss_sync behind them all. `frames`: the items
    as the engine's format and decimation want them. Returns one dict of numpy arrays per call."""
    import torch
    dev = torch.device("cuda", 0)
    d_iq = [torch.from_numpy(np.array(frames[a:b])).to(dev) for a, b in cuts]  # (a copy: the cached vectors are read-only)
    outs = [dict(off=torch.zeros(b - a + 1, dtype=torch.int32, device=dev), idx=torch.empty((b - a) * cap_per_frame, dtype=torch.int32, device=dev),
                 avg=torch.empty((b - a) * cap_per_frame, dtype=torch.float32, device=dev)) for a, b in cuts]
    torch.cuda.synchronize()  # (torch's fills run on torch's stream, the library writes from its own)
    for d, o in zip(d_iq, outs):
        eng.process_device(d, d.shape[0], cand_off=o["off"], cand_idx=o["idx"], cand_avg=o["avg"])
    eng.sync()
    res = []
    for o in outs:
        off = o["off"].cpu().numpy()
        assert off[-1] <= o["idx"].numel(), "the lists' capacity"
        res.append({"cand_off": off, "cand_idx": o["idx"].cpu().numpy()[:off[-1]], "cand_avg": o["avg"].cpu().numpy()[:off[-1]]})
    return res


def _same_calls(tag, got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for key in ("cand_off", "cand_idx", "cand_avg"):
            _same(f"{tag}: call {k} {key}", g[key], w[key])
    return sum(int(g["cand_off"][-1]) for g in got)


def _same_state(tag, a, b):
    ta, ra = a.read_noise()
    tb, rb = b.read_noise()
    assert ra and rb, tag
    _same(f"{tag}: noise ceiling", ta, tb)
    sa, sb = a.stats(), b.stats()
    for key in ("tiles_total", "tiles_tested", "tiles_culled"):
        assert sa[key] == sb[key], (tag, key, sa, sb)
    return sa, sb


def _cat(outs):
    res = {k: np.concatenate([o[k] for o in outs]) for k in ("cand_idx", "cand_avg")}
    res["cand_off"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(o["cand_off"]) for o in outs]))]).astype(np.int32)
    return res


@pytest.mark.parametrize("n", sorted(VECTORS))
def test_flagged_cs16_is_bit_identical_to_the_int8_fold(n):
    """1. frames_cs8 << 8 on a flagged CS16 engine against frames_cs8 on a CS8 engine, both at their default scales."""
    cuts = _cuts(n)
    max_batch = max(b - a for a, b in cuts)
    e16, e8 = _engine(n, CS16, max_batch, flags=FOLD), _engine(n, CS8, max_batch)
    got = _device_calls(e16, _frames_cs8_shifted(n), cuts)
    want = _device_calls(e8, _frames_cs8(n), cuts)
    ncand = _same_calls(f"{n} points", got, want)
    s16, s8 = _same_state(f"{n} points", e16, e8)
    print(f"\n[{n} points, cs8 << 8] {ncand} candidates; tiles {s16['tiles_total']}, tested {s16['tiles_tested']}, culled {s16['tiles_culled']}")
    assert ncand > 1000
    assert s16["fold"] and s8["fold"], (s16, s8)
    if n == 131072:  # (culling exists there only with the fold)
        assert s16["culling"] and s16["tiles_culled"] > 0, s16


@functools.lru_cache(maxsize=None)
def _oracle_lists(oracle_mod, n):
    fs, learn, nframes, _ = VECTORS[n]
    return oracle_mod.oracle_chain(fs, CENTER, fft_size=n, decim=1, learn_frames=learn, max_batch=nframes, in_format=CF32).process(_to_cf32(_frames_cs16(n)))


@pytest.mark.parametrize("n", sorted(VECTORS))
def test_flagged_cs16_matches_the_oracle_on_real_16_bit_values(oracle_mod, n):
    """2. frames_cs16 (low bytes in use, the full range reached) against the oracle fed the exact conversion. The plain-C oracle in
    chunks of 25 / 32 frames against itself in one piece: 65536 points 7338 reference candidates, 1 within +-1e-3 dB of the start
    level (limit 3); 131072 points 14576, 2 (limit 7)."""
    raw = _frames_cs16(n)
    low = float(np.mean((raw.view(np.uint16) & 0xff) != 0))
    print(f"\n[{n} points] {100 * low:.1f} % of the values have a non-zero low byte; range [{raw.min()}, {raw.max()}]")
    assert low > 0.98 and raw.min() == -32768 and raw.max() == 32767
    cuts = _cuts(n)
    max_batch = max(b - a for a, b in cuts)
    eng = _engine(n, CS16, max_batch, flags=FOLD)
    got = _device_calls(eng, raw, cuts)
    st = eng.stats()
    errs, ncand, ndc = check_all(_cat(got), _oracle_lists(oracle_mod, n))
    print(f"[{n} points, fold] {ncand} reference candidates, {ndc} inside the band (limit {dont_care_limit(ncand)}); tiles {st['tiles_total']}, tested {st['tiles_tested']}, culled {st['tiles_culled']}")
    assert ncand > 5000 and ndc <= dont_care_limit(ncand), (ncand, ndc)
    assert st["fold"], st
    if n == 131072:
        assert st["culling"] and st["tiles_culled"] > 0 and st["fold"], st
    plain = _engine(n, CS16, max_batch)
    _device_calls(plain, raw, cuts)
    sp = plain.stats()
    assert sp["fold"] is False, sp
    if n == 131072:
        assert sp["culling"] is False, sp


def test_scale_rides_on_the_table():
    """3. Twelve-bit values under int_scale = 1/2048 against the same values shifted left by four bits under the default 1/32768."""
    n = 65536
    cuts = _cuts(n)
    max_batch = max(b - a for a, b in cuts)
    v = (_frames_cs16(n) >> 4).astype(np.int16)
    assert np.abs(v.astype(np.int64)).max() <= 2048
    e12 = _engine(n, CS16, max_batch, flags=FOLD, int_scale=1.0 / 2048)
    e16 = _engine(n, CS16, max_batch, flags=FOLD)
    ncand = _same_calls("12 bit", _device_calls(e12, v, cuts), _device_calls(e16, (v << 4).astype(np.int16), cuts))
    s12, s16 = _same_state("12 bit", e12, e16)
    assert ncand > 1000 and s12["fold"] and s16["fold"]


def test_decimated_device_input():
    """4. Items of N * 2 samples, poison behind the first N (tests/strided.py), against the compact frames."""
    n = 65536
    cuts = _cuts(n)
    max_batch = max(b - a for a, b in cuts)
    raw = _frames_cs16(n)
    ed = _engine(n, CS16, max_batch, flags=FOLD, decim=2)
    ec = _engine(n, CS16, max_batch, flags=FOLD)
    ncand = _same_calls("decim 2", _device_calls(ed, strided_items(raw, 2, "cs16"), cuts), _device_calls(ec, raw, cuts))
    sd, sc = _same_state("decim 2", ed, ec)
    assert ncand > 1000 and sd["fold"] and sc["fold"]


def _rider_batches(n):
    """The `<< 8` vector in batches of at most 33 frames, the learning frames first."""
    return _cuts(n)


def test_sparse_digest_does_not_look_at_the_format():
    """5a. The synchronous sparse digest (st_create_sparse) of a flagged CS16 engine against the CS8 engine's, call by call; the keys
    are those of a host tracker driven by the CS8 engine's digests."""
    from test_gpu_track_digest_sparse import Runner, _tracker
    n = 65536
    cuts = _rider_batches(n)
    max_batch = max(b - a for a, b in cuts)
    e16, e8 = _engine(n, CS16, max_batch, flags=FOLD), _engine(n, CS8, max_batch)
    d16, d8 = (e.track_digest(G, max_watch=4096, sparse=True) for e in (e16, e8))
    r16, r8 = Runner(e16, True, 4096), Runner(e8, True, 4096)
    trk = _tracker(n, 8.0)
    t = (1_000 + 40 * np.arange(VECTORS[n][2])).astype(np.int64)
    watched = ncand = 0
    for k, (a, b) in enumerate(cuts):
        keys = trk.keys.copy()
        o8, i8, c8 = r8.batch(_frames_cs8(n)[a:b], t[a:b])
        o16, i16, c16 = r16.batch(_frames_cs8_shifted(n)[a:b], t[a:b])
        _same(f"batch {k} cand_avg", c16, c8)
        g8, g16 = d8.digest(o8, i8, keys), d16.digest(o16, i16, keys)
        assert_digest_equal(g16, g8, f"batch {k} [{a}, {b})")
        trk.process_batch_digest(t[a:b], g8)
        watched += g8["watch"].size
        ncand += i8.size
    assert d16.sparse_stats() == d8.sparse_stats(), (d16.sparse_stats(), d8.sparse_stats())
    assert ncand > 1000 and watched > 0 and d8.sparse_stats()["tiles_evaluated"] > 0
    assert e16.stats()["fold"] and e8.stats()["fold"]


def test_ring_feed_does_not_look_at_the_format():
    """5b. The same through feeds with Feed.track(..., sparse=True, ring=True) (stf_create_ring), two batches in flight, keys posted after
    every collect: stf_collect's digests and sparse_stats() equal."""
    from test_gpu_track_digest_sparse import _tracker
    n = 65536
    cuts = _rider_batches(n)
    max_batch = max(b - a for a, b in cuts)
    t = (1_000 + 40 * np.arange(VECTORS[n][2])).astype(np.int64)
    side = []
    for fmt, frames, flags in ((CS16, _frames_cs8_shifted(n), FOLD), (CS8, _frames_cs8(n), 0)):
        eng = _engine(n, fmt, max_batch, flags=flags)
        feed = eng.feed(depth=3, cand_cap=1 << 20)
        side.append(dict(eng=eng, feed=feed, trk=feed.track(G, max_watch=4096, sparse=True, ring=True), tracker=_tracker(n, 8.0), frames=frames))
    waiting, ncand, watched = [], 0, 0

    def collect_one():
        nonlocal ncand, watched
        a, b = waiting.pop(0)
        got = []
        for s in side:
            g = s["trk"].collect()
            g = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in g.items()}
            assert g["status"] == 0 and g["digest_status"] == 0 and g["nframes"] == b - a, (g["status"], g["digest_status"], g["nframes"])
            s["tracker"].process_batch_digest(t[a:b], g)
            s["trk"].post_keys(g["seq"], s["tracker"].keys)
            got.append(g)
        g16, g8 = got
        what = f"batch [{a}, {b})"
        assert g16["seq"] == g8["seq"] and g16["keys_seq"] == g8["keys_seq"], what
        assert_digest_equal(g16, g8, what)
        _same(f"{what} feed_cand_avg", g16["feed_cand_avg"], g8["feed_cand_avg"])
        np.testing.assert_array_equal(side[0]["tracker"].keys, side[1]["tracker"].keys, err_msg=what)
        ncand += g8["cand_idx"].size
        watched += g8["watch"].size

    for a, b in cuts:
        for s in side:
            buf = s["feed"].acquire()
            buf[:b - a] = s["frames"][a:b]
            s["feed"].submit(b - a)
        waiting.append((a, b))
        if len(waiting) > 2:
            collect_one()
    while waiting:
        collect_one()
    s16, s8 = (s["trk"].sparse_stats() for s in side)
    print(f"\n[ring feed] {ncand} candidates, {watched} watched columns, sparse_stats {s8}")
    assert s16 == s8, (s16, s8)
    assert ncand > 1000 and watched > 0 and s8["tiles_evaluated"] > 0
    assert side[0]["eng"].stats()["fold"] and side[1]["eng"].stats()["fold"]
    for s in side:
        s["trk"].close()
        s["feed"].close()


@pytest.mark.parametrize("name,n,fmt,flags", [("cs16 at 8192 points", 8192, CS16, 0), ("cs16 keeping planes", 65536, CS16, A.SS_FLAG_KEEP_PLANES), ("cf32", 65536, CF32, 0)])
def test_flag_without_effect(name, n, fmt, flags):
    """6. Contexts that cannot fold: ss_create takes the flag, and the engine behaves as the unflagged one — same bits over one short
    session, fold == False."""
    learn, calls = 6, [12, 3, 17]
    nframes = learn + sum(calls)
    band = pkg.synth.SyntheticBand(n, seed=46, on_frame=learn + 4, off_frame=nframes - 3)
    raw = band.frames_cs16(nframes) if fmt == CS16 else np.ascontiguousarray(band.frames_cf32(nframes).view(np.float32).reshape(nframes, n, 2))
    cuts = np.concatenate([[0, learn], learn + np.cumsum(calls)]).astype(int)
    cuts = list(zip(cuts[:-1], cuts[1:]))
    kw = dict(fft_size=n, decim=1, learn_frames=learn, max_batch=max(calls), in_format=fmt)
    flagged = pkg.SpectrumEngine(n * 250, CENTER, flags=flags | FOLD, **kw)
    plain = pkg.SpectrumEngine(n * 250, CENTER, flags=flags, **kw)
    ncand = _same_calls(name, _device_calls(flagged, raw, cuts, cap_per_frame=4096), _device_calls(plain, raw, cuts, cap_per_frame=4096))
    sf, sp = _same_state(name, flagged, plain)
    assert ncand > 50, ncand
    assert sf["fold"] is False and sp["fold"] is False and sf["culling"] == sp["culling"], (sf, sp)
