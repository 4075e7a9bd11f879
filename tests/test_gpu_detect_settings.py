"""The detection settings on the product paths: candidate detection is `start_level <= avg && pass(i)` behind tile culling
(csrc/detect_fused.h: plan_tiles; csrc/plan_long.h: plan_long_run, plan_dif8_run, plan_x256_run), and start_level is a per-device user setting
(start_recording_level). Everything else that exercises culling runs at the default of 8 dB, where the synthetic band
separates cleanly — noise tiles 4 dB below the cut, comb tiles 14 dB above it. Here, on every culled path of the product library:

  (a) start levels — the stream's own straddle level (the median culling bound of its noise tiles, from the ORACLE's planes: half
      of the noise tiles dropped, half evaluated), 15 (between noise and combs), 22 with 20 dB combs (comb tiles live with few or
      no hits), 3 (nothing dropped), 8 + 2^-10 (no round float): culled == unculled bit for bit, and both equal the oracle's lists
      at that level outside the +-1e-3 dB band around it;
  (b) dense lists at -30 dB — every passing bin of every frame behind the warm-up: all eight 1024-entry pieces of every
      256-word trip of emit_span, every wide slice full — on the full band and on a part of it with ragged edges and an ignored
      range, host and device entry points;
  (c) list capacity where the emit stage is a role of a later call's launch: cand_cap inside a frame's list, at a frame
      boundary, total - 1 and total — offsets exact, the first cap entries right, nothing written behind cap, the calls after
      it right again;
  and start_level = -120, below the -100 of learning and warm-up frames: every passing bin of every frame, as the reference.

No number here comes from the engine: levels, expected lists and counts come from one oracle run per stream
(parity.lists_at_level, anchored against the oracle's own lists by tests/test_cull_bound_math.py). Needs an MI355X: run with -m gpu."""
import functools
import json
import os

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from parity import BAND, check_plane, dont_care_limit, lists_at_level, pass_mask, running_sum_drift_at, tile_bounds

pytestmark = pytest.mark.gpu

CENTER = 145_000_000
CF32, CS8 = "cf32", "cs8"
# one row per culled path of the product library. cuts: the calls (the learning frames a call of their own on the device paths,
# as the shipped forms want them); reach: what a tile's maximum M covers (plan_long.h: 256 bins and a 32-bin run on either side,
# or the whole neighbouring columns for the fold's per-column values); seed: chosen on the CPU so that the oracle's own avg plane
# holds at most dont_care_limit values inside the band around each level (asserted below; 0 .. 2 per level for these seeds, 9 of a
# limit of 15 at 3 dB on the deep 8192-point path; seeds 801, 805 and 806 had 8, 5 and 2 at 22 dB / the straddle level and were
# dropped). 2^20 points: two learning frames leave a low ceiling and noise tiles' bounds of 14.6 .. 37.8 dB; seed 811 is one whose
# stream has tiles below 15 dB at all (two of 8192, the lower at 14.61 dB; seeds 807, 812, 814 and 815 have none).
# Frame counts: about 100 (192 on the deep path, whose calls are 64 frames), 70 at 262144 points, 64 at 2^20.
PATHS = {
    "8192-cf32-host-calls": dict(n=8192, fs=2_048_000, fmt=CF32, entry="host", learn=17, cuts=[0, 20, 21, 128], reach="runs", seed=831),
    "8192-cf32-deep-device-calls": dict(n=8192, fs=2_048_000, fmt=CF32, entry="device", learn=24, cuts=[0, 64, 128, 192], reach="runs", seed=802),
    "65536-cs8-fold": dict(n=65536, fs=20_000_000, fmt=CS8, entry="device", learn=9, cuts=[0, 9, 25, 41, 57, 73, 89, 105], reach="columns", seed=803),
    "65536-cf32-one-launch": dict(n=65536, fs=20_000_000, fmt=CF32, entry="device", learn=9, cuts=[0, 9, 25, 41, 57, 73, 89, 105], reach="runs", seed=804),
    "131072-cs8": dict(n=131072, fs=20_000_000, fmt=CS8, entry="device", learn=9, cuts=[0, 9, 33, 57, 81, 105], reach="columns", seed=835),
    "262144-cf32": dict(n=1 << 18, fs=61_440_000, fmt=CF32, entry="device", learn=6, cuts=[0, 6, 22, 38, 54, 70], reach="runs", seed=826),
    "1048576-cs8": dict(n=1 << 20, fs=61_440_000, fmt=CS8, entry="device", learn=2, cuts=[0, 16, 32, 48, 64], reach="runs", seed=811),
}
LEVELS = {"straddle": None, "15": 15.0, "22": 22.0, "3": 3.0, "8+2^-10": 8.0 + 2.0 ** -10}
DENSE = -30.0
SENTINEL_IDX, SENTINEL_AVG = 0x5A5A5A5A, -12345.0
# tiles_total / tiles_tested / tiles_culled of the culling run of every (path, level) pair of (a), recorded from the commit before the long
# plans moved to csrc/plan_long.h (two runs on an MI355X, equal for every pair: integers out of fp32 sums in a fixed order). Culled ==
# unculled cannot see a plan that lists too much, and 0 < culled < tested cannot see one that is off by a few: equal counts can.
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_counts_parent.json")) as _fh:
    PLAN_COUNTS = json.load(_fh)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The path's stream (20 dB combs: 15 dB lies between noise and combs, 22 dB inside the combs' spread) and ONE oracle run of it at
    the default level: the avg plane — which does not depend on the level —, and the straddle level from its dB plane and ceiling."""
    from oracle import oracle as O
    s = PATHS[name]
    n, fs, learn, total = s["n"], s["fs"], s["learn"], s["cuts"][-1]
    band = pkg.synth.SyntheticBand(n, seed=s["seed"], rel_db=20.0, on_frame=learn + 24, off_frame=total - 7)
    raw = band.frames_cf32(total) if s["fmt"] == CF32 else band.frames_cs8(total)
    step = 16 if n >= (1 << 18) else total
    ch = O.oracle_chain(fs, CENTER, fft_size=n, decim=1, in_format=pkg.abi.SS_FMT_CF32 if s["fmt"] == CF32 else pkg.abi.SS_FMT_CS8, learn_frames=learn, max_batch=step)
    outs = [ch.process(raw[a:a + step], want=("psd", "avg")) for a in range(0, total, step)]
    avg = np.concatenate([o["avg"] for o in outs])
    bounds = tile_bounds(np.concatenate([o["psd"] for o in outs]), ch.read_noise()[0], learn, reach=s["reach"])
    ch.close()
    del outs
    cols = n // 256
    comb = np.zeros(cols, bool)
    for c in np.unique(np.concatenate(band.comb_bins) // 256):
        comb[max(c - 1, 0):c + 2] = True  # (a comb column's neighbours have it within reach)
    quiet = bounds[:, ~comb]
    straddle = float(np.float32(np.nanmedian(quiet)))
    return dict(raw=raw, avg=avg, straddle=straddle, quiet=(float(np.nanmin(quiet)), float(np.nanmax(quiet))), loud=float(np.nanmax(bounds)),
                bounds=np.sort(bounds[np.isfinite(bounds)]))


def _level(name, key):
    return _reference(name)["straddle"] if LEVELS[key] is None else LEVELS[key]


def _in_band(avg, level, passes):
    return int((np.abs(avg[:, passes] - np.float32(level)) < BAND).sum())


def _engine(name, level, flags=0, max_batch=None, **kw):
    s = PATHS[name]
    sizes = np.diff(s["cuts"])
    mb = int(max(sizes.max(), 64 if "deep" in name else 1)) if max_batch is None else max_batch
    return pkg.SpectrumEngine(s["fs"], CENTER, fft_size=s["n"], decim=1, in_format=pkg.abi.SS_FMT_CF32 if s["fmt"] == CF32 else pkg.abi.SS_FMT_CS8,
                              learn_frames=s["learn"], max_batch=mb, start_level=level, flags=flags, **kw)


def _host_calls(eng, raw, cuts):
    return [eng.process(raw[a:b], want=()) for a, b in zip(cuts[:-1], cuts[1:])]


def _device_calls(eng, raw, cuts, caps, views=None):
    """ss_process_device, one call per batch, nothing in between (stages of earlier calls ride on later launches). caps[k]: the
    length of call k's candidate buffers; views: {k: (idx tensor, avg tensor)} to hand call k instead (capacity tests)."""
    import torch
    dev = torch.device("cuda", 0)
    d_iq = [torch.from_numpy(raw[a:b].view(np.float32) if raw.dtype == np.complex64 else raw[a:b]).to(dev) for a, b in zip(cuts[:-1], cuts[1:])]
    outs = []
    for k, d in enumerate(d_iq):
        idx, avg = (views or {}).get(k) or (torch.full((max(int(caps[k]), 1),), SENTINEL_IDX, dtype=torch.int32, device=dev),
                                            torch.full((max(int(caps[k]), 1),), SENTINEL_AVG, dtype=torch.float32, device=dev))
        outs.append(dict(off=torch.zeros(d.shape[0] + 1, dtype=torch.int32, device=dev), idx=idx, avg=avg))
    torch.cuda.synchronize()
    for d, o in zip(d_iq, outs):
        eng.process_device(d, d.shape[0], cand_off=o["off"], cand_idx=o["idx"], cand_avg=o["avg"])  # (raises unless SS_OK)
    eng.sync()
    res = []
    for o in outs:
        off = o["off"].cpu().numpy()
        m = min(int(off[-1]), int(o["idx"].numel()))
        res.append({"cand_off": off, "cand_idx": o["idx"].cpu().numpy()[:m], "cand_avg": o["avg"].cpu().numpy()[:m]})
    return res


def _join(outs):
    counts = np.concatenate([np.diff(o["cand_off"]) for o in outs])
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.concatenate([o["cand_idx"] for o in outs]), np.concatenate([o["cand_avg"] for o in outs]))


def _keys(off, idx, n):
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off)) * n + idx


def _ascending(off, idx):
    first = np.zeros(len(idx), bool)
    first[off[:-1][np.diff(off) > 0]] = True
    return bool((np.diff(idx.astype(np.int64), prepend=-1)[~first] > 0).all())


def _call_caps(ref_off, cuts, slack):
    return [int(ref_off[b] - ref_off[a]) + slack for a, b in zip(cuts[:-1], cuts[1:])]


def _run(name, level, flags, ref_off, entry=None, slack=64, **kw):
    s = PATHS[name]
    eng = _engine(name, level, flags, **kw)
    raw = _reference(name)["raw"]
    if (entry or s["entry"]) == "host":
        outs = _host_calls(eng, raw, s["cuts"])
        assert all(o["status"] == pkg.abi.SS_OK for o in outs)
    else:
        outs = _device_calls(eng, raw, s["cuts"], _call_caps(ref_off, s["cuts"], slack))
    eng.sync()
    st = eng.stats()
    eng.close()
    return _join(outs), st


# ---- (a) start levels

def _levels_of(name):
    return ("straddle", "15") if name == "1048576-cs8" else tuple(LEVELS)


@pytest.mark.parametrize("name,key", [(p, k) for p in PATHS for k in _levels_of(p)])
def test_start_levels_culled_equal_unculled_and_the_oracle(name, key):
    s, ref = PATHS[name], _reference(name)
    n, level = s["n"], _level(name, key)
    passes = pass_mask(n, s["fs"], CENTER - s["fs"] // 2, CENTER + s["fs"] // 2)
    ref_off, ref_idx = lists_at_level(ref["avg"], level, passes)
    limit = dont_care_limit(len(ref_idx))
    assert _in_band(ref["avg"], level, passes) <= limit, "choose another seed: the oracle's own avg plane sits inside the band too often"
    (off, idx, avg), st = _run(name, level, 0, ref_off)
    (off_nc, idx_nc, avg_nc), st_nc = _run(name, level, pkg.abi.SS_FLAG_NO_CULL, ref_off)
    print(f"\n[{name}, level {key} = {level:.4f} dB] noise tiles' bounds {ref['quiet'][0]:.2f} .. {ref['quiet'][1]:.2f} dB, largest bound {ref['loud']:.2f}; "
          f"{len(ref_idx)} reference candidates; tiles {st['tiles_total']}, tested {st['tiles_tested']}, culled {st['tiles_culled']}, live {st['tiles_total'] - st['tiles_culled']}")
    np.testing.assert_array_equal(off, off_nc)
    np.testing.assert_array_equal(idx, idx_nc)
    np.testing.assert_array_equal(avg, avg_nc)
    assert st_nc["tiles_culled"] == 0
    assert {k: st[k] for k in ("tiles_total", "tiles_tested", "tiles_culled")} == PLAN_COUNTS[name][key]
    diff = np.setxor1d(_keys(off, idx, n), _keys(ref_off, ref_idx, n))
    outside = [(int(k // n), int(k % n)) for k in diff if not abs(ref["avg"][k // n, k % n] - np.float32(level)) < BAND]
    assert not outside, f"candidate sets differ outside the {BAND} dB band around {level}: {outside[:10]}"
    assert len(diff) <= limit, (len(diff), limit)
    assert _ascending(off, idx)
    if key in ("straddle", "15", "3", "8+2^-10"):
        assert len(ref_idx) > 1000, len(ref_idx)  # (22 dB over 20 dB combs: few or none, which is that level's point)
    if key == "straddle":
        assert ref["quiet"][0] < level < ref["quiet"][1]
        assert 0 < st["tiles_culled"] < st["tiles_tested"], st
    if key == "15":
        assert st["tiles_culled"] > 0, st
    if level < ref["bounds"][0] - 1.0:  # (level 3 everywhere) every tile's bound is a dB and more above the cut: nothing may be dropped
        assert st["tiles_culled"] == 0 and st["tiles_tested"] > 0, st
    assert key != "3" or level < ref["bounds"][0] - 1.0


def _session(chain, raw, cuts, fs, retune_at, reset_at, want):
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a in retune_at:  # away and back: the other centre's ceiling is learnt from scratch, the averager keeps its rows
            chain.set_frequency_range(CENTER + fs - fs // 2, CENTER + fs + fs // 2)
            outs.append(chain.process(raw[a:a + 30], want=want))
            chain.set_frequency_range(CENTER - fs // 2, CENTER + fs // 2)
        if a in reset_at:
            chain.reset()
        outs.append(chain.process(raw[a:b], want=want))
    return outs


@pytest.mark.parametrize("name,cuts,retune_at,reset_at", [("8192-cf32-host-calls", [0, 20, 21, 110, 150, 192], (110,), (150,)),
                                                        ("65536-cs8-fold", [0, 9, 41, 57, 73, 105], (57,), (73,))])
def test_a_retune_and_reset_session_at_the_straddle_level(name, cuts, retune_at, reset_at):
    """Away to another centre (its ceiling learnt from scratch, thr_tilemin with it) and back, then ss_reset: the oracle plays the
    same session once, its lists at the straddle level come from its avg planes."""
    from oracle import oracle as O
    s = PATHS[name]
    n, fs = s["n"], s["fs"]
    total = cuts[-1]
    band = pkg.synth.SyntheticBand(n, seed=s["seed"] + 50, rel_db=20.0, on_frame=s["learn"] + 24, off_frame=total - 7)
    raw = band.frames_cf32(total) if s["fmt"] == CF32 else band.frames_cs8(total)
    in_format = pkg.abi.SS_FMT_CF32 if s["fmt"] == CF32 else pkg.abi.SS_FMT_CS8
    level = _reference(name)["straddle"]
    mb = int(np.diff(cuts).max())
    orc = O.oracle_chain(fs, CENTER, fft_size=n, decim=1, in_format=in_format, learn_frames=s["learn"], max_batch=mb)
    ref_avg = np.concatenate([o["avg"] for o in _session(orc, raw, cuts, fs, retune_at, reset_at, ("avg",))])
    orc.close()
    passes = pass_mask(n, fs, CENTER - fs // 2, CENTER + fs // 2)
    ref_off, ref_idx = lists_at_level(ref_avg, level, passes)
    limit = dont_care_limit(len(ref_idx))
    assert _in_band(ref_avg, level, passes) <= limit
    res = {}
    for tag, flags in (("cull", 0), ("nocull", pkg.abi.SS_FLAG_NO_CULL)):
        eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, in_format=in_format, learn_frames=s["learn"], max_batch=mb, start_level=level, flags=flags)
        res[tag] = _join(_session(eng, raw, cuts, fs, retune_at, reset_at, ()))
        eng.sync()
        res[tag + " stats"] = eng.stats()
        eng.close()
    for a, b in zip(res["cull"], res["nocull"]):
        np.testing.assert_array_equal(a, b)
    off, idx, _ = res["cull"]
    diff = np.setxor1d(_keys(off, idx, n), _keys(ref_off, ref_idx, n))
    outside = [(int(k // n), int(k % n)) for k in diff if not abs(ref_avg[k // n, k % n] - np.float32(level)) < BAND]
    assert not outside, outside[:10]
    assert len(diff) <= limit and len(ref_idx) > 1000, (len(diff), len(ref_idx))
    st = res["cull stats"]
    print(f"\n[{name}, retune and reset at the straddle level {level:.4f}] {len(ref_idx)} reference candidates; tested {st['tiles_tested']}, culled {st['tiles_culled']}")
    assert 0 < st["tiles_culled"] < st["tiles_tested"], st


# ---- (b) dense lists

def _dense_cuts(name):
    """The dense sessions: the learning frames as a call of their own, ss_reset (what the scanner does on every retune), the rest.
    The averager then goes from its warm-up's -100 straight to windows of 21 real rows: no window mixes -100 rows with real ones,
    and no avg value comes anywhere near -30 (asserted) — with learning rows inside the window the means step through
    -31 .. -27 dB in 4 dB steps, and a handful of the band's bins land inside the +-1e-3 dB band. 2^20 points: 26 frames."""
    s = PATHS[name]
    total = 26 if name == "1048576-cs8" else s["cuts"][-1]
    return sorted({0, s["learn"], total} | {c for c in s["cuts"] if s["learn"] < c < total})


@functools.lru_cache(maxsize=None)
def _dense_reference(name):
    """The oracle's avg plane of the dense session (the level does not enter it)."""
    from oracle import oracle as O
    s = PATHS[name]
    cuts = _dense_cuts(name)
    raw = _reference(name)["raw"]
    ch = O.oracle_chain(s["fs"], CENTER, fft_size=s["n"], decim=1, in_format=pkg.abi.SS_FMT_CF32 if s["fmt"] == CF32 else pkg.abi.SS_FMT_CS8, learn_frames=s["learn"],
                        max_batch=int(np.diff(cuts).max()))
    rows = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a == s["learn"]:
            ch.reset()
        rows.append(ch.process(raw[a:b], want=("avg",))["avg"])
    ch.close()
    return np.concatenate(rows)


def _dense_calls(eng, name, entry, raw, cuts, ref_off):
    """Learning call, ss_reset, then the rest by the host or the device entry point."""
    learn = PATHS[name]["learn"]
    head = _host_calls(eng, raw, cuts[:2]) if entry == "host" else _device_calls(eng, raw, cuts[:2], [0])
    eng.reset()
    rest = cuts[1:]
    tail = _host_calls(eng, raw, rest) if entry == "host" else _device_calls(eng, raw, rest, _call_caps(ref_off, rest, 0))  # buffers sized from the oracle's totals
    assert cuts[1] == learn and all(o.get("status", pkg.abi.SS_OK) == pkg.abi.SS_OK for o in head + tail)
    return head + tail


def _dense_form(name, form):
    """(cuts, range / ignored keywords, pass mask) of a dense case."""
    s = PATHS[name]
    n, fs = s["n"], s["fs"]
    cuts = _dense_cuts(name)
    if form == "full band":
        return cuts, {}, pass_mask(n, fs, CENTER - fs // 2, CENTER + fs // 2)
    half = int(0.12155 * fs) + 7  # about a quarter of the band around its middle, edges on no 32-bin boundary
    lo, hi = CENTER - half, CENTER + half
    ignored = [CENTER + int(0.0101 * fs), CENTER + int(0.0237 * fs)]
    passes = pass_mask(n, fs, lo, hi, ignored)
    first, last = np.flatnonzero(passes)[[0, -1]]
    gap = np.flatnonzero(~passes[first:last + 1]) + first
    assert first % 32 and (last + 1) % 32 and gap.size and gap[0] % 32 and (gap[-1] + 1) % 32 and n // 5 < passes.sum() < n // 4
    return cuts, dict(range_lo=lo, range_hi=hi, ignored=ignored), passes


@pytest.mark.parametrize("form", ["full band", "ragged quarter with an ignored range"])
@pytest.mark.parametrize("name", list(PATHS))
def test_dense_lists_every_passing_bin_of_a_frame(name, form):
    s, ref = PATHS[name], _reference(name)
    n = s["n"]
    cuts, kw, passes = _dense_form(name, form)
    total = cuts[-1]
    ref_avg = _dense_reference(name)
    ref_off, ref_idx = lists_at_level(ref_avg, DENSE, passes)
    assert _in_band(ref_avg, DENSE, passes) == 0  # nothing for rounding to decide: the lists must be EQUAL
    assert int(np.diff(ref_off).max()) == int(passes.sum())  # a whole row of hits (N on the full band)
    frames = np.repeat(np.arange(total), np.diff(ref_off))
    want_avg = ref_avg[frames, ref_idx][None]
    drift = running_sum_drift_at(n, ref_avg, frames, ref_idx)[None]
    for entry in ("host", "device"):
        eng = _engine(name, DENSE, 0, **kw)
        outs = _dense_calls(eng, name, entry, ref["raw"], cuts, ref_off)
        eng.close()
        off, idx, avg = _join(outs)
        np.testing.assert_array_equal(off, ref_off, err_msg=f"{entry}: cand_off")
        assert int(np.diff(off).max()) == int(passes.sum())
        np.testing.assert_array_equal(idx, ref_idx, err_msg=f"{entry}: cand_idx")
        worst = check_plane(f"{entry}: cand_avg", avg[None], want_avg, floor=drift)
    print(f"\n[{name}, {form}, level {DENSE}] {len(ref_idx)} candidates, {int(passes.sum())} in the fullest frame; cand_avg max |err| {worst:.1e} dB")


# ---- (c) capacity

# (262144 points: the combs reach 15 dB in the fourth call of the stream's five: halves of it, so that two calls follow the short one)
CAP_CUTS = {"262144-cf32": [0, 6, 22, 38, 46, 54, 62, 70]}


def _untruncated(name, level, cuts):
    """The session with room in every call (buffers sized from the oracle's totals and a little more): what the short call's
    offsets and entries are held to. Its own lists are held to the oracle's by the tests above; here, their number."""
    s, ref = PATHS[name], _reference(name)
    passes = pass_mask(s["n"], s["fs"], CENTER - s["fs"] // 2, CENTER + s["fs"] // 2)
    orc_off, orc_idx = lists_at_level(ref["avg"], level, passes)
    eng = _engine(name, level)
    outs = _device_calls(eng, ref["raw"], cuts, _call_caps(orc_off, cuts, 64))
    eng.close()
    off, idx, _ = _join(outs)
    assert abs(len(idx) - len(orc_idx)) <= dont_care_limit(len(orc_idx)) and int(np.abs(off - orc_off).max()) <= dont_care_limit(len(orc_idx))
    return off, idx


@pytest.mark.parametrize("band", ["ordinary", "dense"])
@pytest.mark.parametrize("name", ["8192-cf32-deep-device-calls", "65536-cs8-fold", "262144-cf32"])
def test_list_capacity_where_emit_rides_on_a_later_launch(name, band):
    """One call of a session gets a cand_cap-long view of a larger sentinel-filled tensor. ss_process_device only enqueues: it
    returns SS_OK and cand_off tells (include/specscan.h); ss_process returns SS_ERR_CAND_OVERFLOW when the total exceeds cand_cap
    and SS_OK when it fits exactly. The calls after it have room and must be right: mask words, counts and list headers were left
    clean. Everything is held to the same session with room in every call."""
    import torch
    s, ref = PATHS[name], _reference(name)
    cuts, raw = CAP_CUTS.get(name, s["cuts"]), ref["raw"]
    level = DENSE if band == "dense" else 15.0
    ref_off, ref_idx = _untruncated(name, level, cuts)
    per_call = _call_caps(ref_off, cuts, 0)
    # the short call: the first with lists in two frames at least and two more calls behind it
    j = next(k for k in range(len(per_call) - 2) if (np.diff(ref_off[cuts[k]:cuts[k + 1] + 1]) > 3).sum() >= 2)
    a, b = cuts[j], cuts[j + 1]
    call_off = ref_off[a:b + 1] - ref_off[a]
    call_idx = ref_idx[ref_off[a]:ref_off[b]]
    total = int(call_off[-1])
    f_last = int(np.flatnonzero(np.diff(call_off) > 3)[-1])  # the call's last frame with a list
    inside = int(call_off[f_last]) + int(call_off[f_last + 1] - call_off[f_last]) // 2
    boundary = int(call_off[f_last])
    assert 0 < boundary < inside < total - 1 and boundary in call_off and inside not in call_off
    dev = torch.device("cuda", 0)
    for cap in (inside, boundary, total - 1, total):
        big_idx = torch.full((total + 4096,), SENTINEL_IDX, dtype=torch.int32, device=dev)
        big_avg = torch.full((total + 4096,), SENTINEL_AVG, dtype=torch.float32, device=dev)
        eng = _engine(name, level)
        outs = _device_calls(eng, raw, cuts, per_call, views={j: (big_idx[:cap], big_avg[:cap])})
        eng.close()
        off = _join(outs)[0]
        np.testing.assert_array_equal(off, ref_off, err_msg=f"cap {cap}: cand_off")  # exact, whatever fitted
        got_idx, got_avg = big_idx.cpu().numpy(), big_avg.cpu().numpy()
        np.testing.assert_array_equal(got_idx[:cap], call_idx[:cap], err_msg=f"cap {cap}: the first cap entries")
        assert (got_idx[cap:] == SENTINEL_IDX).all() and (got_avg[cap:] == np.float32(SENTINEL_AVG)).all(), f"cap {cap}: written behind cand_cap"
        assert not (got_avg[:cap] == np.float32(SENTINEL_AVG)).any(), f"cap {cap}: cand_avg not written up to cand_cap"
        for k in (j + 1, j + 2):
            np.testing.assert_array_equal(outs[k]["cand_idx"], ref_idx[ref_off[cuts[k]]:ref_off[cuts[k + 1]]], err_msg=f"cap {cap}: call {k} after the short one")
    # the host entry point on the same call of the same session: the status the header promises
    for cap, want in ((total - 1, pkg.abi.SS_ERR_CAND_OVERFLOW), (total, pkg.abi.SS_OK)):
        eng = _engine(name, level)
        for k, (x, y) in enumerate(zip(cuts[:-1], cuts[1:])):
            o = eng.process(raw[x:y], want=(), cand_cap=cap if k == j else None)
            assert o["status"] == (want if k == j else pkg.abi.SS_OK), (k, cap, o["status"])
            np.testing.assert_array_equal(o["cand_off"], ref_off[x:y + 1] - ref_off[x])
            m = min(cap, total) if k == j else int(ref_off[y] - ref_off[x])
            np.testing.assert_array_equal(o["cand_idx"][:m], ref_idx[ref_off[x]:ref_off[x] + m], err_msg=f"host, cap {cap}, call {k}")
        eng.close()


# ---- start_level below the -100 of learning and warm-up frames

@pytest.mark.parametrize("name", ["8192-cf32-host-calls", "65536-cs8-fold"])
def test_a_start_level_below_the_no_data_value_lists_every_passing_bin_of_every_frame(name):
    """-100 >= -120: the reference lists every passing bin of every frame, learning and warm-up frames included (setNoData's
    -100 rows average to -100, transmission.cpp:91 compares that with the level like any value). The engine does the same."""
    s, ref = PATHS[name], _reference(name)
    n, cuts = s["n"], s["cuts"]
    passes = pass_mask(n, s["fs"], CENTER - s["fs"] // 2, CENTER + s["fs"] // 2)
    ref_off, ref_idx = lists_at_level(ref["avg"], -120.0, passes)
    assert (np.diff(ref_off) == n).all()
    for entry in ("host", "device"):
        (off, idx, avg), _ = _run(name, -120.0, 0, ref_off, entry=entry, slack=0)
        np.testing.assert_array_equal(off, ref_off, err_msg=entry)
        np.testing.assert_array_equal(idx, ref_idx, err_msg=entry)
        frames = np.repeat(np.arange(cuts[-1]), np.diff(ref_off))
        check_plane(f"{entry}: cand_avg", avg[None], ref["avg"][frames, ref_idx][None], floor=running_sum_drift_at(n, ref["avg"], frames, ref_idx)[None])
