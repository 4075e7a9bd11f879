"""Shared parity checks: HIP engine vs CPU oracle (or vs golden planes made by the reference's own code).

Contract (BASELINE.json north_star):
  * per-bin dB planes:  |got - ref| <= 1e-4 * max(1, |ref|);  -100 sentinels and -inf must match exactly
    (plus the fp32-FFT rounding floor on deep nulls, and what it propagates into the 21 x 21 mean — see below);
  * candidate indices:  identical per frame, except bins whose reference avg lies within BAND dB of
    start_level — there the fp32 rounding of two different FFTs decides, and they are counted and
    reported, not compared.
"""
import numpy as np

TOL = 1e-4
BAND = 1e-3  # dB
# fp32 rounding floor of ANY single-precision FFT (FFTW included): the rounding noise of an fp32 FFT is
# ~eps_fft * RMS(spectrum) per bin in amplitude, whatever the bin holds. A bin whose power sits `depth` dB
# below the mean power of its frame therefore agrees between two correct fp32 FFTs only to a relative
# power error of 2*eps_fft*10^(depth/20), i.e. 8.7*eps_fft*10^(depth/20) dB. The per-bin tolerance is the
# contract's 1e-4*max(1,|ref|) plus this floor (it only matters for deep nulls: at
# N = 8192 it exceeds 1e-3 dB from ~34 dB and 1e-2 dB from ~54 dB below the frame mean).
def eps_fft(n):
    """Worst-case amplitude DIFFERENCE of two fp32 FFTs on a weak bin, in units of the spectrum RMS. Each
    fp32 FFT is off from fp64 by ~1.5e-7*RMS rms and, at worst over weak bins, by 0.6e-6 (N=2^10), 1.1e-6
    (2^13), 2.2e-6 (2^16), 3.2e-6 (2^17), 4.3e-6 (2^20) — measured alike for the oracle's radix-2, MKL's FFTW
    interface (tests/test_oracle_fft.py) and the HIP kernels, generic and register-pass alike
    (scripts/fft_accuracy.py). Two of them differ by up to twice that."""
    return max(0.8e-6, 2.6e-6 * (n / 8192.0) ** 0.35)


def floor_tolerance(ref_psd):
    """Per-bin dB tolerance implied by the fp32 FFT rounding floor, from the reference PSD plane."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        lin = np.power(10.0, ref_psd.astype(np.float64) / 10.0)
        fin = np.isfinite(lin) & (lin > 0)
        mean = np.where(fin, lin, 0.0).sum(axis=1, keepdims=True) / np.maximum(fin.sum(axis=1, keepdims=True), 1)
        depth_amp = np.sqrt(np.where(fin, mean / np.where(fin, lin, 1.0), 1.0))  # 10^(depth/20)
    return 8.7 * eps_fft(ref_psd.shape[1]) * np.maximum(depth_amp, 1.0)


def running_sum_drift(n, ref_avg=None):
    """Rounding drift of the REFERENCE's frequency average: utils.cpp:31-53 walks one fp32 running sum
    along the whole row (two roundings per bin), a random walk whose step is the ulp of the sum's magnitude:
    |sum| ~ 21 * 10 dB -> ulp 1.5e-5 for ordinary frames, up to ulp(2100) = 2.4e-4 while -100 sentinels are still
    inside the 21-frame mean (after a retune, at the end of learning). It reaches ~3e-4 dB at bin 2^20 in the
    ordinary case. The engine restarts its sums every 16 bins and does not drift, so the avg plane is compared
    with the contract's 1e-4 plus this 3-sigma allowance, per bin index and per frame (from the frame's own
    largest |avg|)."""
    i = np.arange(n, dtype=np.float64)
    walk = np.sqrt(2.0 * (i + 1.0)) / 21.0
    if ref_avg is None:
        return 3.0 * (1.53e-5 / np.sqrt(12.0)) * walk
    fin = np.where(np.isfinite(ref_avg), np.abs(ref_avg), 0.0)
    mag = np.maximum(21.0 * fin.max(axis=1), 128.0)  # |running sum| bound per frame (never below the ordinary case)
    ulp = np.exp2(np.floor(np.log2(mag)) - 23.0)
    return 3.0 * (ulp[:, None] / np.sqrt(12.0)) * walk[None, :]


def running_sum_drift_at(n, ref_avg, frames, bins):
    """running_sum_drift's allowance at chosen (frame, bin) pairs only — the candidates: a [frames x n] float64 plane of it would be
    hundreds of megabytes at 65536 points and more."""
    fin = np.where(np.isfinite(ref_avg), np.abs(ref_avg), 0.0)
    mag = np.maximum(21.0 * fin.max(axis=1), 128.0)
    ulp = np.exp2(np.floor(np.log2(mag)) - 23.0)
    walk = np.sqrt(2.0 * (np.asarray(bins, dtype=np.float64) + 1.0)) / 21.0
    return 3.0 * (ulp[np.asarray(frames)] / np.sqrt(12.0)) * walk


def check_plane(name, got, ref, floor=None):
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    exact = got == ref  # covers -100 and +-inf
    special = ~np.isfinite(ref) | (ref == -100.0)
    assert exact[special].all(), f"{name}: sentinel / non-finite bins differ"
    err = np.abs(got - ref)
    tol = TOL * np.maximum(1.0, np.abs(ref))
    if floor is not None:
        tol = tol + floor  # independent error sources add (dB conversion / subtraction on top of the FFT's rounding floor)
    bad = ~exact & ~(err <= tol)
    assert not bad.any(), f"{name}: {int(bad.sum())} bins outside tolerance, worst {np.nanmax(np.where(bad, err, 0)):.3e} dB"
    fin = np.isfinite(ref) & (ref != -100.0)
    return float(err[fin].max()) if fin.any() else 0.0


def cand_set(off, idx):
    frames = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return set(zip(frames.tolist(), np.asarray(idx).tolist()))


def pass_mask(n, fs, range_lo, range_hi, ignored=()):
    """Which bins a chain lists at all: isIndexInRange && !isIndexIgnored (sdr_device.cpp:153-158, transmission.cpp:156-164) — the
    bin's frequency, centre of the scanned range plus (int32)(fs / N * (i + 0.5)) - fs / 2, lies inside the range and in no ignored one
    (both ends inclusive). Anchored against the oracle's own lists by tests/test_cull_bound_math.py."""
    shift = (np.float64(fs) / n * (np.arange(n) + 0.5)).astype(np.int32) - fs // 2
    f = (int(range_lo) + int(range_hi)) // 2 + shift.astype(np.int64)
    ok = (range_lo <= f) & (f <= range_hi)
    ig = np.asarray(ignored, dtype=np.int64).reshape(-1, 2)
    for lo, hi in ig:
        ok &= ~((lo <= f) & (f <= hi))
    return ok


def lists_at_level(ref_avg, level, passes):
    """The reference's candidate lists at ANOTHER start level from one run's avg plane (which does not depend on the level):
    float32(level) <= avg[f, i] for the bins that pass (transmission.cpp:90-94; a NaN never passes). Returns (cand_off, cand_idx)
    as the chains hand them out — the set is cand_set(cand_off, cand_idx)."""
    with np.errstate(invalid="ignore"):
        hit = (np.float32(level) <= ref_avg) & np.asarray(passes, bool)[None, :]
    off = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int64)
    return off, np.nonzero(hit)[1].astype(np.int32)


def tile_bounds(psd, thr, learn, reach="runs", frames_per_tile=16, bins_per_tile=256, g=21):
    """csrc/detect_fused.h's culling bound restated on a reference's planes, for every 16-frame x 256-bin tile (frame tiles aligned
    to frame 0) whose 36 rows all lie behind the `learn` learning frames: max over the tile's frames f of mean(M_{f-20} .. M_f) - m,
    with M_g the largest dB value of frame g over the tile's reach and m the smallest noise ceiling over the column's 256 bins and
    32 more on either side. reach = "runs": those 320 bins (8192 points; the long rows' 32-bin runs); "columns": the column and both
    whole neighbours (the radix-8 / radix-16 fold keeps a maximum per column and residue). Returns [frame tiles, columns] float64,
    NaN for the tiles that are never tested."""
    nframes, n = psd.shape
    cols, side = n // bins_per_tile, (32 if reach == "runs" else bins_per_tile)
    nft = nframes // frames_per_tile
    out = np.full((nft, cols), np.nan)
    colmax = psd.astype(np.float64).reshape(nframes, cols, bins_per_tile)
    edge_lo, edge_hi = colmax[:, :, -side:].max(axis=2), colmax[:, :, :side].max(axis=2)
    m_all = colmax.max(axis=2)
    m_all[:, 1:] = np.maximum(m_all[:, 1:], edge_lo[:, :-1])
    m_all[:, :-1] = np.maximum(m_all[:, :-1], edge_hi[:, 1:])
    t = thr.astype(np.float64).reshape(cols, bins_per_tile)
    tm = t.min(axis=1)
    tm[1:] = np.minimum(tm[1:], t[:-1, -32:].min(axis=1))
    tm[:-1] = np.minimum(tm[:-1], t[1:, :32].min(axis=1))
    csum = np.vstack([np.zeros((1, cols)), np.cumsum(m_all, axis=0)])
    for ft in range(nft):
        f0 = ft * frames_per_tile
        if f0 - (g - 1) < learn:
            continue
        f = np.arange(f0, f0 + frames_per_tile)
        out[ft] = ((csum[f + 1] - csum[f + 1 - g]) / g).max(axis=0) - tm
    return out


def check_candidates(got_off, got_idx, ref_off, ref_idx, ref_avg, start_level, got_avg_plane=None):
    """Returns (n_reference_candidates, n_dont_care)."""
    a, b = cand_set(got_off, got_idx), cand_set(ref_off, ref_idx)
    near = np.abs(ref_avg - np.float32(start_level)) < BAND
    diff = [(f, i) for (f, i) in a ^ b if not near[f, i]]
    assert not diff, f"candidate sets differ outside the {BAND} dB band: {sorted(diff)[:10]}"
    # inside each frame the engine lists candidates in ascending bin order
    for f in range(len(got_off) - 1):
        seg = np.asarray(got_idx[got_off[f]:got_off[f + 1]])
        assert (np.diff(seg) > 0).all()
    return len(b), len(a ^ b)


def propagated_floor(floor, gy=21, gx=21):
    """What the fp32-FFT rounding floor of the PSD bins can add to the 21 x 21 mean that contains them: the mean of the
    per-bin floors over the same window (newest gy frames, gx bins centred, clipped at the band edges). Bins at the
    contract's own tolerance average out; this only matters where the window holds deep nulls."""
    f = np.asarray(floor, dtype=np.float64)
    nf, n = f.shape
    ct = np.vstack([np.zeros((1, n)), np.cumsum(f, axis=0)])
    lo = np.maximum(np.arange(nf) - (gy - 1), 0)
    ty = (ct[np.arange(nf) + 1] - ct[lo]) / gy  # frames before the stream's start contribute nothing
    cx = np.hstack([np.zeros((nf, 1)), np.cumsum(ty, axis=1)])
    a = gx // 2
    i = np.arange(n)
    l, r = np.maximum(i - a, 0), np.minimum(i + a, n - 1)
    return (cx[:, r + 1] - cx[:, l]) / (r - l + 1)[None, :]


def error_quantiles(got, ref, planes=("psd", "rel", "avg")):
    """Achieved |got - ref| in dB per plane over the ordinary bins (finite, not the -100 sentinel): p50, p99.9, max — so that
    the slack the tolerances leave is visible next to every verdict."""
    out = {}
    for k in planes:
        if k in got and k in ref:
            fin = np.isfinite(ref[k]) & (ref[k] != -100.0) & np.isfinite(got[k])
            if fin.any():
                e = np.abs(got[k][fin].astype(np.float64) - ref[k][fin].astype(np.float64))
                out[k] = {"p50": float(np.quantile(e, 0.5)), "p99.9": float(np.quantile(e, 0.999)), "max": float(e.max())}
    return out


def format_quantiles(q):
    return "; ".join(f"{k} p50 {v['p50']:.1e} p99.9 {v['p99.9']:.1e} max {v['max']:.1e}" for k, v in q.items())


def strict_excess(got, ref, planes=("psd", "rel", "avg")):
    """How much of each plane the contract's BARE tolerance 1e-4 * max(1, |ref|) does not cover — the bins held by the fp32-FFT
    floor / drift allowances instead: count, fraction of the ordinary bins, and the worst error among them."""
    out = {}
    for k in planes:
        if k in got and k in ref:
            fin = np.isfinite(ref[k]) & (ref[k] != -100.0) & np.isfinite(got[k])
            err = np.abs(got[k].astype(np.float64) - ref[k].astype(np.float64))
            over = fin & (err > TOL * np.maximum(1.0, np.abs(ref[k])))
            out[k] = {"n": int(over.sum()), "frac": float(over.sum() / max(int(fin.sum()), 1)), "worst": float(err[over].max()) if over.any() else 0.0}
    return out


def hamming_f32(n):
    """gr::fft::window::hamming(N) as fft_v gets it (sdr_device.cpp:164): 0.54 - 0.46 cos(2 pi k / (N - 1)) in double, stored as float."""
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))).astype(np.float32)


def fp64_psd_rows(iq_rows, fs, window=None):
    """dB rows of the SAME windowed frames (the fp32 product sample x tap both chains form) through an fp64 FFT: the truth two
    fp32 FFTs are measured against. window: the caller's taps (ss_config.window); None = the default Hamming taps."""
    n = iq_rows.shape[1]
    w = hamming_f32(n) if window is None else np.ascontiguousarray(window, dtype=np.float32)
    assert w.shape == (n,)
    x = (iq_rows.real.astype(np.float32) * w).astype(np.float64) + 1j * (iq_rows.imag.astype(np.float32) * w).astype(np.float64)
    spec = np.fft.fftshift(np.fft.fft(x, axis=1), axes=1)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10((spec.real ** 2 + spec.imag ** 2) / float(fs))


def excess_vs_fp64(iq, got_psd, ref_psd, fs, max_rows=256, window=None):
    """On the PSD bins outside the bare 1e-4 tolerance (deep nulls, where two correct fp32 FFTs part): how far the engine and the
    reference's fp32 FFT each are from an fp64 FFT of the same windowed frame. The engine is held to being no worse than 1.5 x the
    reference there (rms), i.e. the allowance covers fp32 rounding, not a defect. iq: complex64 frames [nframes, N] (decimated).
    Returns None when no bin is outside."""
    fin = np.isfinite(ref_psd) & np.isfinite(got_psd)
    err = np.abs(got_psd.astype(np.float64) - ref_psd.astype(np.float64))
    over = fin & (err > TOL * np.maximum(1.0, np.abs(ref_psd)))
    rows = np.flatnonzero(over.any(axis=1))
    if rows.size == 0:
        return None
    if rows.size > max_rows:
        rows = rows[np.linspace(0, rows.size - 1, max_rows).astype(int)]
    truth = fp64_psd_rows(iq[rows], fs, window)
    m = over[rows]
    de = np.abs(got_psd[rows].astype(np.float64) - truth)[m]
    dr = np.abs(ref_psd[rows].astype(np.float64) - truth)[m]
    res = {"bins": int(m.sum()), "frames": int(rows.size), "engine_rms": float(np.sqrt(np.mean(de ** 2))), "reference_rms": float(np.sqrt(np.mean(dr ** 2))),
           "engine_max": float(de.max()), "reference_max": float(dr.max()), "floor_max": float(floor_tolerance(ref_psd[rows])[m].max())}
    _arbitrate(res)
    return res


def _arbitrate(res):
    """The engine must be no farther from the fp64 truth than 1.5 x the reference (rms) on the bins in question — where there is a
    population to speak of; a handful of bins (a bin is outside BECAUSE the two FFTs part there: either may be the closer one) is
    held to twice the reference's own worst distance plus the fp32-FFT floor AT THOSE BINS (floor_tolerance: what any single-precision
    transform may be off by at that depth below the frame's mean) — no hand-set constant."""
    if res["bins"] >= 8:
        assert res["engine_rms"] <= 1.5 * res["reference_rms"] + 1e-6, res
    else:
        assert res["engine_max"] <= 2.0 * res["reference_max"] + res["floor_max"], res


def all_bins_vs_fp64(iq, got_psd, ref_psd, fs, max_rows=None, window=None):
    """Engine and reference against an fp64 FFT of the same windowed frames over ALL ordinary bins of a sample of rows (not only
    the bins where the two part): rms, p99.9 and max of |dB - fp64| for each, and the ratio of the rms values — whether the engine's
    transform is systematically farther from the truth than the reference's fp32 FFT is. (A sample of rows: an fp64 FFT of every
    frame of a long stream is minutes of host time.)"""
    n = got_psd.shape[1]
    if max_rows is None:
        max_rows = 64 if n <= 8192 else (24 if n <= 65536 else 6)
    rows = np.arange(got_psd.shape[0])
    if rows.size > max_rows:
        rows = rows[np.linspace(0, rows.size - 1, max_rows).astype(int)]
    truth = fp64_psd_rows(iq[rows], fs, window)
    fin = np.isfinite(truth) & np.isfinite(got_psd[rows]) & np.isfinite(ref_psd[rows])
    if not fin.any():
        return None
    de = np.abs(got_psd[rows].astype(np.float64) - truth)[fin]
    dr = np.abs(ref_psd[rows].astype(np.float64) - truth)[fin]
    # (the rms of |dB - fp64| has a heavy tail — a deep null's error is its fp32-floor error times the null's depth: on the benchmark's band
    # the five largest of half a million bins hold 15-45 % of the sum of squares, scripts/fft8192_accuracy_model.py — so the ratio of the
    # rms values moves by +-0.2 with the data; the median and the 99th percentile beside it say what is systematic)
    q = lambda e: {"rms": float(np.sqrt(np.mean(e ** 2))), "median": float(np.median(e)), "p99": float(np.quantile(e, 0.99)), "p99.9": float(np.quantile(e, 0.999)), "max": float(e.max()),  # noqa: E731
                   "top5_share_of_squares": float(np.sum(np.sort(e)[-5:] ** 2) / max(np.sum(e ** 2), 1e-300))}
    out = {"rows": int(rows.size), "bins": int(fin.sum()), "engine": q(de), "reference": q(dr)}
    out["engine_over_reference_rms"] = out["engine"]["rms"] / max(out["reference"]["rms"], 1e-30)
    out["engine_over_reference_median"] = out["engine"]["median"] / max(out["reference"]["median"], 1e-30)
    out["engine_over_reference_p99"] = out["engine"]["p99"] / max(out["reference"]["p99"], 1e-30)
    return out


def format_all_bins(v):
    if not v:
        return "no finite bins"
    e, r = v["engine"], v["reference"]
    return (f"all {v['bins']} ordinary bins of {v['rows']} rows against an fp64 FFT of the same windowed frames: engine rms {e['rms']:.2e} p99.9 {e['p99.9']:.1e} max {e['max']:.1e}; "
            f"reference's fp32 FFT rms {r['rms']:.2e} p99.9 {r['p99.9']:.1e} max {r['max']:.1e} dB; engine / reference rms {v['engine_over_reference_rms']:.2f}, "
            f"median {v['engine_over_reference_median']:.2f}, p99 {v['engine_over_reference_p99']:.2f} (the five largest bins hold {e['top5_share_of_squares']:.0%} / {r['top5_share_of_squares']:.0%} of the squares)")


def excess_vs_fp64_rel(iq, got_rel, ref_rel, fs, n_learn, max_rows=256, window=None):
    """The same arbitration for the noise-relative plane (rel = dB - learned ceiling, noise_learner.cpp:55): on its bins outside the
    bare 1e-4 tolerance, the distance of the engine and of the reference to an fp64 chain — fp64 FFT of the same windowed frames,
    ceiling = the maximum over the first n_learn frames, subtraction in fp64. None when no bin is outside."""
    fin = np.isfinite(ref_rel) & np.isfinite(got_rel) & (ref_rel != -100.0)
    err = np.abs(got_rel.astype(np.float64) - ref_rel.astype(np.float64))
    over = fin & (err > TOL * np.maximum(1.0, np.abs(ref_rel)))
    rows = np.flatnonzero(over.any(axis=1))
    if rows.size == 0 or n_learn <= 0:
        return None
    if rows.size > max_rows:
        rows = rows[np.linspace(0, rows.size - 1, max_rows).astype(int)]
    thr = fp64_psd_rows(iq[:n_learn], fs, window).max(axis=0)
    truth = fp64_psd_rows(iq[rows], fs, window) - thr[None, :]
    m = over[rows]
    de = np.abs(got_rel[rows].astype(np.float64) - truth)[m]
    dr = np.abs(ref_rel[rows].astype(np.float64) - truth)[m]
    res = {"bins": int(m.sum()), "frames": int(rows.size), "engine_rms": float(np.sqrt(np.mean(de ** 2))), "reference_rms": float(np.sqrt(np.mean(dr ** 2))),
           "engine_max": float(de.max()), "reference_max": float(dr.max()), "floor_max": float(floor_tolerance(ref_rel[rows] + thr[None, :].astype(np.float32))[m].max())}
    _arbitrate(res)
    return res


def linear_power_error(got_psd, ref_psd):
    """north_star's own wording — "per-bin power within 1e-4 relative" — on LINEAR power |X|^2 / fs: |10^((got - ref) / 10) - 1| over the
    ordinary bins, p50 / p99.9 / max, and the share of bins above 1e-4 (the deep nulls two correct fp32 FFTs disagree on)."""
    fin = np.isfinite(ref_psd) & np.isfinite(got_psd)
    d = got_psd[fin].astype(np.float64) - ref_psd[fin].astype(np.float64)
    r = np.abs(np.expm1(d * (np.log(10.0) / 10.0)))
    if r.size == 0:
        return None
    return {"p50": float(np.quantile(r, 0.5)), "p99.9": float(np.quantile(r, 0.999)), "max": float(r.max()), "frac_above_1e-4": float((r > 1e-4).mean())}


def format_excess(ex, vs64=None):
    s = "; ".join(f"{k} {v['n']} bins ({100.0 * v['frac']:.3f} %) worst {v['worst']:.1e}" for k, v in ex.items())
    if vs64:
        s += (f"; on those PSD bins, distance to an fp64 FFT of the same windowed frame: engine rms {vs64['engine_rms']:.1e} max {vs64['engine_max']:.1e}, "
              f"reference's fp32 FFT rms {vs64['reference_rms']:.1e} max {vs64['reference_max']:.1e} dB")
    return s


def dont_care_limit(ncand):
    """How many candidates may sit inside the +-1e-3 dB band around start_level (decided by fp32 rounding, counted, not
    compared): 2, or one per 2000 reference candidates for the very long vectors."""
    return max(2, ncand // 2000)


def check_all(got, ref, start_level=8.0, gy=21, gx=21):
    floor = floor_tolerance(ref["psd"]) if "psd" in ref else None
    errs = {}
    for k in ("psd", "rel", "avg"):
        if k in got and k in ref:
            if k in ("psd", "rel"):
                extra = floor
            else:
                extra = running_sum_drift(ref[k].shape[1], ref[k])
                if floor is not None:
                    extra = extra + propagated_floor(floor, gy, gx)
            errs[k] = check_plane(k, got[k], ref[k], extra)
    if floor is not None:  # the allowance must stay an exception: almost every bin is held to ~1e-4 x |ref|
        # (achieved on the suite's signals, every frame carrying its four combs: <= 6.0 % / 0.071 % at N = 2048, less at every other size)
        assert (floor > 1e-3).mean() < 0.08 and (floor > 1e-2).mean() < 0.0015
    ncand, ndc = check_candidates(got["cand_off"], got["cand_idx"], ref["cand_off"], ref["cand_idx"], ref["avg"], start_level)
    # cand_avg = avg plane at the candidates
    frames = np.repeat(np.arange(len(got["cand_off"]) - 1), np.diff(got["cand_off"]))
    if "avg" in got and len(frames):
        np.testing.assert_array_equal(got["cand_avg"], got["avg"][frames, got["cand_idx"]])
    return errs, ncand, ndc
