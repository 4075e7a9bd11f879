"""The tracking digest on the CPU: the host tracker's digest form (SignalTracker::processFrameDigest, sst_process_frame_digest)
fed by the numpy restatement of the two kernels (tests/digest_ref.py) on the ORACLE's planes must give, frame by frame, what
process_batch gives on the planes themselves — and what the reference's own Transmission / Signal code recorded — on the scenarios
of tests/test_signal_tracker.py; the stream cut into uneven batches must give the same lists (the tail logic the GPU test then holds the
kernels to). Integer work and copies of plane floats: equality, no tolerance. Also: the header declares only st_*, libspecscan.so
exports them, and the two kernels compile for gfx950 without scratch."""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from digest_ref import DigestRef, argmax_literal, most_frequent, window_argmax
from refrecords import reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_tracker_*.npz")))
SPLITS = (None, (7, 64, 1, 100))  # one batch; 7, 64, 1, 100 frames and the rest


def test_restatement_matches_the_literal_walk():
    """window_argmax (vectorised) against std::max_element written out, on rows with ties, -inf runs and NaNs — at lo and elsewhere."""
    rng = np.random.default_rng(11)
    for trial in range(60):
        n = int(rng.choice([64, 257, 300]))
        half = int(rng.choice([0, 1, 5, 16, 40]))
        row = rng.integers(-3, 4, n).astype(np.float32)  # many ties
        kind = trial % 4
        if kind == 1:
            row[rng.random(n) < 0.3] = np.nan
        elif kind == 2:
            row[rng.random(n) < 0.5] = -np.inf
            row[rng.random(n) < 0.1] = np.nan
        elif kind == 3:
            row[:] = -100.0 if trial % 8 == 3 else -np.inf
        keys = np.arange(n)
        want = [argmax_literal(row, max(0, k - half), min(n, k + half + 1)) for k in keys]
        np.testing.assert_array_equal(window_argmax(row, keys, half), want, err_msg=f"trial {trial}")
    assert most_frequent([5, 3, 3, 5, 9]) == 5 and most_frequent([4, 2, 9]) == 4 and most_frequent([7, 7, 1]) == 7  # tied values ascending, position size // 2


def _scenario(n, seed, nframes, on, off, dt):
    band = pkg.synth.SyntheticBand(n, seed=seed, on_frame=on, off_frame=off, comb_width=max(8, n // 32))
    return band.frames_cf32(nframes), (1_000 + dt * np.arange(nframes)).astype(np.int64)


def _random_traffic(seed):
    """The stream of tests/test_signal_tracker.py::test_tracker_matches_reference_on_random_traffic, draw for draw."""
    rng = np.random.default_rng(600 + seed)
    n = int(rng.choice([256, 512, 1024]))
    fs = n * 250
    nframes = int(rng.integers(260, 420))
    dt = int(rng.choice([20, 40, 55]))
    min_ms, timeout_ms = int(rng.choice([0, 300, 2000])), int(rng.choice([60, 500, 2000]))
    step = int(rng.choice([2500, 1000, 12500]))
    bandwidth = int(rng.choice([8000, 16000, 32000]))
    sigma = 0.05
    x = (rng.standard_normal((nframes, n)) + 1j * rng.standard_normal((nframes, n))) * sigma
    k = np.arange(n)
    amp = pkg.synth.comb_amplitude(n, sigma)
    for _ in range(int(rng.integers(3, 9))):
        c0 = int(rng.integers(30, n - 30))
        width = int(rng.integers(6, 40))
        level = amp * float(rng.uniform(0.6, 2.0))
        start = int(rng.integers(50, nframes - 60))
        stop = min(nframes, start + int(rng.integers(5, 150)))
        bins = np.arange(c0 - width // 2, c0 + width // 2)
        for f in range(start, stop):
            ph = rng.uniform(0, 2 * np.pi, size=len(bins))
            x[f] += level * np.exp(2j * np.pi * ((bins - n // 2)[:, None] * k[None, :]) / n + 1j * ph[:, None]).sum(axis=0)
    t = (5_000 + dt * np.arange(nframes)).astype(np.int64)
    return x.astype(np.complex64), t, n, fs, dict(min_time_ms=min_ms, timeout_ms=timeout_ms, tuning_step=step, bandwidth=bandwidth)


def _batches(nframes, split):
    if split is None:
        return [(0, nframes)]
    edges = [0]
    for s in split:
        if edges[-1] + s < nframes:
            edges.append(edges[-1] + s)
    edges.append(nframes)
    return list(zip(edges[:-1], edges[1:]))


def _run_digest(r, t, n, fs, split, **tk):
    """The oracle's planes through the restatement and the digest form, batch by batch. Returns the per-frame results and whether some
    frame inserted a signal under a key that is getBestIndex of a candidate but not that candidate's own bin (the mode path)."""
    tr = pkg.tracker.SignalTracker(n, fs, **tk)
    ref = DigestRef(n, tr.group_size, tr.start_level)
    off, idx = r["cand_off"].astype(np.int64), r["cand_idx"]
    got, moved = [], False
    for a, b in _batches(len(t), split):
        d = ref.digest(r["rel"][a:b], r["avg"][a:b], off[a:b + 1] - off[a], idx[off[a]:off[b]], tr.keys)
        np.testing.assert_array_equal(d["cand_avg"], r["cand_avg"][off[a]:off[b]])  # (the oracle's list is the plane's float)
        before = set(tr.keys.tolist())
        for f, res in enumerate(tr.process_batch_digest(t[a:b], d)):
            got.append(res)
            lo, hi = int(d["cand_off"][f]), int(d["cand_off"][f + 1])
            own = set(d["cand_idx"][lo:hi].tolist())
            for key in set(res[1].tolist()) - before:
                moved |= key not in own and key in set(d["cand_best"][lo:hi].tolist())
            before = set(res[1].tolist())
    return got, moved


def _check(oracle_mod, iq, t, n, fs, want_tx, want_sig, **tk):
    O = oracle_mod
    O.lib().orc_set_fft_backend(0)
    r = O.oracle_chain(fs, 145_000_000, fft_size=n, decim=1, max_batch=iq.shape[0]).process(iq, t_ms=t)
    planes = pkg.tracker.SignalTracker(n, fs, **tk).process_batch(t, r["avg"], r["rel"], r["cand_off"], r["cand_idx"])
    seen_tx = 0
    for split in SPLITS:
        got, moved = _run_digest(r, t, n, fs, split, **tk)
        assert len(got) == len(t)
        for f in range(len(t)):
            for k in (0, 1):
                np.testing.assert_array_equal(got[f][k], planes[f][k], err_msg=f"split {split} frame {f}: digest form vs process_batch")
            np.testing.assert_array_equal(got[f][0], want_tx[f], err_msg=f"split {split} frame {f}: vs the reference")
            np.testing.assert_array_equal(got[f][1], want_sig[f], err_msg=f"split {split} frame {f}: vs the reference")
        seen_tx = sum(len(g[0]) for g in got)
    return seen_tx, moved


@pytest.mark.parametrize("n,fs,seed,min_ms,timeout_ms", [(256, 64_000, 31, 2000, 2000), (1024, 256_000, 32, 400, 600), (512, 128_000, 33, 0, 40)])
def test_digest_form_matches_planes_and_reference_live(oracle_mod, n, fs, seed, min_ms, timeout_ms):
    O = oracle_mod
    center, nframes, dt = 145_000_000, 330, 40
    iq, t = _scenario(n, seed, nframes, on=70, off=190, dt=dt)

    def live():
        O.ref().orc_set_fft_backend(0)
        return O.RefChain(n, fs, center - fs // 2, center + fs // 2, min_time_ms=min_ms, timeout_ms=timeout_ms).process(iq, t)
    want = reference(O, f"tracker_live_{n}_{fs}_{seed}", live, keep=("tx", "signals"))
    seen_tx, moved = _check(O, iq, t, n, fs, want["tx"], want["signals"], min_time_ms=min_ms, timeout_ms=timeout_ms)
    assert seen_tx > 100 and len(want["tx"][-1]) == 0
    assert moved, "no signal was inserted under a key other than its candidate: the mode path is not exercised"


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_digest_form_matches_planes_and_golden(oracle_mod, path):
    g = np.load(path)
    n, fs = int(g["n"]), int(g["fs"])
    assert int(g["center"]) == 145_000_000
    tx_off, tx, sig_off, sig = g["tx_off"], g["tx"], g["sig_off"], g["sig"]
    nframes = len(g["t_ms"])
    want_tx = [tx[tx_off[f]:tx_off[f + 1]] for f in range(nframes)]
    want_sig = [sig[sig_off[f]:sig_off[f + 1]] for f in range(nframes)]
    seen_tx, moved = _check(oracle_mod, g["iq"], g["t_ms"], n, fs, want_tx, want_sig, min_time_ms=int(g["min_ms"]), timeout_ms=int(g["timeout_ms"]))
    assert tx_off[-1] > 50 and seen_tx == tx_off[-1]
    assert moved, "no signal was inserted under a key other than its candidate: the mode path is not exercised"


@pytest.mark.parametrize("seed", range(10))
def test_digest_form_matches_planes_and_reference_on_random_traffic(oracle_mod, seed):
    O = oracle_mod
    iq, t, n, fs, tk = _random_traffic(seed)
    center = 145_000_000

    def live():
        O.ref().orc_set_fft_backend(0)
        return O.RefChain(n, fs, center - fs // 2, center + fs // 2, **tk).process(iq, t)
    want = reference(O, f"tracker_random_{seed}", live, keep=("tx", "signals"))
    _check(O, iq, t, n, fs, want["tx"], want["signals"], **tk)


def test_missing_watch_key_and_reset():
    n, fs = 256, 64_000
    tr = pkg.tracker.SignalTracker(n, fs)
    ref = DigestRef(n, tr.group_size, tr.start_level)
    avg = np.full((1, n), 20.0, np.float32)
    rel = np.full((1, n), 20.0, np.float32)
    cand = np.arange(100, 110, dtype=np.int32)
    d = ref.digest(rel, avg, [0, cand.size], cand, tr.keys)
    short = dict(d, watch=d["watch"][:0], peak_idx=d["peak_idx"][:, :0], peak_avg=d["peak_avg"][:, :0])
    with pytest.raises(ValueError):
        tr.process_batch_digest([1000], short)  # sst_process_frame_digest returned -1: the inserted key is not watched
    tr.reset()
    (tx, sig), = tr.process_batch_digest([1000], d)
    assert len(sig) >= 1 and len(tx) == len(sig)
    # reset between batches clears the signals (and the restatement's tail with them)
    tr.reset()
    ref.reset()
    assert tr.keys.size == 0
    quiet = ref.digest(np.full((1, n), -100.0, np.float32), np.full((1, n), -100.0, np.float32), [0, 0], np.zeros(0, np.int32), tr.keys)
    assert quiet["watch"].size == 0
    (tx, sig), = tr.process_batch_digest([1040], quiet)
    assert len(sig) == 0 and len(tx) == 0


def test_header_declares_only_st_names_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "specscan_track.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z]+_[a-z_0-9]+)\s*\(", text)))
    assert names == ["st_create", "st_destroy", "st_digest", "st_last_error", "st_reset"], names
    pkg.build.build_lib()
    lib = pkg.load_library()
    for name in names:
        assert hasattr(lib, name), name
    assert not [e for e in pkg.engine.EXPORTS if e.startswith("st_")] and pkg.abi.SS_ABI_VERSION == 3  # (the scan ABI is untouched)


def test_digest_kernels_use_no_scratch(tmp_path):
    """tests/host/track_digest_resources.hip instantiates the kernels; hipcc compiles them for gfx950 with the product's code-generation
    flags and reports what they use (the figures are in DESIGN.md)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"),
                          os.path.join(ROOT, "tests", "host", "track_digest_resources.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), spill=get("VGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"),
                          occupancy=get(r"Occupancy \[waves/SIMD\]"))
    print(seen)
    for kernel in ("k_window_peaks", "k_save_tail"):
        hit = [r for name, r in seen.items() if kernel in name]
        assert len(hit) == 1, (kernel, list(seen))
        assert hit[0]["scratch"] == 0 and hit[0]["spill"] == 0, (kernel, hit[0])
