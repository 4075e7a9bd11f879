"""The tracked feed on the CPU (include/specscan_track_feed.h, csrc/track_feed.h): the header declares only stf_*, libspecscan.so
cross-compiles and exports them, the new kernels compile for gfx950 without scratch or spills — and the WATCH RULE the device
implements is checked where it can be checked without a GPU: on the oracle's planes, the numpy restatement (tests/digest_ref.py) fed
with W_k = sort(unique(K_p U cand_best(p + 1 .. k))), keys taken from `lag` batches before the previous one (p = k - 1 - lag; lag 0 is the synchronous rule), must take the host tracker through exactly
the transmissions and keys the synchronous rule (keys = the tracker's own, batch by batch) gives. Integers: equality."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from digest_ref import DigestRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STF = ["stf_collect", "stf_create", "stf_destroy", "stf_last_error", "stf_post_keys", "stf_reset"]
KERNELS = ("k_feed_prepare", "k_feed_stamp", "k_feed_count", "k_feed_scan", "k_feed_scatter", "k_feed_peaks")


def test_header_declares_only_stf_names():
    text = open(os.path.join(ROOT, "include", "specscan_track_feed.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b([a-z]+_[a-z_0-9]+)\s*\(", text)))
    assert names == STF, names
    assert '#include "specscan.h"' in text and '#include "specscan_track.h"' in text
    assert sorted(pkg.tracker.STF_EXPORTS) == STF


def test_library_exports_the_stf_names():
    pkg.build.build_lib()
    lib = pkg.load_library()
    for name in STF:
        assert hasattr(lib, name), name
    assert not [e for e in pkg.engine.EXPORTS if e.startswith("stf_")] and pkg.abi.SS_ABI_VERSION == 3  # (the scan ABI is untouched)
    assert pkg.tracker.bind_track_feed(lib) is pkg.tracker.bind_track_feed(lib)  # (one result class: a second tracker leaves the first one's usable)


def test_feed_kernels_use_no_scratch(tmp_path):
    """tests/host/track_feed_resources.hip instantiates the kernels; hipcc compiles them for gfx950 with the product's code-generation
    flags and reports what they use (the figures are in DESIGN.md)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    codegen = [f for f in pkg.build.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f not in ("-fPIC",)]
    out = subprocess.run([hipcc, *codegen, "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.o"),
                          os.path.join(ROOT, "tests", "host", "track_feed_resources.hip")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        seen[name] = dict(vgprs=get("VGPRs"), spill=get("VGPRs Spill"), scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"),
                          occupancy=get(r"Occupancy \[waves/SIMD\]"))
    print(seen)
    assert len([name for name in seen if "k_feed_" in name]) == len(KERNELS), list(seen)
    for kernel in KERNELS:
        hit = [r for name, r in seen.items() if kernel in name]
        assert len(hit) == 1, (kernel, list(seen))
        assert hit[0]["scratch"] == 0 and hit[0]["spill"] == 0, (kernel, hit[0])
    # the digest's own kernels are launched unchanged: track_feed.h adds no second body under one of their names
    text = open(os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc", "track_feed.h")).read()
    assert not re.search(r"__global__[^;{]*\b\w*(k_cand_best|k_window_peaks|k_save_tail)\w*\s*\(", text)


def _batches(nframes, sizes):
    edges, k = [0], 0
    while edges[-1] < nframes:
        edges.append(min(nframes, edges[-1] + sizes[k % len(sizes)]))
        k += 1
    return list(zip(edges[:-1], edges[1:]))


STREAMS = [  # n, seed, on, off, frames, batch sizes, lag
    (1024, 21, 28, 110, 170, (1, 16, 7, 3, 16, 16, 5), 2),
    (1024, 21, 28, 110, 170, (1, 16, 7, 3, 16, 16, 5), 1),
    (1024, 21, 28, 110, 170, (16,), 3),
    (256, 5, 30, 90, 150, (7, 64, 1, 30), 2),
]


@pytest.mark.parametrize("n,seed,on,off,nframes,sizes,lag", STREAMS)
def test_watch_rule_gives_the_synchronous_transmissions(oracle_mod, n, seed, on, off, nframes, sizes, lag):
    O = oracle_mod
    fs, g = n * 250, 128
    iq = pkg.synth.SyntheticBand(n, seed=seed, on_frame=on, off_frame=off).frames_cf32(nframes)
    t = (1_000 + 40 * np.arange(nframes)).astype(np.int64)
    O.lib().orc_set_fft_backend(0)
    r = O.oracle_chain(fs, 145_000_000, fft_size=n, decim=1, max_batch=nframes, learn_ms=280).process(iq, t_ms=t)
    off_all, idx_all = r["cand_off"].astype(np.int64), r["cand_idx"]
    tk = dict(group_size=g, min_time_ms=200, timeout_ms=400)
    tr_sync, tr_feed = pkg.tracker.SignalTracker(n, fs, **tk), pkg.tracker.SignalTracker(n, fs, **tk)
    ref_sync, ref_feed = DigestRef(n, g, tr_sync.start_level), DigestRef(n, g, tr_feed.start_level)
    keys_after = {0: np.zeros(0, np.int32)}  # K_p as the feed's tracker had them after batch p
    best_of = {}
    larger = total_tx = longest = 0
    cuts = _batches(nframes, sizes)
    for k, (a, b) in enumerate(cuts, start=1):
        off, idx = off_all[a:b + 1] - off_all[a], idx_all[off_all[a]:off_all[b]]
        d_sync = ref_sync.digest(r["rel"][a:b], r["avg"][a:b], off, idx, tr_sync.keys)
        best_of[k] = d_sync["cand_best"]  # (no function of the tracker's state)
        p = max(0, k - 1 - lag)  # the synchronous rule is lag 0: keys after batch k - 1
        w_k = np.unique(np.concatenate([keys_after[p]] + [best_of[q] for q in range(p + 1, k + 1)])).astype(np.int32)
        d_feed = ref_feed.digest(r["rel"][a:b], r["avg"][a:b], off, idx, w_k)
        np.testing.assert_array_equal(d_feed["watch"], w_k)
        np.testing.assert_array_equal(d_feed["cand_best"], d_sync["cand_best"])
        assert set(d_sync["watch"].tolist()) <= set(w_k.tolist()), f"batch {k}: W_k misses a key of the synchronous watch list"
        larger += w_k.size > d_sync["watch"].size
        longest = max(longest, w_k.size)
        got_sync = tr_sync.process_batch_digest(t[a:b], d_sync)
        got_feed = tr_feed.process_batch_digest(t[a:b], d_feed)  # (raises if a tracked key is missing from the watch list)
        for f in range(b - a):
            np.testing.assert_array_equal(got_feed[f][0], got_sync[f][0], err_msg=f"batch {k} frame {f}: transmissions")
            np.testing.assert_array_equal(got_feed[f][1], got_sync[f][1], err_msg=f"batch {k} frame {f}: signal keys")
        total_tx += sum(len(x[0]) for x in got_feed)
        keys_after[k] = tr_feed.keys.copy()
    print(f"n {n} seed {seed} lag {lag}: {len(cuts)} batches, {total_tx} transmissions, W_k strictly larger in {larger}, longest {longest}")
    assert larger >= 1
    if n == 1024:
        assert total_tx > 100
