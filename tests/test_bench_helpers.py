"""bench.py's bookkeeping, on the CPU: which command lines count as a configuration's own (the committed PMC passes belong to those),
the kernels a chain's `roofline.kernels` lists with what each must move, and the fabric bytes per launch read back from the
committed passes under profiles/ (steady-state launch shapes)."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def test_presets_and_what_counts_as_one():
    b = _bench()
    a = b.parse_args([])
    assert (a.fft, a.frames, a.fmt, a.no_psd_out, a.gpus) == (8192, 1024, "cf32", False, 1) and b.is_preset(a)
    a = b.parse_args(["--config", "3", "--gpus", "1"])
    assert (a.fft, a.frames, a.fmt, a.no_psd_out, a.sample_rate) == (65536, 128, "cs8", True, 20_000_000) and b.is_preset(a)
    a = b.parse_args(["--config", "5", "--gpus", "1"])
    assert (a.fft, a.frames, a.fmt, a.shard, a.sample_rate) == (1 << 20, 16, "cf32", "frames", 61_440_000) and b.is_preset(a)
    assert b.parse_args(["--config", "5"]).gpus == 8 and b.parse_args(["--config", "4"]).gpus == 8
    for extra in (["--no-cull"], ["--no-psd-out"], ["--fmt", "cs8"], ["--frames", "512"], ["--spectrogram"], ["--start-level", "3"]):
        assert not b.is_preset(b.parse_args(extra)), extra
    assert not b.is_preset(b.parse_args(["--config", "5", "--gpus", "1", "--frames", "64"]))


def test_chain_kernels_and_their_bytes():
    b = _bench()
    assert [k[0] for k in b.chain_kernels(8192, "cf32")] == ["step"] and b.chain_kernels(8192, "cf32")[0][3] == 12.0
    assert b.chain_kernels(8192, "cs8")[0][3] == 6.0
    for nb in (None, 128, 512):  # config 3 as it ships (int8 IQ, detect mode): the radix-8 fold, one launch per call whatever its length, int8 in + rel rows out
        assert {k[0]: k[3] for k in b.chain_kernels(65536, "cs8", nb, True)} == {"step": 6.0}
        assert b.traffic_from_profiles(3, b.chain_kernels(65536, "cs8", nb, True)[0][1]) is not None  # (the kernel name the committed pass is searched for)
    assert {k[0]: k[3] for k in b.chain_kernels(131072, "cs8", 64, True)} == {"step": 6.0}  # what getFft picks at 20 MS/s: the same fold with radix 16
    k3 = {k[0]: k[3] for k in b.chain_kernels(65536, "cs8")}  # ... a call that keeps a plane: the four-step form
    assert k3 == {"step": 22.0}  # one launch per call: columns (int8 in + work buffer out) and rows (work in + dB out)
    k3 = {k[0]: k[3] for k in b.chain_kernels(65536, "cs8", 256)}
    assert k3 == {"step": 10.0, "rows": 12.0, "plan": 0.0}  # calls of more than 128 frames: two launches
    assert {k[0]: k[3] for k in b.chain_kernels(65536, "cf32", 128, True)} == {"step": 28.0}  # CF32 IQ: the four-step form in detect mode too
    k5 = {k[0]: k[3] for k in b.chain_kernels(1 << 20, "cf32")}
    assert k5 == {"step": 16.0, "rows": 12.0, "plan": 0.0}  # 2^20 points in two passes: column half (a launch of its own), row half (k_scan_step's FFT role), plan
    os.environ["SS_FFT_TWOPASS"] = "0"  # (a switch of the diagnostics build: round 3's three passes)
    try:
        assert {k[0]: k[3] for k in b.chain_kernels(1 << 20, "cf32")} == {"step": 16.0, "sub": 16.0, "rows": 12.0, "plan": 0.0}
    finally:
        del os.environ["SS_FFT_TWOPASS"]
    assert b.algo_bytes_per_sample("cf32", True) == 12.0 and b.algo_bytes_per_sample("cs8", False) == 2.0


def test_ranks_take_their_own_device_and_only_rank_zero_of_one_runs_the_side_legs():
    """bench.py at N > 1 (the driver's 2 / 4 / 8-GPU runs, which no round could try on hardware): rank r works on device LOCAL_RANK,
    and the legs beside the timed region — CPU baseline, live PMC passes, `also`, the parity sample — run at N = 1 with --full only."""
    b = _bench()
    args = b.parse_args(["--full"])
    for world in (2, 4, 8):
        seen = set()
        for r in range(world):
            p = b.rank_plan(r, r, world, 8, args, 8192)
            seen.add(p["device_index"])
            assert p["device_index"] == r and not p["shares_device"]
            assert not (p["cpu_baseline"] or p["live_pmc"] or p["also"] or p["parity"]), (world, r, p)
        assert seen == set(range(world))
    p = b.rank_plan(0, 0, 1, 1, args, 8192)
    assert p["device_index"] == 0 and p["cpu_baseline"] and p["live_pmc"] and p["also"] and p["parity"]
    p = b.rank_plan(3, 3, 4, 1, args, 8192)  # a one-GPU box asked for four ranks (gloo, functional only): they share device 0 and say so
    assert p["device_index"] == 0 and p["shares_device"]
    sub = b.parse_args(["--config", "3", "--gpus", "1", "--sub", "--no-cpu-baseline", "--full"])
    p = b.rank_plan(0, 0, 1, 1, sub, 65536)
    assert p["parity"] and not (p["cpu_baseline"] or p["live_pmc"] or p["also"])  # an `also` run: its own parity sample, nothing else
    for argv in ([], ["--gpus", "1", "--steps", "20", "--warmup", "5"], ["--config", "3", "--gpus", "1"]):  # a plain run: the timed region only
        plain = b.parse_args(argv)
        p = b.rank_plan(0, 0, 1, 1, plain, plain.fft)
        assert not plain.full and not (p["cpu_baseline"] or p["live_pmc"] or p["also"] or p["parity"]), (argv, p)


def test_kernel_tally_is_per_launch():
    """A call the library takes through in chunks has several launches per slot: bytes per launch are those of the chunk's frames
    (round 4 divided a 64-frame call's bytes by one 16-frame launch's duration and printed 2.07 of peak)."""
    b = _bench()
    n, nb = 1 << 20, 64
    chain = b.chain_kernels(n, "cf32", nb, True)
    # twenty sampled launches per slot, each over a 16-frame chunk: 64.8 and 57.6 us per launch (BENCH_r04's figures)
    slots = {"step": (20 * 64.78e-3, 20, 20 * 16), "rows": (20 * 57.61e-3, 20, 20 * 16), "sub": (0.0, 0, 0), "plan": (0.0, 0, 0)}
    ks = {k["slot"]: k for k in b.kernel_tally(chain, slots, n, nb)}
    assert set(ks) == {"step", "rows"}
    for k in ks.values():
        assert k["frames_per_launch"] == 16 and k["launches_per_call"] == 4.0, k
        assert 0.3 < k["frac_of_peak"] <= 1.0, k
    assert abs(ks["step"]["bytes_per_launch_it_must_move"] - 16.0 * 16 * n) < 1 and abs(ks["step"]["gbs"] - 16.0 * 16 * n / 64.78e-6 / 1e9) < 1.0
    # a tally without frame counts (an older library): the call's frames per launch, as before
    ks = b.kernel_tally(b.chain_kernels(8192, "cf32"), {"step": (8 * 44e-3, 8, 0)}, 8192, 1024)
    assert ks[0]["frames_per_launch"] == 1024 and ks[0]["launches_per_call"] == 1.0 and ks[0]["frac_of_peak"] <= 1.0


def test_traffic_from_the_committed_pmc_passes():
    b = _bench()
    step = b.traffic_from_profiles(2, "k_scan_step", (1024 + 20 + 128 + 4) * 512)
    assert step and 100.66e6 < step["bytes_per_launch"] < 1.35 * 100.66e6, step  # the review's mark: <= 1.35 x the algorithmic 100.66 MB
    assert b.traffic_from_profiles(2, "k_scan_step", 12345) is None  # no launch of that shape
    # config 3 as it ships (round 5: the radix-8 fold, one launch per call, no work buffer): every launch of the step kernel in the pass
    c3 = b.traffic_from_profiles(3, "k_scan_step<1, false, 2, true, false, 8>")["bytes_per_launch"]
    # config 5 in two passes: column half (the plan of the call before at its front), row half (+ the deferred stages riding on it)
    c5 = sum(b.traffic_from_profiles(5, m, s)["bytes_per_launch"]
             for m, s in (("k_fft_cols1024", (16 * 64 + 128) * 1024), ("k_scan_step", (16 * 128 + 16 + 64) * 512)))
    assert 5.0 < c3 / (128 * 65536) < 10.0 and 24.0 < c5 / (16 * (1 << 20)) < 31.0, (c3 / (128 * 65536), c5 / (16 * (1 << 20)))  # 7.0 and 30.3 B per sample (round 4: 25.9 and 30.3; the review's marks: <= 10 and <= 27)
    assert b.traffic_from_profiles(4, "k_scan_step") is None


def test_the_line_the_driver_parses_is_a_few_kb_whatever_the_run_measured():
    """Round 5's single ~30 KB JSON line was more than the driver parses (BENCH_r05.parsed: null). The last line of stdout is now
    compact_line(full): the contract's keys, roofline and cpu_baseline, a parity verdict and one short record per `also` entry; the
    full form goes to bench_full.json. Held here on round 5's own full line and on a line with absurdly long strings."""
    import json
    b = _bench()
    full = json.loads(open(os.path.join(ROOT, "profiles", "r05", "s38_bench_default_k20.json")).read().strip().splitlines()[-1])
    assert len(json.dumps(full)) > 25_000
    line = b.compact_line(full)
    text = json.dumps(line)
    assert len(text) < 6000, len(text)
    back = json.loads(text)
    assert back == line
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in back, k
    assert back["value"] == full["value"] and back["ms_per_step"] == full["ms_per_step"] and back["config"]["workload"].startswith("8192-pt FFT")
    r = back["roofline"]
    assert r["bound"] == "hbm" and r["frac"] == full["roofline"]["frac"] and r["peak"] == 8000.0 and r["traffic"] == full["roofline"]["traffic"] and len(r["kernel"]) <= 120
    assert back["cpu_baseline"]["kind"] == "reference" and back["cpu_baseline"]["cores"] == 16 and back["cpu_baseline"]["value"] == full["cpu_baseline"]["value"]
    assert back["parity"]["inside_band"] == 0 and back["parity"]["engine_over_reference_rms"] == 1.24 and back["parity"]["timed_path"]["inside_band"] == 0
    assert len(back["also"]) == len(full["also"]) and all(len(json.dumps(e)) < 420 for e in back["also"])
    assert [e.get("variant") for e in back["also"]][-2:] == ["drop_in_path", "drop_in_path"]
    # whatever a run puts into its strings and lists, the line stays small
    fat = json.loads(json.dumps(full))
    fat["config"]["workload"] = "w" * 5000
    fat["roofline"]["kernel"] = "k" * 5000
    fat["cpu_baseline"]["sample"] = "s" * 5000
    fat["parity"] = {"failed": "f" * 5000}
    fat["also"].append({"baseline_config": 3, "error": "e" * 5000})
    assert len(json.dumps(b.compact_line(fat))) < 6500
    # a CPU-only line (config 1) and a multi-rank line (no side legs) go through as well
    assert b.compact_line({"metric": "m", "value": 1.0, "roofline": None, "cpu_baseline": None, "config": {"workload": "x"}})["roofline"] is None


def test_dumped_outputs_are_float_within_the_limit_and_the_same_every_time(tmp_path):
    """--dump-outputs: the candidate lists whole (integers exactly, as float64), the planes whole while everything fits in the
    limit and otherwise the same seeded sample of frames of every plane, with the frames' indices beside them."""
    import numpy as np
    b = _bench()
    a = b.parse_args(["--dump-outputs", str(tmp_path)])
    assert a.dump_outputs == str(tmp_path) and b.parse_args([]).dump_outputs is None
    rng = np.random.default_rng(1)
    psd = rng.standard_normal((64, 256)).astype(np.float32)
    off = np.arange(65, dtype=np.int32) * 3
    idx = rng.integers(0, 256, off[-1], dtype=np.int32)
    lists = {"cand_off": off, "cand_idx": idx, "cand_avg": rng.standard_normal(off[-1]).astype(np.float32)}
    shapes = b.dump_outputs(str(tmp_path / "whole"), {"psd": psd}, lists)
    assert shapes == {"cand_off": (65,), "cand_idx": (192,), "cand_avg": (192,), "psd": (64, 256)}
    got = {k: np.load(tmp_path / "whole" / f"{k}.npy") for k in shapes}
    assert got["cand_off"].dtype == np.float64 and np.array_equal(got["cand_off"], off) and np.array_equal(got["cand_idx"], idx)
    assert got["cand_avg"].dtype == np.float32 and got["psd"].dtype == np.float32 and np.array_equal(got["psd"], psd)
    limit = 40 * 1024
    for d in ("s1", "s2"):
        shapes = b.dump_outputs(str(tmp_path / d), {"psd": psd, "rel": psd + 1}, lists, limit=limit)
        assert sum(os.path.getsize(tmp_path / d / f"{k}.npy") for k in shapes) <= limit + 128 * len(shapes)  # (+ the .npy headers)
    rows = np.load(tmp_path / "s1" / "plane_frames.npy")
    assert 0 < rows.size < 64 and np.all(np.diff(rows) > 0) and np.array_equal(rows, np.load(tmp_path / "s2" / "plane_frames.npy"))
    r = rows.astype(int)
    assert np.array_equal(np.load(tmp_path / "s1" / "psd.npy"), psd[r]) and np.array_equal(np.load(tmp_path / "s1" / "rel.npy"), psd[r] + 1)
