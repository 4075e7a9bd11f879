"""Decimated device input — items of N * D samples, item_stride = N * D in every FFT front end — on every transform path.
ss_process_device is the only entry point that hands the kernels a stride (ss_process and the feeds compact first), so every case
here runs two engines that differ in `decim` alone: A (decim = 1) takes the compact frames, B (decim = D) takes the same frames as
the first N samples of items whose remainder is poison (tests/strided.py: NaN for CF32, the formats' extremes for the integers),
both through ss_process_device, the same calls, the same outputs asked, every call of a session in flight before one ss_sync. What
they hand out must be the same bits: a front end that strode by N, for one format, one chunk of a long call or one of the fold's two
load stages, would read poison or the wrong frame. The buffers always hold the whole nframes * N * D samples and start where torch
allocates them: no case can read out of bounds or at an odd address. A few cases are held to the oracle as well (decim = D on the
strided items, the project's tolerances), so that the file does not rest on engine against engine alone. Run with -m gpu."""
import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from parity import check_all, check_plane, dont_care_limit, hamming_f32
from strided import strided_items

pytestmark = pytest.mark.gpu

A = pkg.abi
CENTER = 145_000_000
ALL = ("psd", "rel", "avg")
IN_FORMAT = {"cf32": A.SS_FMT_CF32, "cs8": A.SS_FMT_CS8, "cu8": A.SS_FMT_CU8, "cs16": A.SS_FMT_CS16}
STATS = ("calls", "calls_overlapped", "calls_in_order", "demotions", "tiles_total", "tiles_tested", "tiles_culled")


def case(cid, n, fs, fmt, decim, calls, want, learn, seed, flags=0, env=None, window=False, form=(), **cfg):
    return dict(id=cid, n=n, fs=fs, fmt=fmt, decim=decim, calls=calls, want=want, learn=learn, seed=seed, flags=flags, env=env or {}, window=window, form=form, cfg=cfg)


# Sizes, sample rates, learning frames, frame counts and seeds: tests/test_gpu_parity.py CASES and tests/test_gpu_cs16.py BIT_CASES.
# The combs come on three frames after learning and go off three frames before the end; the 21-frame averager hands out its first
# value 20 frames after learning, so a session is at least learn + 21 frames long: where the calls a path needs are fewer than that
# (2^20 points [8, 8], 262144 points [12, 12], one call of 17 or 20 or 10 frames), a call with the learning frames stands in front.
# The culled forms test a tile only where its 16 frames (aligned to frame 0) and the 20 before them lie behind the learning frames and,
# on the fold's contexts, behind the first fold call (it rewrites the ring: ss_ctx::clean_abs): frames 48 .. 55 of [25, 6, 25] at 65536
# points, frames 32 .. 47 of [10, 19, 19] at 131072 points, whose fold starts at frame 10.
# form: what ss_get_stats / ss_read_window must show — "overlap" (calls_overlapped > 0), "in_order" (every call in order), "tiles"
# (tiles_tested > 0: the culled forms), "no_plane" (the last call kept no dB plane: a PSD window is refused).
CASES = [
    # LDS kernel, several frames per workgroup
    case("64-cu8-d3", 64, 16_000, "cu8", 3, [17, 1, 30], ALL, 20, 1),
    case("512-cs16-d2", 512, 128_000, "cs16", 2, [40, 7, 33], ALL, 15, 29),
    # register kernels, 1024 .. 4096 points: odd call sizes, a 1-frame call
    case("1024-cs8-d3", 1024, 256_000, "cs8", 3, [63, 1, 57, 29], ALL, 30, 2),
    case("2048-cf32-d2", 2048, 512_000, "cf32", 2, [31, 1, 29, 29], ALL, 25, 3),
    case("2048-cs16-d5", 2048, 512_000, "cs16", 5, [31, 1, 29, 29], ALL, 25, 3),
    case("4096-cu8-d5", 4096, 1_024_000, "cu8", 5, [37, 1, 42], ALL, 22, 4),
    # 8192 points: deep pipelining (the next launch reads a call's last frames once more), and every stage in order on the public stream
    case("8192-cs8-d3-overlapped", 8192, 2_048_000, "cs8", 3, [37, 64, 5, 64, 30], ALL, 10, 63, form=("overlap",)),
    case("8192-cu8-d4-stream-ordered", 8192, 2_048_000, "cu8", 4, [33, 1, 36], ALL, 21, 6, flags=A.SS_FLAG_STREAM_ORDERED, form=("in_order",)),
    # four-step, 256-point column tiles
    case("16384-cf32-d3-planes", 16384, 4_096_000, "cf32", 3, [30, 30, 4], ALL, 10, 7),
    case("32768-cu8-d2-planes", 32768, 6_000_000, "cu8", 2, [24, 24, 12], ALL, 8, 10),
    # 65536 points: the radix-8 fold, the culled chain in one launch per call, the calls that keep their planes
    case("65536-cs8-d3-fold", 65536, 20_000_000, "cs8", 3, [25, 6, 25], (), 6, 8, form=("tiles", "no_plane")),
    case("65536-cf32-d2-merged", 65536, 20_000_000, "cf32", 2, [25, 6, 25], (), 6, 8, form=("tiles", "no_plane")),
    case("65536-cs16-d2-merged", 65536, 20_000_000, "cs16", 2, [25, 6, 25], (), 6, 8, form=("tiles", "no_plane")),
    case("65536-cs8-d2-planes", 65536, 20_000_000, "cs8", 2, [16, 16, 8], ALL, 6, 8),
    # 131072 points at a third of 20 MS/s (the reference's rule D = max(1, int(fs / N / 50)) gives D = 3): the radix-16 fold, the four-step form
    case("131072-cs8-d3-fold", 131072, 20_000_000, "cs8", 3, [10, 19, 19], (), 4, 9, form=("tiles", "no_plane")),
    case("131072-cf32-d3-psd", 131072, 20_000_000, "cf32", 3, [20, 20], ("psd",), 4, 9),
    # 262144 points (61.44 MS/s: D = 4): the culled chain
    case("262144-cs8-d4-culled", 262144, 61_440_000, "cs8", 4, [24, 12, 12], (), 4, 71, form=("tiles", "no_plane")),
    case("262144-cf32-d2-culled", 262144, 61_440_000, "cf32", 2, [24, 12, 12], (), 4, 71, form=("tiles", "no_plane")),
    # 2^20 points in two passes of 1024
    case("1048576-cs8-d2-detect", 1 << 20, 61_440_000, "cs8", 2, [12, 8, 8], (), 3, 62, form=("no_plane",)),
    case("1048576-cf32-d2-planes-gy3", 1 << 20, 61_440_000, "cf32", 2, [6], ALL, 2, 9, grouping_y=3),
    # per-chunk base offsets of chunked calls, product library: 2^20 points in chunks of 16 (16 + 1), 262144 points in chunks of 64 (64 + 2)
    case("1048576-cs8-d2-chunks-16+1", 1 << 20, 61_440_000, "cs8", 2, [12, 17], (), 3, 62, form=("no_plane",)),
    case("262144-cs8-d2-chunks-64+2", 262144, 61_440_000, "cs8", 2, [66], (), 4, 71),
    # ... under the diagnostics library's chunk sizes
    case("65536-cf32-d2-chunks-8", 65536, 20_000_000, "cf32", 2, [10, 20], ALL, 6, 8, env={"SS_CHUNK_65536": "8"}),
    case("1048576-cs8-d3-chunks-4", 1 << 20, 61_440_000, "cs8", 3, [10, 10, 10], (), 3, 62, env={"SS_CHUNK_LONG": "4"}, form=("no_plane",)),
    # the generic forms: k_fft_psd_lds, k_fft_cols
    case("2048-cs8-d3-generic", 2048, 512_000, "cs8", 3, [31, 1, 29, 29], ALL, 25, 3, env={"SS_FFT_IMPL": "generic"}),
    case("65536-cs8-d2-generic", 65536, 20_000_000, "cs8", 2, [25, 6, 25], ("psd",), 6, 8, env={"SS_FFT_IMPL": "generic"}),
    # a caller's window: no fold, the taps from the table
    case("65536-cs8-d2-hamming-taps", 65536, 20_000_000, "cs8", 2, [25, 6, 25], (), 6, 8, window=True, form=("tiles", "no_plane")),
]
ANCHORS = ["1024-cs8-d3", "8192-cs8-d3-overlapped", "16384-cf32-d3-planes", "65536-cs8-d2-planes", "131072-cf32-d3-psd"]
BY_ID = {c["id"]: c for c in CASES}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a


def _same(tag, a, b):
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    ba, bb = _bits(a).reshape(-1), _bits(b).reshape(-1)
    bad = np.flatnonzero(ba != bb)
    assert bad.size == 0, (tag, bad.size, bad[:5], a.reshape(-1)[bad[:5]], b.reshape(-1)[bad[:5]])


def _frames(c):
    """The session's compact frames, [nframes, N(, 2)]."""
    nframes = sum(c["calls"])
    on, off = (2, 100) if "grouping_y" in c["cfg"] else (c["learn"] + 3, nframes - 3)
    band = pkg.synth.SyntheticBand(c["n"], seed=c["seed"], on_frame=on, off_frame=off)
    return {"cf32": band.frames_cf32, "cs8": band.frames_cs8, "cu8": band.frames_cu8, "cs16": band.frames_cs16}[c["fmt"]](nframes)


def _config(c, decim):
    kw = dict(fft_size=c["n"], decim=decim, in_format=IN_FORMAT[c["fmt"]], learn_frames=c["learn"], max_batch=max(max(c["calls"]), 8), flags=c["flags"], **c["cfg"])
    if c["n"] == 8192 and not c["flags"]:
        kw["max_batch"] = max(kw["max_batch"], 64)
    if c["window"]:
        kw["window"] = hamming_f32(c["n"])
    return kw


def _to_device(items, dev):
    import torch
    return torch.from_numpy(items.view(np.float32) if items.dtype == np.complex64 else items).to(dev)


class Session:
    """Every call of c["calls"] on one engine through ss_process_device, nothing in between; then one ss_sync. Input and output
    tensors live as long as the object does."""

    def __init__(self, c, eng, items, one_allocation=False):
        import torch
        dev = torch.device("cuda", 0)
        n, cuts = c["n"], np.concatenate([[0], np.cumsum(c["calls"])])
        if one_allocation:  # the calls' inputs back to back: call k + 1 starts at the byte call k's last item ends at
            whole = _to_device(items, dev)
            self.d_iq = [whole[a:b] for a, b in zip(cuts, cuts[1:])]
            assert all(x.data_ptr() + x.numel() * x.element_size() == y.data_ptr() for x, y in zip(self.d_iq, self.d_iq[1:]))
        else:
            self.d_iq = [_to_device(items[a:b], dev) for a, b in zip(cuts, cuts[1:])]
        cap = min(n, 2048)
        self.outs = []
        for size in c["calls"]:
            o = {k: torch.empty((size, n), dtype=torch.float32, device=dev) for k in c["want"]}
            o.update(cand_off=torch.zeros(size + 1, dtype=torch.int32, device=dev), cand_idx=torch.empty(size * cap, dtype=torch.int32, device=dev),
                     cand_avg=torch.empty(size * cap, dtype=torch.float32, device=dev))
            self.outs.append(o)
        torch.cuda.synchronize()  # (torch's copies and fills run on torch's stream, the library works on its own)
        for d, o, size in zip(self.d_iq, self.outs, c["calls"]):
            assert d.shape[0] == size and d.numel() * d.element_size() == size * n * eng.cfg.decim * A.SS_FMT_BYTES[eng.cfg.in_format]
            eng.process_device(d, size, **o)
        eng.sync()
        self.stats = eng.stats()
        self.res = []
        for o in self.outs:
            r = {k: v.cpu().numpy() for k, v in o.items()}
            total = int(r["cand_off"][-1])
            assert total <= r["cand_idx"].size
            r["cand_idx"], r["cand_avg"] = r["cand_idx"][:total], r["cand_avg"][:total]
            self.res.append(r)
        self.total = sum(len(r["cand_idx"]) for r in self.res)

    def joined(self):
        got = {k: np.concatenate([r[k] for r in self.res]) for k in self.res[0] if k != "cand_off"}
        got["cand_off"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(r["cand_off"]) for r in self.res]))]).astype(np.int32)
        return got


def _use(c, request, monkeypatch):
    if c["env"]:  # (the product library never reads the environment)
        request.getfixturevalue("diag_lib")
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_strided_items_give_the_bits_of_compact_frames(cid, request, monkeypatch):
    c = BY_ID[cid]
    _use(c, request, monkeypatch)
    n, fs, decim = c["n"], c["fs"], c["decim"]
    x = _frames(c)
    y = strided_items(x, decim, c["fmt"])
    ea, eb = pkg.SpectrumEngine(fs, CENTER, **_config(c, 1)), pkg.SpectrumEngine(fs, CENTER, **_config(c, decim))
    sa, sb = Session(c, ea, x), Session(c, eb, y)
    for k, (ra, rb) in enumerate(zip(sa.res, sb.res)):
        for key in c["want"] + ("cand_off", "cand_idx", "cand_avg"):
            _same(f"call {k} {key}", ra[key], rb[key])
    (ta, ready_a), (tb, ready_b) = ea.read_noise(), eb.read_noise()
    assert ready_a and ready_b
    _same("noise ceiling", ta, tb)
    last, ring = c["calls"][-1], -min(3, ea.cfg.grouping_y - 1)
    for frame in (last // 2, ring):  # a row of the last call, and a ring row from before it
        if frame < 0 and len(c["calls"]) == 1:
            continue  # (one call and nothing before it: the ring holds no row yet)
        _same(f"rel window, frame {frame}", ea.read_window(A.SS_PLANE_REL, frame, 0, n), eb.read_window(A.SS_PLANE_REL, frame, 0, n))
    sta, stb = sa.stats, sb.stats
    print(f"\n[{cid}] {sa.total} candidates; " + ", ".join(f"{k} {sta[k]}" for k in STATS))
    assert {k: sta[k] for k in STATS} == {k: stb[k] for k in STATS}
    assert sta["calls"] == len(c["calls"]) and sta["demotions"] == 0
    if "overlap" in c["form"]:
        assert sta["calls_overlapped"] > 0, sta
    if "in_order" in c["form"]:
        assert sta["calls_overlapped"] == 0 and sta["calls_in_order"] == len(c["calls"]), sta
    if "tiles" in c["form"]:
        assert sta["tiles_tested"] > 0, sta
    if "no_plane" in c["form"]:
        for e in (ea, eb):
            with pytest.raises(A.SpecscanError) as err:
                e.read_window(A.SS_PLANE_PSD, 0, 0, 16)
            assert err.value.status == A.SS_ERR_INVALID
    assert sa.total > 50, "equal lists say little when they are short"


@pytest.mark.parametrize("cid", ANCHORS)
def test_strided_items_match_the_oracle(oracle_mod, cid):
    """The oracle at decim = D on the same strided items, in the same cuts: engine B is held to it as test_engine_matches_oracle
    (tests/test_gpu_parity.py) holds the host entry point."""
    c = BY_ID[cid]
    y = strided_items(_frames(c), c["decim"], c["fmt"])
    kw = _config(c, c["decim"])
    eng = pkg.SpectrumEngine(c["fs"], CENTER, **kw)
    got = Session(c, eng, y).joined()
    orc = oracle_mod.oracle_chain(c["fs"], CENTER, **kw)
    cuts = np.concatenate([[0], np.cumsum(c["calls"])])
    outs = [orc.process(y[a:b]) for a, b in zip(cuts, cuts[1:])]
    ref = {k: np.concatenate([o[k] for o in outs]) for k in ALL + ("cand_idx", "cand_avg")}
    ref["cand_off"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(o["cand_off"]) for o in outs]))]).astype(np.int32)
    errs, ncand, ndc = check_all(got, ref)
    print(f"\n[{cid}] {ncand} reference candidates, {ndc} inside the band")
    assert ncand > 50, "the test vector must produce detections"
    assert ndc <= dont_care_limit(ncand), (ncand, ndc)
    (thr_g, ready_g), (thr_o, ready_o) = eng.read_noise(), orc.read_noise()
    assert ready_g and ready_o
    check_plane("noise ceiling", thr_g[None], thr_o[None])


def test_adjacent_inputs_do_not_clash():
    """run_call_deep's clash check takes a call's input as [d_iq, d_iq + nframes * item_stride * bytes per sample). Four calls whose
    items lie back to back in one allocation — call k + 1 starts at the byte call k ends at — are adjacent, not overlapping: nothing is
    demoted, the calls overlap, and the results are the compact engine's."""
    c = case("8192-cs8-d3-adjacent", 8192, 2_048_000, "cs8", 3, [40, 40, 40, 40], ALL, 10, 63)
    x = _frames(c)
    y = strided_items(x, c["decim"], c["fmt"])
    ea, eb = pkg.SpectrumEngine(c["fs"], CENTER, **_config(c, 1)), pkg.SpectrumEngine(c["fs"], CENTER, **_config(c, c["decim"]))
    sa, sb = Session(c, ea, x, one_allocation=True), Session(c, eb, y, one_allocation=True)
    for s in (sa, sb):
        assert s.stats["demotions"] == 0 and s.stats["calls_overlapped"] > 0 and not s.stats["demoted"], s.stats
    assert sa.stats["calls_overlapped"] == sb.stats["calls_overlapped"]
    for k, (ra, rb) in enumerate(zip(sa.res, sb.res)):
        for key in ALL + ("cand_off", "cand_idx", "cand_avg"):
            _same(f"call {k} {key}", ra[key], rb[key])
    assert sa.total > 50
