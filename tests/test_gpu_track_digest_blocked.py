"""The blocked candidates' kernel (csrc/track_digest_blocked.h) on the GPU, through st_digest and the tracked feed, with the harness of
tests/test_gpu_track_digest.py (_run: detected lists at start_level 8 with a digest tracker and a plane tracker, grid lists at
start_level -30 with keys 0, N / 2 and N - 1, every batch against the numpy restatement on the engine's own planes) and of
tests/test_gpu_track_feed.py (route A: a second engine with st_digest and the plane tracker; route B: the tracked feed): every window
width at which the kernel takes another path — one bin, blocks narrower and wider than a lane's chunk, windows wider than the tile, than
the row (both clips) — and the wide recording bandwidths, up to 4096 bins. Integers equal, floats bit-equal: no tolerance anywhere.
Needs an MI355X: run with -m gpu."""
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
import test_gpu_track_digest as digest_tests
import test_gpu_track_feed as feed_tests

pytestmark = pytest.mark.gpu

KEEP = pkg.abi.SS_FLAG_KEEP_PLANES
CENTER = 145_000_000
INVALID = pkg.abi.SS_ERR_INVALID


def _tx(route):
    return sum(len(x) for x in route.tx)


def _small(g, gy=21):
    """Learning frames are all-tie rows of -100: "the first maximum wins" at every alignment of the blocks against the tile."""
    real, grid, total = digest_tests._run(256, "frames_cf32", g=g, nframes=150, sizes=(7, 64, 1, 30), max_batch=64, gy=gy)
    assert total > 100
    return real, grid


@pytest.mark.parametrize("g", [0, 1, 2, 3, 40, 128, 255, 256, 600])
def test_small_fused(g):
    real, grid = _small(g)  # g = 600: every window is clipped on both sides
    assert g < 2 or grid.moved > 100


@pytest.mark.parametrize("g", [40, 300])
def test_small_unfused(g):
    _small(g, gy=9)  # the unfused back end (rel rows stored), ceil(9 / 2) = 5 rows


@pytest.mark.parametrize("g", [130, 1100])
@pytest.mark.parametrize("flags", [KEEP, KEEP | pkg.abi.SS_FLAG_REFERENCE_NAN])
def test_zero_frame_and_the_nan_rows_behind_it(flags, g):
    """A -inf row, and with SS_FLAG_REFERENCE_NAN the NaN rows behind it, under windows of 131 and of 1101 bins."""
    real, grid, total = digest_tests._run(2048, "frames_cf32", flags=flags, g=g, nframes=200, sizes=(50,), max_batch=64, zero_frame=90, on=40)
    assert total > 1000


@pytest.mark.parametrize("g", [2048, 4096])
def test_wide_8192(g):
    real, grid, total = digest_tests._run(8192, "frames_cf32", g=g, nframes=100, sizes=(7, 64, 1, 100), grid_every=97)
    assert total > 1000 and _tx(real) > 50 and grid.moved > 100, (total, _tx(real), grid.moved)


def test_wide_8192_cs16_and_a_retune():
    real, grid, total = digest_tests._run(8192, "frames_cs16", fmt=pkg.abi.SS_FMT_CS16, g=2048, nframes=300, retune_after=3, grid_every=97)
    assert total > 1000 and _tx(real) > 50 and grid.moved > 100, (total, _tx(real), grid.moved)


def test_wide_65536_cs8():
    real, grid, total = digest_tests._run(65536, "frames_cs8", fmt=pkg.abi.SS_FMT_CS8, g=1600, nframes=64, sizes=(5, 32, 1), max_batch=32, grid_every=301)
    assert total > 1000 and _tx(real) > 50 and grid.moved > 100, (total, _tx(real), grid.moved)


def test_wide_2_20():
    """Windows of 4097 bins in rows of 2^20, batches of 16 and 4 frames so that the tail rows of either stand in front of the other.
    44 frames, not 20: the detect stage reports nothing before frame 26 (7 learning frames — learn_ms 280 at 40 ms a frame — and a
    21-frame averaging window), so a 20-frame stream has empty detected lists and nothing for the two trackers to compare. On this
    stream the oracle's planes give 133 to 218 candidates and 4 transmissions a frame from frame 26 on: 3736 and 72 after 44 frames.
    The grid lists' floor: in the 7 learning frames alone the only rows that qualify are the zero tail's (-100 is below the start
    level), all ties, whose first maximum is the window's first bin: each of those 7 x 257 grid candidates other than bin 0 moves."""
    real, grid, total = digest_tests._run(1 << 20, "frames_cf32", g=4096, nframes=44, sizes=(16, 4), max_batch=16, grid_every=4099, on=12)
    assert total > 1000 and _tx(real) > 50 and grid.moved > 1000, (total, _tx(real), grid.moved)


FEED_SHAPES = [(2048, 1100, 120, (7, 64, 1, 30), 64), (8192, 2048, 100, (7, 64, 1, 100), 128)]


@pytest.mark.parametrize("n,g,nframes,sizes,max_batch", FEED_SHAPES)
def test_feed_lockstep_wide(n, g, nframes, sizes, max_batch):
    """The feed's digest equals st_digest on a second engine, its transmissions the plane tracker's."""
    iq, t = feed_tests._stream(n, nframes=nframes)
    total, tx = feed_tests._lockstep(n, iq, t, sizes, g=g, max_batch=max_batch)
    assert total > 1000 and tx > 50, (total, tx)


@pytest.mark.parametrize("n,g,nframes,sizes,max_batch", FEED_SHAPES)
def test_feed_two_batches_in_flight_wide(n, g, nframes, sizes, max_batch):
    """Depth 3, two batches in flight: the watch list is K_p U cand_best(p + 1 .. k) (RouteB.collect holds it to that)."""
    iq, t = feed_tests._stream(n, nframes=nframes)
    a = feed_tests.RouteA(n, g, max_batch=max_batch, flags=KEEP)
    b = feed_tests.RouteB(n, g, max_batch=max_batch, flags=KEEP)
    cuts = feed_tests._batches(nframes, sizes)
    waiting, total, tx = [], 0, 0
    for k, (lo, hi) in enumerate(cuts):
        waiting.append((k, a.batch(iq[lo:hi], t[lo:hi])))
        b.submit(iq[lo:hi], t[lo:hi])
        while len(waiting) == 2 or (waiting and k == len(cuts) - 1):
            kk, ra = waiting.pop(0)
            got = b.collect(ra, f"batch {kk} {cuts[kk]}")
            total += got["cand_idx"].size
            tx += sum(len(x[0]) for x in ra["tx"])
    lags = sorted({s - p for s, (p, _) in b.at_submit.items()})
    b.close()
    print(f"in flight n {n} g {g}: {total} candidates, {tx} transmissions, lags {lags}")
    assert total > 1000 and tx > 50 and 2 in lags, (total, tx, lags)


def test_4096_bins_are_accepted_and_16384_refused():
    n, fs = 1024, 256_000
    eng = pkg.SpectrumEngine(fs, CENTER, fft_size=n, decim=1, max_batch=16, flags=KEEP, learn_ms=280)  # grouping_y 21: eleven rows
    eng.track_digest(4096).close()
    with pytest.raises(pkg.abi.SpecscanError) as e:
        eng.track_digest(1 << 14)  # (the row alone, 4 B a bin, is over 64 KiB)
    assert e.value.status == INVALID and "LDS" in str(e.value), str(e.value)
    feed = eng.feed(depth=3)
    with pytest.raises(pkg.abi.SpecscanError) as e:
        feed.track(1 << 14)
    assert e.value.status == INVALID and "LDS" in str(e.value), str(e.value)
    trk = feed.track(4096)
    # ... and the accepted width runs: one batch through the feed (both clips at n = 1024), its cand_best inside the windows
    iq, t = feed_tests._stream(n, nframes=16, on=8)
    buf = feed.acquire()
    buf[:16] = iq
    feed.submit(16, t_ms=t)
    got = trk.collect()
    assert got["digest_status"] == 0 and got["status"] == 0 and got["nframes"] == 16
    assert ((got["cand_best"] >= 0) & (got["cand_best"] < n)).all()
    trk.close()
    feed.close()
