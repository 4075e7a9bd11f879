"""specscan::RangePlanner (host/range_planner.h) through srp_* against recorder.RangePlanner, the oracle, without a GPU: seeded
random sessions of per-frame (shift, flush) lists — 1..4 slots, batches of 0..70 frames, 0..6 shifts a frame out of a pool of 8 that
stay for random spans, so recordings span batches and more shifts than slots occur — must give the same ranges, ends, flushes,
slot shifts and ignored sets after every batch. A plan of more than SC_MAX_RANGES ranges is refused and changes nothing.
tests/host/recording_check.cpp drives the two headers alone under the sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from rtl_sdr_scanner_cpp_amd import recorder
from rtl_sdr_scanner_cpp_amd.recorder import SC_MAX_RANGES, HostRangePlanner, RangePlanner
from test_scan_form import GXX_FLAGS, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "host")
POOL = (-412_500, -270_000, -100_000, -2_500, 0, 57_500, 182_500, 310_000)
SESSIONS = 240


def session(seed):
    """(slots, stride, [batch, ...]); batch = [frame, ...]; frame = [(shift, flush), ...] with distinct shifts."""
    rng = np.random.default_rng(seed)
    slots = int(rng.integers(1, 5))
    stride = int(rng.choice([256, 1024, 1280, 2048]))
    busy = float(rng.choice([0.02, 0.08, 0.3]))  # how often a new shift appears
    active, order, batches = {}, [], []
    for _ in range(int(rng.integers(3, 9))):
        batch = []
        for _ in range(0 if rng.random() < 0.12 else int(rng.integers(1, 71))):
            for s in [s for s in order if active[s] <= 0]:
                order.remove(s)
                del active[s]
            if len(order) < 6 and rng.random() < busy:
                s = int(rng.choice(POOL))
                if s not in active:
                    active[s] = int(rng.integers(3, 120))  # frames it stays: across batches more often than not
                    order.insert(int(rng.integers(0, len(order) + 1)), s)
            if rng.random() < 0.05:
                rng.shuffle(order)  # the tracker sorts by power: the order moves
            batch.append([(s, bool(rng.random() < 0.5)) for s in order])
            for s in order:
                active[s] -= 1
        batches.append(batch)
    return slots, stride, batches


def same_state(host, oracle):
    assert host.slots == oracle.slots
    assert host.ignored == oracle.ignored


def test_the_library_exports_the_bindings():
    lib = recorder._host_lib()
    assert [name for name in recorder.SRP_EXPORTS + recorder.SRS_EXPORTS if not hasattr(lib, name)] == []


def test_sessions_equal_the_python_planner():
    seen = {"ranges": 0, "stop": 0, "batch": 0, "flush": 0, "spanning": 0, "ignored": 0, "empty": 0, "refused": 0, "more_than_slots": 0}
    for seed in range(SESSIONS):
        slots, stride, batches = session(seed)
        host, oracle = HostRangePlanner(slots, stride), RangePlanner(slots, stride)
        for batch in batches:
            before = (host.slots, host.ignored)
            want = oracle.plan(batch)
            if len(want[0]) > SC_MAX_RANGES:  # the oracle has no limit; the C++ planner refuses and keeps its state: the session ends
                with pytest.raises(ValueError, match="smaller batch"):
                    host.plan(batch)
                assert (host.slots, host.ignored) == before
                seen["refused"] += 1
                break
            got = host.plan(batch)
            assert got == want, (seed, got, want)
            same_state(host, oracle)
            seen["ranges"] += len(want[0])
            seen["stop"] += want[1].count("stop")
            seen["batch"] += want[1].count("batch")
            seen["flush"] += sum(want[2])
            seen["spanning"] += sum(1 for r, why in zip(*want[:2]) if why == "batch" and r[2] == 0 and len(batch) > 1)
            seen["ignored"] += bool(oracle.ignored)
            seen["empty"] += not batch
            seen["more_than_slots"] += any(len(f) > slots for f in batch)
        host.close()
    print(seen)
    assert SESSIONS >= 200 and seen["ranges"] > 2000 and min(seen[k] for k in ("stop", "batch", "flush", "spanning", "ignored", "empty", "more_than_slots")) > 20, seen


def test_more_than_sc_max_ranges_is_refused_and_changes_nothing():
    host, oracle = HostRangePlanner(1, 1024), RangePlanner(1, 1024)
    first = [[(57_500, True)]] * 3
    assert host.plan(first) == oracle.plan(first)
    before = (host.slots, host.ignored)
    assert before[0] == [{"rec": True, "shift": 57_500}]
    # one slot that stops and starts every other frame: 1 range from the last batch and 65 more
    frames = [[(57_500, False)], []] + [[(s, True)] if f % 2 == 0 else [] for f, s in zip(range(130), [0, 0, 310_000, 310_000] * 33)]
    assert len(oracle.plan(frames)[0]) == 66 > SC_MAX_RANGES
    with pytest.raises(ValueError, match="SC_MAX_RANGES.*smaller batch"):
        host.plan(frames)
    assert (host.slots, host.ignored) == before
    half = frames[:64]  # the same frames in two plans are taken
    oracle2 = RangePlanner(1, 1024)
    oracle2.plan(first)
    for part in (half, frames[64:]):
        assert host.plan(part) == oracle2.plan(part)
    same_state(host, oracle2)
    with pytest.raises(ValueError):
        HostRangePlanner(0, 1024)
    with pytest.raises(ValueError):
        HostRangePlanner(17, 1024)
    with pytest.raises(ValueError):
        HostRangePlanner(2, 0)


def test_the_two_classes_are_plain_cpp():
    import re
    for name in ("range_planner.h", "recording_store.h"):
        text = open(os.path.join(HOST, name)).read()
        included = re.findall(r"#\s*include\s*[<\"]([^>\"]+)", text)
        assert not [h for h in included if h.startswith("hip") or h in ("specscan.h", "specscan_record_feed.h")] and "hipError_t" not in text, (name, included)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("recording") / "recording_check")
    subprocess.run([gxx, *GXX_FLAGS, "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-o", exe, os.path.join(ROOT, "tests", "host", "recording_check.cpp")],
                   check=True)
    return exe


def test_recording_check_under_the_sanitizers(check):
    """A fresh process, no Python in it: every plan passes chan_ranges::validate and covers each recording's frames exactly once; the
    store cuts what it is fed into items and loses nothing."""
    lines = _run([check])
    print("\n".join(lines[-3:]))
    last = lines[-1].split()  # sessions <n> batches <n> ranges <n> refused <n> items <n> bad <b>
    assert last[0::2] == ["sessions", "batches", "ranges", "refused", "items", "bad"], last
    sessions, batches, ranges, refused, items, bad = (int(v) for v in last[1::2])
    assert sessions >= 200 and batches > 1000 and ranges > 2000 and refused > 0 and items > 100 and bad == 0, last
