"""What one call decides (csrc/call_route.h: CallAsk, CallRoute, decide_call), without a GPU. tests/host/call_route_check.cpp is a
stand-alone program built with g++ under the sanitizers: it walks forms and asks and asserts what the code's comments promise of a route,
and it prints, for the calls scripts/record_call_route.py recorded, what decide_call decides: it must be what run_batch of the commit
before it decided on an MI355X (tests/golden/call_route_parent.json), in every field."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

from test_scan_form import GXX_FLAGS, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FIXTURE = os.path.join(ROOT, "tests", "golden", "call_route_parent.json")


def recorder():
    spec = importlib.util.spec_from_file_location("record_call_route", os.path.join(ROOT, "scripts", "record_call_route.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("call_route") / "call_route_check")
    subprocess.run([gxx, *GXX_FLAGS, "-o", exe, os.path.join(HOST, "call_route_check.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fp:
        return json.load(fp)


def test_the_route_is_plain_cpp():
    text = open(os.path.join(CSRC, "call_route.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", text) and "hipError_t" not in text and "getenv" not in text
    assert re.findall(r"#\s*include\s*[<\"]([^>\"]+)", text) == ["ring_place.h", "scan_form.h"]
    assert re.search(r"CallRoute decide_call\(const ScanForm& \w+, const Diag& \w+, uint32_t \w+, const CallAsk& \w+\)", text)


def test_the_step_branch_reads_the_route():
    """run_batch holds none of the nine predicate definitions and no chunk loop of its own; one function holds the one loop"""
    text = open(os.path.join(CSRC, "specscan.hip")).read()
    body = text.split("\nint run_batch(", 1)[1].split("\n}\n", 1)[0]
    for name in "keeps_no_plane ring_room dif_call db_call cull_call ring_by_rows ring_only overlap merged_call plan_fused".split():
        assert not re.search(r"\bbool " + name + r"\b", body), name
    assert "for (int f0" not in body and text.count("for (int f0") == 1
    assert "ring_room" not in text and "without a place for its rows" not in text


def test_route_check_under_the_sanitizers(check):
    lines = _run([check])
    print("\n".join(lines[-5:]))
    last = lines[-1].split()  # forms <n> spec_forms <n> asks <n> bad <b>
    assert last[0::2] == ["forms", "spec_forms", "asks", "bad"], last
    forms, spec_forms, asks, bad = (int(v) for v in last[1::2])
    # 8 sizes x 2 formats x 2 windows x 32 flag combinations x 2 batch sizes (16 and 1024: at 1024 a batch has its room in the ring from
    # decide_form's "three batches and three windows" line, not from the 1024-row floor: without that line the check fails 30704 times);
    # the product's choices and each of the ten switches alone
    assert forms == 8 * 2 * 2 * 32 * 2 * 11 and spec_forms == forms // 2
    # 12 frame counts x 3 learning counts x 8 subsets of planes x device or host call, and with and without the container where there is one
    assert asks == (forms + spec_forms) * 12 * 3 * 8 * 2 and bad == 0, last


def test_the_fixture_holds_the_sessions_of_the_script(fixture):
    assert os.path.getsize(FIXTURE) < 300_000
    rec = recorder()
    assert fixture["fields"] == rec.FIELDS and fixture["sessions_sha256"] == rec.sessions_digest()
    assert len(fixture["calls"]) == len(rec.sessions()) and all(len(calls) >= 10 for calls in fixture["calls"])
    assert sorted({k for calls in fixture["calls"] for k in calls}) == list(range(len(fixture["lines"]))) and len(set(fixture["lines"])) == len(fixture["lines"])
    assert rec.complete(fixture["lines"]) == []  # every shape, and both values of every predicate


def test_routes_are_the_parents(check, fixture, tmp_path):
    rec = recorder()
    cases, want = [], []
    for session, calls in zip(rec.sessions(), fixture["calls"]):
        for k in sorted(set(calls)):
            kv = rec.parse(fixture["lines"][k])
            cases.append(rec.case_line(session) + " | " + " ".join(kv[name] for name in rec.ASK))
            want.append(fixture["lines"][k])
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(cases) + "\n")
    got = _run([check, "--cases", str(path)])
    assert len(got) == len(want) > 100
    for case, g, w in zip(cases, got, want):
        assert g == w, (case, {name: (a, b) for (name, a), b in zip(rec.parse(g).items(), rec.parse(w).values()) if a != b})
