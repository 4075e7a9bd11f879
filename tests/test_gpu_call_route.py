"""run_batch follows what decide_call names (csrc/call_route.h): the sessions of scripts/record_call_route.py once more, on the built
diagnostics library with SS_ROUTE_RECORD set — the lines each call leaves must be the ones the commit before call_route.h left on an
MI355X (tests/golden/call_route_parent.json), call by call. Every session is a dozen short calls in a child process of its own, under
that script's time limit. Run with -m gpu."""
import json

import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from test_call_route import FIXTURE, recorder

pytestmark = pytest.mark.gpu

REC = recorder()


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fp:
        return json.load(fp)


@pytest.mark.parametrize("k", range(len(REC.sessions())), ids=[REC.case_line(s).replace(" ", "_") for s in REC.sessions()])
def test_the_calls_of_a_session_take_the_parents_routes(fixture, k):
    got = REC.record_sessions(pkg.build.LIB_DIAG, which=[k])[k]
    want = [fixture["lines"][i] for i in fixture["calls"][k]]
    assert len(got) == len(want)
    for call, (g, w) in enumerate(zip(got, want)):
        assert g == w, (call, {name: (a, b) for (name, a), b in zip(REC.parse(g).items(), REC.parse(w).values()) if a != b})
