"""Which form of the pipeline a configuration gets, and what a context of that form allocates, without a GPU.

csrc/scan_form.h (the choices, the form, decide_form) is plain C++; csrc/ctx_buffers.h (the sized buffers of a context) needs
device_buffers.h and a HIP runtime, for which tests/host/fake_hip stands in. Two stand-alone checks, built with g++ under the sanitizers:
tests/host/scan_form_check.cpp walks the configuration space and asserts what the code's comments promise of the form;
tests/host/ctx_buffers_check.cpp allocates six forms with a failure injected at every call in turn. Both also print, for the case lines
of scripts/record_scan_form.py, what they decide and allocate: it must be what the commit before them decided and allocated on an
MI355X (tests/golden/scan_form_parent.json), in every field and in the multiset of sizes."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "host")
FIXTURE = os.path.join(ROOT, "tests", "golden", "scan_form_parent.json")
GXX_FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSS_DIAG"]
# (name in ctx_buffers_check.cpp, case line): the six forms that check allocates, all at 64 frames
SIX_FORMS = {"8192_deep": "8192 2048000 0 0 0 21 21 64", "8192_spectrogram": "8192 2048000 0 0 2 21 21 64", "65536_cs8_fold": "65536 16384000 1 0 0 21 21 64",
             "262144_merged": "262144 65536000 0 0 0 21 21 64", "1048576_two_pass": "1048576 262144000 0 0 0 21 21 64", "256_5x3_unfused": "256 64000 0 0 0 5 3 64"}


def _recorder():
    spec = importlib.util.spec_from_file_location("record_scan_form", os.path.join(ROOT, "scripts", "record_scan_form.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def checks(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not found")
    out = tmp_path_factory.mktemp("scan_form")
    exes = {}
    for name, extra in (("scan_form_check", []), ("ctx_buffers_check", ["-I" + os.path.join(HOST, "fake_hip")])):
        exes[name] = str(out / name)
        subprocess.run([gxx, *GXX_FLAGS, *extra, "-o", exes[name], os.path.join(HOST, name + ".cpp")], check=True)
    exes["dir"] = str(out)
    return exes


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fp:
        return json.load(fp)


def _run(cmd):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    out = subprocess.run(cmd, capture_output=True, text=True, env={k: v for k, v in env.items() if not k.startswith("SS_")})
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    return out.stdout.strip().splitlines()


def test_the_form_is_plain_cpp():
    text = open(os.path.join(CSRC, "scan_form.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", text) and "hipError_t" not in text and "hipMalloc" not in text
    assert re.search(r"int decide_form\(const ss_config& \w+, const Diag& \w+, ScanForm& \w+, char\* \w+\)", text)
    read = text.split("void read() {", 1)[1].split("#else", 1)[0]
    assert "getenv" in read and "getenv" not in text.replace(read, "")  # the environment is read under SS_DIAG only, and nowhere else
    assert text.index("#ifdef SS_DIAG") < text.index("void read() {")


def test_only_the_owners_free_and_destroy():
    calls = re.compile(r"\b(hipFree|hipHostFree|hipEventDestroy|hipStreamDestroy)\b")
    named = {name for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip")) and calls.search(open(os.path.join(CSRC, name)).read())}
    assert named == {"device_buffers.h"}, named
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")):
            text = open(os.path.join(CSRC, name)).read()
            assert not re.search(r"\b(free_ctx|free_sc|CREATE_HIP|SC_CREATE_HIP)\b", text), name


def test_form_check_under_the_sanitizers(checks):
    lines = _run([checks["scan_form_check"]])
    print("\n".join(lines[-5:]))
    last = lines[-1].split()  # configs <n> forms <n> refused <n> bad <b>
    assert last[0::2] == ["configs", "forms", "refused", "bad"], last
    configs, forms, refused, bad = (int(v) for v in last[1::2])
    # 15 sizes x 2 formats x 2 windows x 32 flag combinations x 2 groupings x 3 batch sizes; the product's choices, every switch alone
    # and 300 random combinations for each
    assert configs == 15 * 2 * 2 * 32 * 2 * 3 and forms >= configs * 320 and refused > 0 and bad == 0, last


def test_buffers_check_under_the_sanitizers(checks, fixture):
    lines = _run([checks["ctx_buffers_check"]])
    print("\n".join(line[:200] for line in lines))
    last = lines[-1].split()  # forms <n> runs <n> bad <b>
    assert last[0::2] == ["forms", "runs", "bad"] and int(last[1]) == 6 and int(last[3]) > 6 * 40 and last[-1] == "0", last
    recorded = _recorded(fixture)
    seen = {}
    for line in lines[:-1]:
        _, name, sizes = line.split()
        seen[name] = sorted(int(v) for v in sizes.split(","))
    assert set(seen) == set(SIX_FORMS)
    for name, case in SIX_FORMS.items():
        assert seen[name] == recorded[case][1], name


def _recorded(fixture):
    """case line -> (values by field | [status, text], sorted sizes | None); the lines are those of the script, in its order"""
    out = {}
    for line, k in zip(_recorder().cases(), fixture["form_of_case"]):
        if k < 0:
            continue
        values, sizes = fixture["values"][fixture["forms"][k][0]], fixture["sizes"][fixture["forms"][k][1]]
        if sizes is not None:  # "bytes*count bytes ...", as run_lengths of the script wrote it
            sizes = sorted(int(value) for value, _, count in (item.partition("*") for item in sizes.split()) for _ in range(int(count or 1)))
        out[line] = (values, sizes)
    return out


def test_the_fixture_holds_the_cases_of_the_script(fixture):
    assert os.path.getsize(FIXTURE) < 300_000
    rec = _recorder()
    lines = rec.cases()
    assert fixture["fields"] == rec.FIELDS and fixture["cases_sha256"] == rec.cases_digest()
    assert len(fixture["form_of_case"]) == len(lines) == len(set(lines))
    assert fixture["dropped"] == [k for k, form in enumerate(fixture["form_of_case"]) if form < 0]
    assert all(rec.upper_bound_bytes(lines[k]) > rec.SIZE_LIMIT for k in fixture["dropped"])
    assert sorted(set(fixture["form_of_case"]) - {-1}) == list(range(len(fixture["forms"])))
    assert all(0 <= v < len(fixture["values"]) and 0 <= z < len(fixture["sizes"]) for v, z in fixture["forms"])
    assert set(SIX_FORMS.values()) <= set(_recorded(fixture))


def test_form_and_sizes_are_the_parents(checks, fixture):
    recorded = _recorded(fixture)
    lines = sorted(recorded)
    path = os.path.join(checks["dir"], "cases.txt")
    with open(path, "w") as fp:
        fp.write("\n".join(lines) + "\n")
    forms = _run([checks["scan_form_check"], "--cases", path])
    sizes = _run([checks["ctx_buffers_check"], "--cases", path])
    assert len(forms) == len(lines) == len(sizes) and len(lines) > 2000
    rec = _recorder()
    refused = 0
    for line, form, size in zip(lines, forms, sizes):
        want_values, want_sizes = recorded[line]
        got_values, _ = rec.parse(form)
        assert got_values == want_values, (line, dict(zip(fixture["fields"], zip(got_values, want_values))))
        if want_sizes is None:
            refused += 1
            assert size == "refused", line
        else:
            assert sorted(int(v) for v in size.split("=", 1)[1].split(",")) == want_sizes, line
    assert refused > 0  # (SS_FLAG_REFERENCE_NAN with another grouping: the same status and text, before anything is allocated)
