"""How four-byte samples reach the threads of the radix-8 / radix-16 fold (csrc/fold_cs16_staging.h), without a GPU:
tests/host/fold_cs16_staging_check.cpp walks the functions the kernels call over a model frame and a model LDS array — every sample
fetched once, nothing outside the frame or the piece, thread t's read for (rho, q) is sample t + 512 rho + 8192 q, no place refetched
before its last read or read before its fetch was waited for behind a barrier — as a stand-alone program under the address and
undefined-behaviour sanitizers. (That the kernels hand those functions the arguments the walk uses is what the bit identity of
tests/test_gpu_fold_cs16.py shows on the GPU.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-sdr-scanner-cpp_amd", "csrc")


def test_staging_check_program_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "fold_cs16_staging_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "host", "fold_cs16_staging_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == "all ok" and "FAIL" not in out.stdout


def test_the_staging_header_is_plain_cxx_and_the_fold_includes_it():
    staging = open(os.path.join(CSRC, "fold_cs16_staging.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", staging)  # plain C++: the check compiles it with g++
    assert '#include "fold_cs16_staging.h"' in open(os.path.join(CSRC, "fft65536_dif8.h")).read()
