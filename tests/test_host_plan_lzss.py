"""LZSS units with MSPACK_HIP_UF_LZSS_RING in the host path's planner (libmspack_amd/csrc/hip/host_plan.hpp: plan_batch, plan_shards),
stand-alone under AddressSanitizer + UBSan like tests/test_host_plan_md5.py: tests/hostcheck/plan_lzss_check.cpp includes that header
alone.  Flagged units get no room below in the batch's span, the chunks' spans and the shards' regions (out_off 0 is legal); unflagged
LZSS units and LZH units still get 4096; a chunk asks for the ring kernel exactly when it holds a flagged unit -- the condition under
which launch.hpp launches it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CASES = ["below", "chunks", "shards"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def plan_lzss_check():
    if not os.path.exists(CXX):
        pytest.skip("no clang with sanitizer runtimes")
    out = os.path.join(ROOT, "tests", "_build", "plan_lzss_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    p = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "libmspack_amd", "csrc", "hip"),
                        os.path.join(ROOT, "tests", "hostcheck", "plan_lzss_check.cpp"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    return out


def run(binary, arg):
    p = subprocess.run([binary, arg], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out and "PLAN_FAIL" not in out, out[-4000:]
    return out


def test_case_list_is_complete(plan_lzss_check):
    assert run(plan_lzss_check, "list").split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_plan(plan_lzss_check, case):
    assert ("PLAN_OK " + case) in run(plan_lzss_check, case)
