"""The host path's chunk planner asked what plan it makes (libmspack_amd/csrc/hip/host_plan.hpp: plan_batch, a pure function of the
unit table and a PlanKnobs).  tests/hostcheck/plan_check.cpp includes that header alone -- no HIP, no emulator headers -- and is built
here with AddressSanitizer + UBSan by the clang tests/test_hostcheck.py uses.  Every case is a hand-built unit table, the smallest at
which its rule can go wrong; every accepted plan is also checked against the general invariants (plan_check.cpp: check_plan): the chunks
are consecutive ranges over the units in ascending in_off, each chunk's per-kind lists partition its units of that kind longest first,
its spans hold its units' streams, side tables and output regions, and the rebased offsets reproduce the caller's.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CASES = ["one_unit", "shapes", "unit_cap", "mixed_kinds", "chm_style", "xorsum_only", "not_monotone", "crc_lists", "rejections"]


@pytest.fixture(scope="module")
def plan_check():
    if not os.path.exists(CXX):
        pytest.skip("no clang with sanitizer runtimes")
    out = os.path.join(ROOT, "tests", "_build", "plan_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    p = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "libmspack_amd", "csrc", "hip"),
                        os.path.join(ROOT, "tests", "hostcheck", "plan_check.cpp"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    return out


def test_case_list_is_complete(plan_check):
    p = subprocess.run([plan_check, "list"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_plan(plan_check, case):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([plan_check, case], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and ("PLAN_OK " + case) in out, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out and "PLAN_FAIL" not in out, out[-4000:]
