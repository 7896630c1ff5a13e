"""Stored units (MSPACK_HIP_KIND_STORED) in the host path's planner (libmspack_amd/csrc/hip/host_plan.hpp: plan_batch, plan_shards),
stand-alone under AddressSanitizer + UBSan like tests/test_host_plan_crc32r.py: tests/hostcheck/plan_stored_check.cpp is a program of
its own that includes that header alone.  Stored units are accepted, own exactly their bytes (no slack, nothing below), have a compact
list of their own behind the other kinds', weigh their bytes when chunks and shards are cut; a unit that leaves an arena is refused
with a message that names it; kinds 9, 10 and 12 are still unknown; and the plans of tables without the new kind are byte for byte those of
tests/golden/plan_parent.txt."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CASES = ["accepted_and_listed", "chunks_by_bytes", "rejections"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def plan_stored_check():
    if not os.path.exists(CXX):
        pytest.skip("no clang with sanitizer runtimes")
    out = os.path.join(ROOT, "tests", "_build", "plan_stored_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    p = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "libmspack_amd", "csrc", "hip"),
                        os.path.join(ROOT, "tests", "hostcheck", "plan_stored_check.cpp"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    return out


def run(binary, arg):
    p = subprocess.run([binary, arg], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out and "PLAN_FAIL" not in out, out[-4000:]
    return out


def test_case_list_is_complete(plan_stored_check):
    assert run(plan_stored_check, "list").split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_plan(plan_stored_check, case):
    assert ("PLAN_OK " + case) in run(plan_stored_check, case)


def test_plans_without_the_new_kind_are_the_parents(plan_stored_check):
    want = open(os.path.join(ROOT, "tests", "golden", "plan_parent.txt")).read()
    assert len(want.splitlines()) == 31
    assert run(plan_stored_check, "dump") == want
