"""Digest units (MSPACK_HIP_KIND_MD5) in the host path's planner (libmspack_amd/csrc/hip/host_plan.hpp: plan_batch, plan_shards), stand-alone
under AddressSanitizer + UBSan like tests/test_host_plan.py: tests/hostcheck/plan_md5_check.cpp includes that header alone.  Digest units
carry no weight in the chunk cutting and stand behind the chunks; their list is longest first; a shard cut that would fall inside a digest
range is moved; the three rejections; and the plans of plan_check.cpp's nine cases, which hold no digest unit, are those recorded from the
planner before digest units existed (tests/golden/plan_parent.txt)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CASES = ["no_weight", "longest_first", "md5_only", "shard_cuts", "rejections"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def plan_md5_check():
    if not os.path.exists(CXX):
        pytest.skip("no clang with sanitizer runtimes")
    out = os.path.join(ROOT, "tests", "_build", "plan_md5_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    p = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "libmspack_amd", "csrc", "hip"),
                        os.path.join(ROOT, "tests", "hostcheck", "plan_md5_check.cpp"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    return out


def run(binary, arg):
    p = subprocess.run([binary, arg], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out and "PLAN_FAIL" not in out, out[-4000:]
    return out


def test_case_list_is_complete(plan_md5_check):
    assert run(plan_md5_check, "list").split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_plan(plan_md5_check, case):
    assert ("PLAN_OK " + case) in run(plan_md5_check, case)


def test_plans_without_digest_units_are_the_parents(plan_md5_check):
    want = open(os.path.join(ROOT, "tests", "golden", "plan_parent.txt")).read()
    assert len(want.splitlines()) == 31
    assert run(plan_md5_check, "dump") == want
