"""Wide digest units (MSPACK_HIP_KIND_SHA1 / _SHA256 and their MSPACK_HIP_KIND_DIGEST_MORE tails) in the host path's planner
(libmspack_amd/csrc/hip/host_plan.hpp: plan_batch, plan_shards), stand-alone under AddressSanitizer + UBSan like
tests/test_host_plan_md5.py: tests/hostcheck/plan_sha_check.cpp includes that header alone.  Heads keep their tails at i + 1 behind the
chunks; the order list ends in three lists of heads, one per algorithm, each longest first, and the MD5 list of a mixed table is that of
the same table without the SHA units; no shard is cut inside a range and a head and its tail land in one shard; every rejection with
its message."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CASES = ["tails_follow", "three_lists", "shard_cuts", "rejections"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def plan_sha_check():
    if not os.path.exists(CXX):
        pytest.skip("no clang with sanitizer runtimes")
    out = os.path.join(ROOT, "tests", "_build", "plan_sha_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    p = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "libmspack_amd", "csrc", "hip"),
                        os.path.join(ROOT, "tests", "hostcheck", "plan_sha_check.cpp"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    return out


def run(binary, arg):
    p = subprocess.run([binary, arg], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out and "PLAN_FAIL" not in out, out[-4000:]
    return out


def test_case_list_is_complete(plan_sha_check):
    assert run(plan_sha_check, "list").split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_plan(plan_sha_check, case):
    assert ("PLAN_OK " + case) in run(plan_sha_check, case)
