"""The 64-bit digest units (MSPACK_HIP_KIND_SHA384 / _SHA512 with their two / three MSPACK_HIP_KIND_DIGEST_MORE tails) in the host
path's planner (libmspack_amd/csrc/hip/host_plan.hpp: plan_batch, plan_shards), stand-alone under AddressSanitizer + UBSan like
tests/test_host_plan_sha.py: tests/hostcheck/plan_sha512_check.cpp is a program of its own that includes that header alone.  All five
hashes and CRC-32 ranges mixed in one table: a head keeps all its tails at i + 1 .. behind the chunks; the order list ends in four
lists of heads (SHA-384 and SHA-512 together in the fourth, longest first) and the range list, and everything in front of the fourth
list is what the table without the new kinds gives; no shard is cut inside a range and a head and its tails land in one shard; every
rejection with its message (SHA-384 with 1 tail, SHA-512 with 2, SHA-256 with 2, a tail naming bytes, a lone tail, kinds 21 to 23
unknown); and the plans of tables without the new kinds are byte for byte those of tests/golden/plan_parent.txt."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
CASES = ["tails_follow", "five_kinds_lists", "shard_cuts", "rejections"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def plan_sha512_check():
    if not os.path.exists(CXX):
        pytest.skip("no clang with sanitizer runtimes")
    out = os.path.join(ROOT, "tests", "_build", "plan_sha512_check")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    p = subprocess.run([CXX, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "libmspack_amd", "csrc", "hip"),
                        os.path.join(ROOT, "tests", "hostcheck", "plan_sha512_check.cpp"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-4000:]
    return out


def run(binary, arg):
    p = subprocess.run([binary, arg], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out and "PLAN_FAIL" not in out, out[-4000:]
    return out


def test_case_list_is_complete(plan_sha512_check):
    assert run(plan_sha512_check, "list").split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_plan(plan_sha512_check, case):
    assert ("PLAN_OK " + case) in run(plan_sha512_check, case)


def test_plans_without_the_new_kinds_are_the_parents(plan_sha512_check):
    want = open(os.path.join(ROOT, "tests", "golden", "plan_parent.txt")).read()
    assert len(want.splitlines()) == 31
    assert run(plan_sha512_check, "dump") == want
