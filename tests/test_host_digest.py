"""What the cabinet and the CHM driver share of their digest code (libmspack_amd/csrc/host/host_digest.h), as pure functions on the CPU:
the emitter of one file's digest units and the table of the digests a batch took -- its harvest from units and results (the head / tail
layout of include/mspack_hip.h) and its lookup.  tests/csrc/digest_table_check.c includes that header alone, is built with
-fsanitize=address,undefined and runs as a program of its own, one case per call; any sanitizer report fails the case."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
       "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "include")]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")
HARVEST_CASES = ["empty_batch", "one_md5", "sha1_head_and_tail", "sha256_head_and_tail", "head_error_drops", "tail_error_drops_head",
                 "wide_head_last", "tail_at_index_0", "three_algorithms", "same_offset_two_lengths", "length_off_by_one", "descending_units",
                 "ascending_units_take_no_sort", "second_harvest", "probe_behind_last_hit", "rebase_subtract", "rebase_add_past_4gib"]
EMIT_CASES = ["emit_mask_0", "emit_md5_only", "emit_mask_7", "emit_ratio_edge", "emit_cap_too_small", "emit_counts_only", "units_per_file"]
CASES = HARVEST_CASES + EMIT_CASES


@pytest.fixture(scope="module")
def table_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("digest_table") / "digest_table_check")
    host = os.path.join(ROOT, "libmspack_amd", "csrc", "host")
    subprocess.check_call(["gcc"] + SAN + ["-Wextra", "-Werror", "-I", host, "-o", exe, os.path.join(HERE, "csrc", "digest_table_check.c"),
                                           os.path.join(host, "md5.c"), os.path.join(host, "sha.c")])
    return exe


def test_case_list_is_complete(table_check):
    p = subprocess.run([table_check, "list"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and p.stdout.decode().split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_digest_table_and_emitter(table_check, case):
    p = subprocess.run([table_check, case], env=dict(os.environ, **SAN_ENV), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and ("TABLE_OK " + case) in out, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out and "TABLE_FAIL" not in out, out[-4000:]
