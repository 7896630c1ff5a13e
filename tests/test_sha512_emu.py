"""MSPACK_HIP_KIND_SHA384 / _SHA512 on the wavefront emulator (tests/emu/): the kernel's logic -- the shared loader's three paths with
128-byte blocks and big-endian 64-bit words, ragged heads and tails, the pad's one or two final blocks with the 128-bit big-endian bit
length, the 64-bit rotates made of 32-bit funnel shifts, the initial state picked per lane, lanes whose loops end at different counts,
the head's lane writing its two or three tails' results -- without a GPU.  Runs the first four groups of tests/test_gpu_sha512.py
(lengths x alignments, the FIPS 180-4 strings, 65 ranges in one table, the arena's edges inside guard bytes) against
tests/_build/libmspack_emu.so in a child process."""
import os
import subprocess
import sys

import pytest

from helpers import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_sha512_parity_tests_on_the_emulator(built):
    so = emu_so()
    ids = ["tests/test_gpu_sha512.py::test_lengths_and_alignments", "tests/test_gpu_sha512.py::test_fips_strings",
           "tests/test_gpu_sha512.py::test_65_ranges_of_different_lengths", "tests/test_gpu_sha512.py::test_arena_edges_and_guards"]
    env = dict(os.environ, MSPACK_HIP_SO=so)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1700)
    assert p.returncode == 0 and b"6 passed" in p.stdout, p.stdout.decode()[-3000:]
