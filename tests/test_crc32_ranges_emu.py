"""MSPACK_HIP_KIND_CRC32 on the wavefront emulator (tests/emu/): the range pass's logic -- the results' start values, the one-wave scan,
the control unit, the search for a chunk's first ticket over blocks with and without range units, the walk, the XOR of the shares,
the tidying up -- without a GPU.  Runs the first groups of tests/test_gpu_crc32_ranges.py against tests/_build/libmspack_emu.so in a
child process; the batches behind the decoders stay with the GPU."""
import os
import subprocess
import sys

import pytest

from helpers import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_crc32_range_tests_on_the_emulator(built):
    so = emu_so()
    ids = ["tests/test_gpu_crc32_ranges.py::test_lengths_and_alignments",
           "tests/test_gpu_crc32_ranges.py::test_mixed_sizes_in_one_table",
           "tests/test_gpu_crc32_ranges.py::test_range_units_among_other_units_of_the_table",
           "tests/test_gpu_crc32_ranges.py::test_arena_edges_and_guards"]
    env = dict(os.environ, MSPACK_HIP_SO=so)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1700)
    assert p.returncode == 0 and b"4 passed" in p.stdout, p.stdout.decode()[-3000:]
