"""MSPACK_HIP_UF_CRC32 on the wavefront emulator (tests/emu/): the digest kernels' logic -- table build, slices, the lane tree, ragged
heads and tails, segment shares, the compare-and-swap XOR -- without a GPU.  Runs the first three tests of tests/test_gpu_crc32.py
against tests/_build/libmspack_emu.so in a child process; the 64 MiB units and the 4096-unit batch stay with the GPU."""
import os
import subprocess
import sys

import pytest

from helpers import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_crc32_parity_tests_on_the_emulator(built):
    so = emu_so()
    ids = ["tests/test_gpu_crc32.py::test_mixed_batch_of_all_six_kinds",
           "tests/test_gpu_crc32.py::test_lengths_and_alignments",
           "tests/test_gpu_crc32.py::test_damaged_streams"]
    env = dict(os.environ, MSPACK_HIP_SO=so)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1700)
    assert p.returncode == 0 and b"3 passed" in p.stdout, p.stdout.decode()[-3000:]
