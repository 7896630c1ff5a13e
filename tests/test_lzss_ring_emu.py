"""MSPACK_HIP_UF_LZSS_RING on the wavefront emulator (tests/emu/): the ring kernel's logic -- the stage's refills, the scalar chain of
group starts, items in stream order on the ring, the flushes in whole rows with ragged heads and tails, the room -- without a GPU.
Runs the first three tests of tests/test_gpu_lzss_ring.py against tests/_build/libmspack_emu.so in a child process."""
import os
import subprocess
import sys

import pytest

from helpers import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_lzss_ring_parity_tests_on_the_emulator(built):
    so = emu_so()
    ids = ["tests/test_gpu_lzss_ring.py::test_corpus_vs_oracle",
           "tests/test_gpu_lzss_ring.py::test_crafted_streams",
           "tests/test_gpu_lzss_ring.py::test_room_cut_at_every_length"]
    env = dict(os.environ, MSPACK_HIP_SO=so)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1700)
    assert p.returncode == 0 and b"3 passed" in p.stdout, p.stdout.decode()[-3000:]
