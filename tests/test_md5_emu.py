"""MSPACK_HIP_KIND_MD5 on the wavefront emulator (tests/emu/): the digest kernel's logic -- the three loaders, ragged heads and tails,
the pad's one or two final blocks, lanes whose loops end at different counts, the guard against ranges that leave the arena --
without a GPU.  Runs the first three groups of tests/test_gpu_md5.py (lengths and alignments with the RFC 1321 strings, batch
shapes, edges and guards) against tests/_build/libmspack_emu.so in a child process; the 1 MiB range stays with the GPU."""
import os
import subprocess
import sys

import pytest

from helpers import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_md5_parity_tests_on_the_emulator(built):
    so = emu_so()
    ids = ["tests/test_gpu_md5.py::test_lengths_and_alignments", "tests/test_gpu_md5.py::test_rfc1321_strings",
           "tests/test_gpu_md5.py::test_batch_shapes", "tests/test_gpu_md5.py::test_arena_edges_and_guards"]
    env = dict(os.environ, MSPACK_HIP_SO=so)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1700)
    assert p.returncode == 0 and b"8 passed" in p.stdout, p.stdout.decode()[-3000:]
