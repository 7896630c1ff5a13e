"""MSPACK_HIP_KIND_SHA1 / _SHA256 on the wavefront emulator (tests/emu/): the digest kernels' logic -- the shared loader's three paths
with big-endian words, ragged heads and tails, the pad's one or two final blocks with the big-endian bit length, lanes whose loops
end at different counts, the head's lane writing its tail's result -- without a GPU.  Runs the first three groups of
tests/test_gpu_sha.py (lengths and alignments, the FIPS 180-4 strings, batch shapes) against tests/_build/libmspack_emu.so in a
child process."""
import os
import subprocess
import sys

import pytest

from helpers import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_sha_parity_tests_on_the_emulator(built):
    so = emu_so()
    ids = ["tests/test_gpu_sha.py::test_lengths_and_alignments", "tests/test_gpu_sha.py::test_fips_strings",
           "tests/test_gpu_sha.py::test_batch_shapes"]
    env = dict(os.environ, MSPACK_HIP_SO=so)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1700)
    assert p.returncode == 0 and b"13 passed" in p.stdout, p.stdout.decode()[-3000:]
