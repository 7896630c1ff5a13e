"""MSPACK_HIP_KIND_STORED on the wavefront emulator (tests/emu/): the kernel source of libmspack_amd/csrc/hip/stored_kernel.hpp -- the
one-wave scan, the control unit, the search for a chunk's first ticket over blocks with and without stored units, the walk, the row
copy with its realigned loads, the byte-wise first and last rows, the results -- without a GPU.  Runs tests/test_gpu_stored.py against
tests/_build/libmspack_emu.so in a child process: the lengths 0 .. 200 003 at (in_off, out_off) mod 16 in {0, 1, 7, 15}^2 between
neighbours that share their first and last rows and between canary bytes, short inputs, units that leave an arena, 300 small units
around one of 1 MiB, order lists, the masks -- and the host entry points' groups, which the emulator's runtime carries too."""
import os
import subprocess
import sys

import pytest

from helpers import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
KERNEL = ["test_lengths_and_alignments", "test_short_input_and_arena_edges", "test_many_units_and_a_long_one",
          "test_stored_units_among_other_units_of_the_table", "test_kind_mask"]
HOST = ["test_decode_batch_shapes", "test_rejections", "test_mixed_batch", "test_one_big_unit_beside_a_thousand_small_ones",
        "test_feature_bit_and_constants"]


def run(names):
    env = dict(os.environ, MSPACK_HIP_SO=emu_so())
    ids = ["tests/test_gpu_stored.py::" + n for n in names]
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1700)
    assert p.returncode == 0 and ("%d passed" % len(names)).encode() in p.stdout, p.stdout.decode()[-3000:]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_stored_kernel_on_the_emulator(built):
    run(KERNEL)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_stored_units_through_the_host_entry_points_on_the_emulator(built):
    run(HOST)
