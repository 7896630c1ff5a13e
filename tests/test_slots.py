"""CPU: the public face of the context slots (include/mspack_hip.h: mspack_hip_set_slots / _slots / _slot_stats, MSPACK_HIP_FEAT_SLOTS
and their mirrors in libmspack_amd): the argument's range, the default, the environment variable -- read once, in a process of
its own --, the feature bit, the statistics' reset.  No batch runs here (tests/test_gpu_slots.py and tests/test_hostcheck_slots.py
run them)."""
import os
import subprocess
import sys

import pytest

import libmspack_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys
sys.path.insert(0, %r)
import libmspack_amd as M
want = int(sys.argv[1])
assert M.slots() == want, (M.slots(), want)
# read once: what the environment says later changes nothing
os.environ["MSPACK_HIP_SLOTS"] = "2" if want != 2 else "3"      # (putenv: the C library sees it)
assert M.slots() == want
M.set_slots(2); assert M.slots() == 2
M.set_slots(1); assert M.slots() == 1
print("SLOTS_CHILD_OK")
'''


def child(env_value, want):
    env = dict(os.environ)
    env.pop("MSPACK_HIP_SLOTS", None)
    if env_value is not None:
        env["MSPACK_HIP_SLOTS"] = env_value
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(want)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"SLOTS_CHILD_OK" in p.stdout, p.stdout.decode()[-2000:]


def test_the_default_is_one_slot(built):
    child(None, 1)


@pytest.mark.parametrize("value,want", [("3", 3), ("4", 4), ("1", 1), ("0", 1), ("9", 4), ("junk", 1)])
def test_environment_is_read_once(built, value, want):
    """MSPACK_HIP_SLOTS gives the initial value (clamped to 1..4 like the library's other knobs); later changes of the environment
    are not seen, mspack_hip_set_slots() is"""
    child(value, want)


def test_set_slots_argument_range(built):
    old = M.slots()
    try:
        M.set_slots(3)
        L = M.lib()
        for bad in (0, 5, -1):
            assert L.mspack_hip_set_slots(bad) == -1
            assert M.slots() == 3, "a refused value changed the setting"
            with pytest.raises(ValueError):
                M.set_slots(bad)
        for n in (1, 2, 3, 4):
            assert L.mspack_hip_set_slots(n) == 0 and M.slots() == n
    finally:
        M.set_slots(old)
    assert M.slots() == old


def test_feature_bit_and_stats(built):
    assert M.features() & M.FEAT_SLOTS
    assert M.FEAT_SLOTS == 16
    M.lib().mspack_hip_slot_stats(None, 0)                  # (s may be NULL)
    M.slot_stats(reset=True)
    assert M.slot_stats() == (0, 0, 0)
