"""MSZIP window history beyond the stack's depth on the wavefront emulator (tests/emu/; tests/test_emu_kernels.py): the chains of
7, 8, 9 and 12 blocks of shrinking lengths of tests/crafted_streams.py, in CAB and in KWAJ framing, with requests that end inside
the chain and inside the last block, through the real kernel sources in a fresh process -- results, every byte, the bytes a block
produced beyond the request and the guard bytes around every unit against the oracle (tests/test_gpu_mszip_history.py's checks).
Depth 8 is the last the (B, length) stack of mszip_kernel.hpp holds; from depth 9 on the unit's slack is the ring."""
import os
import subprocess
import sys

import pytest

from helpers import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

WORKER = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
import libmspack_amd as M
import test_gpu_mszip_history as H
assert "emu" in M.HIP_SO
want = ["shrinking_chain_depth_%%d" %% d for d in (7, 8, 9, 12)]
items = [(c, False) for c in H.cases() if any(w + "_" in c.name + "_" for w in want)]
assert len(items) == 4 * 3 + 4, [c.name for c, _t in items]
H.run_device(items, "emulator, device entry")
H.run_host(items + [(c, True) for c, _t in items if c.codec == "mszip"], "emulator, host entry")
print("EMU_HISTORY_OK")
'''


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the emulator build needs ROCm's clang++")
def test_deep_chains_on_the_wavefront_emulator(built, tmp_path):
    so = emu_so()
    script = tmp_path / "w.py"
    script.write_text(WORKER % (ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MSPACK_HIP_SO=so), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=1500)
    assert p.returncode == 0 and b"EMU_HISTORY_OK" in p.stdout, p.stdout.decode()[-3000:]
