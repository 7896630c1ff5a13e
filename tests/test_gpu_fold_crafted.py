"""The hand-built folders of tests/crafted_streams.py fold_cases() through the kernels: the fold tasks (mspack_lzx_fold / mspack_mszip_fold:
lzx_fold.hpp, fold_common.hpp, mszip_kernel.hpp zip_fold_block) and the record pool (wave_common.hpp RecWriter / RecPool) at their
structural edges -- and, through mspack_hip_debug_frame_words, WHICH PATH TOOK EVERY FRAME: a fold task that gave every frame (or every
frame with a placeholder, or every frame from the third on) back to the serial path passes every parity test there is.

The fold policy is read when the library loads, so each policy runs in a process of its own (as tests/test_gpu_fold.py does):
MSPACK_HIP_FOLD=2 (every launch that can runs the fold tasks), 1 (the shipped rule) and 0 (never).  In each process
  * every case goes through mspack_hip_decode_batch alone, then all of them in one batch: err, out_len, in_next, flags without
    FRAMES_ADOPTED and every byte up to out_len against the oracle and against the case's own plaintext;
  * every case goes through mspack_hip_decode_batch_device with the test's own scratch, into a buffer full of 0xA5 between guard bytes:
    the same parity, guards intact; then the frame words: under policy 2 exactly the frames (blocks) of the case's `folds` came back
    with rst == 1 and chain == 1 (MSZIP: fold == 1); under policy 0 no frame has rst != 0 (fold != 0); under policy 1 the folders that
    fold in full must have had their frames adopted;
  * the two folders that run the record pool dry (113 chunks wanted, 54 there), alone and beside an ordinary folder that shares their
    launch's pool: full parity and err 0 for both, the folded frames a prefix of the folder -- which frame finds the pool empty
    depends on which parse task took its chunks first, so nothing else is asserted.
No case is skipped; `folds` is None for the pool-dry folders only.

Wall times on an MI355X: a policy's process 1.2 to 1.4 s from start to end, of which the host entry takes 0.29 to 0.41 s (26 cases
alone and once together), the device entry with the frame words 0.11 s, the pool-dry folders 0.19 s and the oracle 0.03 s.  The
builders are per-byte Python: the case list is built once, by the module's fixture (3.9 s there), and handed to the three processes
as a file."""
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import crafted_streams as CS
import libmspack_amd as M
from helpers import oracle_lzx, oracle_mszip

pytestmark = pytest.mark.gpu
ADOPTED = M.F_FRAMES_ADOPTED
FRAME = 32768
GUARD, FILL = 4096, 0xA5
MASK_FRAME_TABLES = 0x80000000
POOL_DRY = "fold_lzx_pool_runs_dry_"
NEIGHBOUR = "fold_lzx_pool_neighbour"


# ---- one batch of cases ------------------------------------------------------------------------------------------------------------
def batch(cases):
    """-> (units, arena, out_bytes): every case its stream and its frame table in the arena"""
    offs, toffs, pos = [], [], 0
    for c in cases:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(c.stream)
        pos = (pos + 3) & ~3
        toffs.append(pos); pos += 4 * len(c.tab)
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for c, o, to in zip(cases, offs, toffs):
        arena[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
        arena[to:to + 4 * len(c.tab)] = np.asarray(c.tab, dtype=np.uint32).view(np.uint8)
    kinds = [M.KIND_LZX if c.codec == "lzx" else M.KIND_MSZIP for c in cases]
    units, out_bytes = M.make_units(kinds, offs, [len(c.stream) for c in cases], [c.out_len for c in cases],
                                    window_bits=[c.wb for c in cases], reset_frames=[c.reset for c in cases], out_slack=32768,
                                    frame_tabs=toffs)
    return units, arena, out_bytes


_ORACLE = {}


def oracle(c):
    """(err, bytes, result words) of the oracle, computed once per case"""
    if c.name not in _ORACLE:
        _ORACLE[c.name] = oracle_lzx(c.stream, c.out_len, c.wb, c.reset) if c.codec == "lzx" else oracle_mszip(c.stream, c.out_len)[:3]
    return _ORACLE[c.name]


def check_parity(cases, units, out, res, how):
    for i, c in enumerate(cases):
        e, o, r = oracle(c)
        what = (how, c.name, res[i], e, r.out_len, r.in_next, r.flags)
        assert res["err"][i] == e == c.err and res["out_len"][i] == r.out_len and res["in_next"][i] == r.in_next, what
        assert (int(res["flags"][i]) & ~ADOPTED) == r.flags, what
        oo = int(units["out_off"][i])
        got = out[oo:oo + r.out_len].tobytes()
        if got != o[:r.out_len]:
            k = next(k for k in range(r.out_len) if got[k] != o[k])
            raise AssertionError("%s, %s: byte %d (frame %d + %d) is 0x%02X, not 0x%02X; %d bytes differ" % (
                how, c.name, k, k // FRAME, k % FRAME, got[k], o[k], sum(a != b for a, b in zip(got, o[:r.out_len]))))
        assert c.plain is None or got == c.plain, what


def run_host(cases, how):
    units, arena, out_bytes = batch(cases)
    out, res = M.decode_batch(units, arena, out_bytes)
    check_parity(cases, units, out, res, how)
    return res


def run_device(cases, how):
    """the cases through mspack_hip_decode_batch_device with the test's own scratch, the output arena inside a larger buffer of FILL:
    parity, guards intact -> (results, per case the frame words of its real frames / blocks)"""
    from test_gpu_hostpath import DevBuf
    from test_gpu_md5 import dev_write
    lib = M.lib()
    units, arena, out_bytes = batch(cases)
    u = np.ascontiguousarray(units)
    n_frames = int(M.frames_of(u).sum())
    big = DevBuf(out_bytes + 2 * GUARD, FILL)
    d_units, d_in = DevBuf(u.nbytes), DevBuf(arena.size + 64, 0xFF)
    d_res = DevBuf(len(u) * M.RESULT_DTYPE.itemsize, 0x77)
    scratch = DevBuf(max(int(lib.mspack_hip_frame_scratch_bytes(n_frames)), 16))
    dev_write(d_units, 0, u.view(np.uint8))
    dev_write(d_in, 0, arena)
    mask = MASK_FRAME_TABLES
    for k in set(int(k) for k in u["kind"]):
        mask |= 1 << k
    rc = lib.mspack_hip_decode_batch_device(d_units.ptr, None, len(u), d_in.ptr, arena.size, big.ptr + GUARD, out_bytes, d_res.ptr,
                                            scratch.ptr, n_frames, mask, None)
    assert rc == 0, lib.mspack_hip_last_error()
    if big.emu is None:
        assert big.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(u) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE).copy()
    words = [M.debug_frame_words(scratch.ptr, n_frames, int(u["frame_base"][i]), (c.out_len + FRAME - 1) // FRAME, c.codec == "mszip")
             for i, c in enumerate(cases)]
    after = big.to_host()
    for b in (big, d_units, d_in, d_res, scratch):
        b.free()
    assert (after[:GUARD] == FILL).all() and (after[GUARD + out_bytes:] == FILL).all(), (how, "a byte outside the output arena changed")
    check_parity(cases, units, after[GUARD:GUARD + out_bytes], res, how)
    return res, words


def folded(c, w):
    """the frames (blocks) a fold task finished, and the ones one touched at all"""
    if c.codec == "mszip":
        return {b for b in range(len(w)) if w[b][3] == 1}, {b for b in range(len(w)) if w[b][3] != 0}
    return {f for f in range(len(w)) if w[f][4] == 1 and w[f][3] == 1}, {f for f in range(len(w)) if w[f][4] != 0}


def check_words(c, w, res_i, policy, how):
    done, touched = folded(c, w)
    what = (how, c.name, "policy %d" % policy, "folded", sorted(done), "wanted", None if c.folds is None else sorted(c.folds), w.tolist())
    if policy == 0:
        assert not touched, what
    elif policy == 2:
        if c.folds is None:
            assert done == set(range(len(done))), what                    # a prefix of the folder
        else:
            assert done == set(c.folds), what
    elif c.folds is not None and len(c.folds) == len(w):
        assert res_i["flags"] & ADOPTED, what


def run_all(cases, policy):
    t0 = time.time()
    assert all((c.folds is None) == c.name.startswith(POOL_DRY) for c in cases)
    if policy != 2:
        cases = [c for c in cases if not c.props.get("policy_2_only")]
    plain = [c for c in cases if c.folds is not None]
    dry = [c for c in cases if c.folds is None]
    neighbour = next(c for c in cases if c.name == NEIGHBOUR)
    assert len(dry) == 2 and len(plain) >= 25
    for c in cases:
        oracle(c)
    t1 = time.time()
    for c in plain:
        run_host([c], "alone, host entry")
    run_host(plain, "all in one batch, host entry")
    t2 = time.time()
    for c in plain:
        res, words = run_device([c], "alone, device entry")
        check_words(c, words[0], res[0], policy, "alone, device entry")
    t3 = time.time()
    for c in dry:
        run_host([c], "alone, host entry")
        run_host([c, neighbour], "beside its neighbour, host entry")
        run_host([neighbour, c], "behind its neighbour, host entry")
        res, words = run_device([c], "alone, device entry")
        assert res["err"][0] == 0
        check_words(c, words[0], res[0], policy, "alone, device entry")
        res, words = run_device([c, neighbour], "beside its neighbour, device entry")
        assert res["err"][0] == 0 and res["err"][1] == 0
        check_words(c, words[0], res[0], policy, "beside its neighbour, device entry")
        if policy == 2:
            done, _ = folded(neighbour, words[1])
            assert done == set(range(len(done))), ("the starved neighbour", sorted(done))
    t4 = time.time()
    print("policy %d: oracle %.2f s, host entry %.2f s, device entry and frame words %.2f s, pool-dry folders %.2f s" % (
        policy, t1 - t0, t2 - t1, t3 - t2, t4 - t3))
    print("FOLD_CRAFTED_OK")


# ---- the test: one process per policy ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("fold") / "cases.pickle"
    with open(p, "wb") as f:
        pickle.dump(CS.fold_cases(), f)
    return str(p)


@pytest.mark.parametrize("policy", ["2", "1", "0"], ids=["always", "shipped_rule", "never"])
def test_fold_cases_on_every_path(built, case_file, policy):
    env = dict(os.environ, MSPACK_HIP_FOLD=policy)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), case_file], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0 and b"FOLD_CRAFTED_OK" in p.stdout, p.stdout.decode()[-4000:]


if __name__ == "__main__":
    with open(sys.argv[1], "rb") as f:
        run_all(pickle.load(f), int(os.environ["MSPACK_HIP_FOLD"]))
