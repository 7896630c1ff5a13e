"""MSZIP window history at any depth and KWAJ framing, on every path: the hand-built streams of tests/crafted_streams.py
(mszip_history_cases: chains of blocks of shrinking lengths up to 40 levels deep, equal lengths, a full block after a deep chain,
blocks of 0 bytes, matches across level boundaries, mixed block types, never-written indices, repair mode; kwaj_mszip_cases: the
same streams framed as KWAJ files frame them, and the framing's own edges) against the oracle -- err, flags, out_len, good_len,
in_next, every byte of out_len, the bytes a block produced beyond the request (in the unit's slack right behind out_len), the
repair log -- and against the generator's own ring.  Every unit lies between guard bytes: its region is out_len + 32768 bytes of
slack (+ the repair log), and nothing outside may change where the test owns the output buffer.

Paths: the host entry, _to_device, the device-resident entry (also with block tables, where the frame words say which blocks the
parse and fold tasks did), three shards in a child process, a batch mixed with LZSS ring units, the kwajd object API.  The case
lists are built once per process (1.5 s) and the oracle runs once per case."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import crafted_streams as CS
import libmspack_amd as M
from helpers import oracle_mszip, oracle_mszip_kwaj, oracle_set_hard_eof

pytestmark = pytest.mark.gpu
ADOPTED = M.F_FRAMES_ADOPTED
FRAME = 32768
GUARD, FILL = 256, 0xA5
LOG_CAP = 4
MASK_FRAME_TABLES = 0x80000000
MASK_LZSS_RING = 0x20000000

_CASES, _ORACLE = {}, {}


def cases(which="all"):
    if not _CASES:
        _CASES["cab"] = CS.mszip_history_cases()
        _CASES["kwaj"] = CS.kwaj_mszip_cases()
        _CASES["all"] = _CASES["cab"] + _CASES["kwaj"]
    return _CASES[which]


def oracle(c):
    """(err, bytes, result) of the oracle for the unit as the kernels get it, once per case"""
    if c.name not in _ORACLE:
        if c.codec == "kwaj_mszip":
            oracle_set_hard_eof(bool(c.props["uflags"] & CS.UF_HARD_EOF))
            try:
                _ORACLE[c.name] = oracle_mszip_kwaj(c.stream, c.out_len)
            finally:
                oracle_set_hard_eof(0)
        else:
            repair = (c.props["in_chunk"] or 1) if c.props["uflags"] & CS.UF_MSZIP_REPAIR else 0
            # (room behind the request: the oracle hands out the rest of the last block too)
            e, o, r, _ = oracle_mszip(c.stream, c.out_len, repair)
            _e, o2, _r, _ = oracle_mszip(c.stream, c.out_len + FRAME, repair)
            _ORACLE[c.name] = (e, o, r, o2[c.out_len:c.out_len + r.in_next] if e == 0 else b"")
    return _ORACLE[c.name]


def log_bytes(c):
    return 16 + 4 + 8 * LOG_CAP if c.props["uflags"] & CS.UF_MSZIP_LOG else 0


def batch(items):
    """items: (case, with its block table?) -> (units, arena, out_bytes): every unit its own copy of the stream (in_len exact: the
    feeder's end is the stream's), GUARD bytes in front of and behind its region"""
    offs, toffs, pos = [], [], 0
    for c, tab in items:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(c.stream)
        pos = (pos + 3) & ~3
        toffs.append(pos); pos += 4 * len(c.tab) if tab else 0
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for (c, tab), o, to in zip(items, offs, toffs):
        arena[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
        if tab:
            arena[to:to + 4 * len(c.tab)] = np.asarray(c.tab, dtype=np.uint32).view(np.uint8)
    units, _ = M.make_units(M.KIND_MSZIP, offs, [len(c.stream) for c, _t in items], [c.out_len for c, _t in items],
                            flags=[c.props["uflags"] for c, _t in items], out_slack=FRAME)
    pos = GUARD
    for i, (c, tab) in enumerate(items):
        assert not tab or c.codec == "mszip"
        if tab:
            units["flags"][i] |= M.UF_FRAME_TABLE
            units["in_chunk"][i] = toffs[i] // 4
        else:
            units["in_chunk"][i] = c.props.get("in_chunk", 0)
        if c.props["uflags"] & CS.UF_MSZIP_LOG:
            units["e8_base"][i] = LOG_CAP
        units["out_off"][i] = pos
        pos = (pos + c.out_len + FRAME + 15) & ~15
        pos += log_bytes(c) + GUARD
    fr = M.frames_of(units)
    units["frame_base"] = np.concatenate([[0], np.cumsum(fr)[:-1]])
    return units, arena, pos


def check(items, units, out, res, how, guards=True):
    for i, (c, tab) in enumerate(items):
        orc = oracle(c)
        e, o, r = orc[:3]
        what = (how, c.name, "table" if tab else "", res[i], e, r.out_len, r.in_next, r.flags)
        assert res["err"][i] == e == c.err, what
        assert res["out_len"][i] == res["good_len"][i] == r.out_len == c.props["written"], what
        assert res["in_next"][i] == r.in_next == c.props["in_next"], what
        assert (int(res["flags"][i]) & ~ADOPTED) == r.flags == c.props.get("rflags", 0), what
        oo = int(units["out_off"][i])
        got = out[oo:oo + r.out_len].tobytes()
        if got != o[:r.out_len]:
            k = next(k for k in range(r.out_len) if got[k] != o[k])
            raise AssertionError("%s, %s: byte %d is 0x%02X, not 0x%02X; %d bytes differ" % (
                how, c.name, k, got[k], o[k], sum(a != b for a, b in zip(got, o[:r.out_len]))))
        assert got == c.plain, what
        if c.codec == "mszip" and r.in_next:
            # what the last block produced beyond the request lies in the slack right behind out_len
            assert out[oo + c.out_len:oo + c.out_len + r.in_next].tobytes() == orc[3], what
        end = (oo + c.out_len + FRAME + 15) & ~15
        if c.props["uflags"] & CS.UF_MSZIP_LOG:
            log = out[end:end + 4 + 8 * LOG_CAP].view(np.uint32)
            want = c.props["repaired"]
            assert log[0] == len(want) and log[1:1 + 2 * len(want)].tolist() == [v for p in want for v in p], what + (log.tolist(),)
        if guards:
            end += log_bytes(c)
            assert (out[oo - GUARD:oo] == FILL).all() and (out[end:end + GUARD] == FILL).all(), what + ("a guard byte changed",)


def all_items(tables=False):
    it = [(c, False) for c in cases()]
    if tables:
        it += [(c, True) for c in cases("cab") if not c.props["uflags"] & CS.UF_MSZIP_REPAIR]
    return it


def run_host(items, how="host entry", n_devices=1, reverse_out=False):
    units, arena, out_bytes = batch(items)
    if reverse_out:
        units, arena, out_bytes = batch(items[::-1])
        units = units[::-1].copy()
        units["frame_base"] = np.concatenate([[0], np.cumsum(M.frames_of(units))[:-1]])
    out, res = M.decode_batch(units, arena, out_bytes, n_devices=n_devices)
    check(items, units, out, res, how, guards=False)        # (decode_batch owns the output buffer: zeros, copied back per unit)
    return res


def run_to_device(items, how="to_device"):
    from test_gpu_crafted import to_device
    units, arena, out_bytes = batch(items)
    out, res = to_device(units, arena, out_bytes)
    check(items, units, out, res, how)
    return res


def run_device(items, how="device entry", extra=None):
    """mspack_hip_decode_batch_device with the test's own scratch and an output buffer full of FILL -> (results, frame words per item).
    extra: (units, arena bytes, room) of other kinds to mix in behind the MSZIP units -> their results and output come back too"""
    from test_gpu_hostpath import DevBuf
    from test_gpu_md5 import dev_write
    lib = M.lib()
    units, arena, out_bytes = batch(items)
    mask = MASK_FRAME_TABLES | (1 << M.KIND_MSZIP)
    if extra is not None:
        xu, xa, xroom, xmask = extra
        xu = xu.copy()
        xu["in_off"] += arena.size
        xu["out_off"] += out_bytes
        arena = np.concatenate([arena, xa])
        units = np.concatenate([units, xu])
        order = np.argsort(np.arange(len(units)) % 7, kind="stable")      # (the kinds interleaved through the table)
        units, inv = units[order], np.argsort(order)
        out_bytes += xroom
        mask |= xmask
    u = np.ascontiguousarray(units)
    n_frames = int(M.frames_of(u).sum())
    u["frame_base"] = np.concatenate([[0], np.cumsum(M.frames_of(u))[:-1]])
    big = DevBuf(out_bytes, FILL)
    d_units, d_in = DevBuf(u.nbytes), DevBuf(arena.size + 64, 0xFF)
    d_res = DevBuf(len(u) * M.RESULT_DTYPE.itemsize, 0x77)
    scratch = DevBuf(max(int(lib.mspack_hip_frame_scratch_bytes(n_frames)), 16))
    dev_write(d_units, 0, u.view(np.uint8))
    dev_write(d_in, 0, arena)
    rc = lib.mspack_hip_decode_batch_device(d_units.ptr, None, len(u), d_in.ptr, arena.size, big.ptr, out_bytes, d_res.ptr,
                                            scratch.ptr, n_frames, mask, None)
    assert rc == 0, lib.mspack_hip_last_error()
    if big.emu is None:
        assert big.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(u) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE).copy()
    words = [M.debug_frame_words(scratch.ptr, n_frames, int(u["frame_base"][i]), int(M.frames_of(u[i:i + 1])[0]), True)
             if u["flags"][i] & M.UF_FRAME_TABLE else None for i in range(len(u))]
    out = big.to_host()
    for b in (big, d_units, d_in, d_res, scratch):
        b.free()
    if extra is not None:
        res, u, words = res[inv], u[inv], [words[k] for k in inv]
    check(items, u[:len(items)], out, res[:len(items)], how)
    return res, words[:len(items)], out, u


# ---- the tests -------------------------------------------------------------------------------------------------------------------
def test_host_entry(built):
    run_host(all_items(tables=True))


def test_to_device(built):
    run_to_device(all_items(tables=True))


def test_device_entry(built):
    run_device(all_items())


HUFFMAN = "mszip_history_huffman_blocks_only_full_blocks_around_a_chain"
MIXED = "mszip_history_stored_fixed_dynamic_mixed_in_a_chain"


def test_block_tables_and_frame_words(built):
    """CAB framing with MSPACK_HIP_UF_FRAME_TABLE: the same results, and what the frame words (status, n_tokens, total_out, fold)
    and MSPACK_HIP_F_FRAMES_ADOPTED show.  A parse wave parses any Huffman block its table names; the folder's wave adopts a record
    only while the block lies at block index x 32768 -- up to the first short block, never again behind it, also not behind a
    later full block; a fold task finishes only blocks with full, folded blocks below them.  Adoption
    throughout is checked on a folder of full blocks only; MSPACK_HIP_FOLD=2 (the next test's child process) forces the folds."""
    forced = os.environ.get("MSPACK_HIP_FOLD") == "2"
    items = [(c, True) for c in cases("cab") if not c.props["uflags"] & CS.UF_MSZIP_REPAIR]
    res, words, _out, _u = run_device(items, "device entry, block tables")
    for (c, _t), w, r in zip(items, words, res):
        blocks = c.props["blocks"]
        lead = next((k for k, n in enumerate(blocks) if n != FRAME), len(blocks))       # full blocks in front of the first short one
        assert len(w) == (c.out_len + FRAME - 1) // FRAME, c.name
        done = {b for b in range(len(w)) if w[b][3] == 1}
        assert done <= set(range(lead + 1)), (c.name, sorted(done), lead, w.tolist())
        for b in range(len(w)):
            assert w[b][0] != 1 or w[b][2] == blocks[b], (c.name, b, w.tolist())         # (a parsed block: its own length)
        if c.name == HUFFMAN:
            assert lead == 2 and len(w) >= 7 and all(w[b][0] == 1 for b in range(len(w))), w.tolist()
            assert r["flags"] & ADOPTED, r
            if forced:
                assert done == {0, 1, 2}, (sorted(done), w.tolist())
        if c.name == MIXED:
            # (block 1 -- short, fixed Huffman, behind one full block -- lies where its parse wave assumed: adopted; block 2 does not)
            assert w[1][0] == 1 and r["flags"] & ADOPTED, (r, w.tolist())
    assert {HUFFMAN, MIXED} <= {c.name for c, _t in items}
    deep = next(c for c, _t in items if c.name == "mszip_history_full_block_after_a_deep_chain")
    full = CS.Deflate()
    for k in range(3):
        full.frame(); full.fixed([('L', CS._text(1900 + k, 300)), ('M', 258, 100)] + ([('M', 30, FRAME)] if k else []) +
                                 [('L', CS._text(1910 + k, FRAME - 558 - (30 if k else 0)))], last=1)
    cf = CS._hist_case("mszip_history_full_blocks_only", full)
    res, words, _out, _u = run_device([(deep, True), (cf, True)], "device entry, block tables, full blocks behind a deep chain")
    assert res["flags"][1] & ADOPTED and all(words[1][b][0] == 1 for b in range(3)), (res[1], words[1].tolist())
    assert not res["flags"][0] & ADOPTED, res[0]          # (stored blocks throughout: nothing for a parse wave)
    if forced:
        assert {b for b in range(3) if words[1][b][3] == 1} == {0, 1, 2}, words[1].tolist()


def test_block_tables_with_fold_tasks_forced_in_a_child_process(built):
    """the test above with MSPACK_HIP_FOLD=2 (read when the library is loaded: a fresh process)"""
    env = dict(os.environ, MSPACK_HIP_FOLD="2")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "test_block_tables_and_frame_words"], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    assert p.returncode == 0 and b"1 passed" in p.stdout, p.stdout.decode()[-3000:]


SHARD_WORKER = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import libmspack_amd as M
import test_gpu_mszip_history as H
assert os.environ["MSPACK_HIP_FORCE_SHARDS"] == "3"
items = H.all_items(tables=True)
M.slot_stats(reset=True)
H.run_host(items, "host entry, three shards", n_devices=2)
# every shard is a batch of its own on its device's context slot
assert M.slot_stats()[0] == 3, M.slot_stats()
# output regions in falling order: the shards' spans interleave and the copies back go unit by unit
H.run_host(items[::-1], "host entry, three shards, units reversed", n_devices=2, reverse_out=True)
print("SHARDS_OK")
'''


def test_three_shards_in_a_child_process(built, tmp_path):
    """mspack_hip_decode_batch_multi with MSPACK_HIP_FORCE_SHARDS=3 (as tests/test_gpu_hostpath.py does): the batch of every case
    cut into three shards, which run as three batches"""
    script = tmp_path / "w.py"
    script.write_text(SHARD_WORKER % (ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MSPACK_HIP_FORCE_SHARDS="3"), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0 and b"SHARDS_OK" in p.stdout, p.stdout.decode()[-3000:]


def test_mixed_batch_with_lzss_ring_units(built):
    """the deep chains of both framings in one table with LZSS units that keep their window in LDS (MSPACK_HIP_MASK_LZSS_RING)"""
    from helpers import oracle_lzss
    lz = [c for c in CS.lzss_cases() if c.err == 0 and c.wb <= 2][:12]
    offs, pos = [], 0
    for c in lz:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(c.stream)
    xa = np.zeros(pos + 64, dtype=np.uint8)
    for c, o in zip(lz, offs):
        xa[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
    xu, xroom = M.make_units(M.KIND_LZSS, offs, [len(c.stream) for c in lz], [c.rooms[0] for c in lz], window_bits=[c.wb for c in lz],
                             flags=M.UF_LZSS_RING)
    items = [(c, False) for c in cases() if "depth" in c.name or "deep" in c.name]
    res, _w, out, u = run_device(items, "mixed with LZSS ring units", extra=(xu, xa, xroom, (1 << M.KIND_LZSS) | MASK_LZSS_RING))
    for k, c in enumerate(lz):
        i = len(items) + k
        e, o, r = oracle_lzss(c.stream, c.wb, c.rooms[0])
        assert res["err"][i] == e == 0 and res["out_len"][i] == r.out_len, (c.name, res[i])
        oo = int(u["out_off"][i])
        assert out[oo:oo + r.out_len].tobytes() == o[:r.out_len] == c.plain, c.name


def test_kwajd_object_api(built):
    """kwajd extract() of the KWAJ cases as files (method 4): error and every byte written, also before a failure -- the driver
    refits the room (MSPACK_HIP_F_OUT_FULL) where the header's length is too small; and KwajSet.prefetch() of all of them"""
    from libmspack_amd import api
    seen, files = set(), []
    for c in cases("kwaj"):
        if c.stream in seen or c.props["uflags"] & CS.UF_HARD_EOF:
            continue
        seen.add(c.stream)
        total = sum(c.props["blocks"])
        e, o, _r = oracle_mszip_kwaj(c.stream, total + 2 * FRAME)
        for length in (total, 1):                     # (the header's length field is a hint: 1 forces the refit)
            blob = CS.kwaj_container(c.stream, 4, length)
            g = api.szdd_kwaj_extract(1, blob)
            assert g["open_err"] == 0 and g["err"] == e and g["data"] == o, (c.name, length, g["err"], e, len(g["data"]), len(o))
        files.append((c.name, CS.kwaj_container(c.stream, 4, total), e, o))
    assert len(files) >= 25
    s = api.KwajSet([f[1] for f in files])
    try:
        assert s.prefetch() == 0
        for k, (name, _blob, e, o) in enumerate(files):
            g = s.extract(k)
            assert g["open_err"] == 0 and g["err"] == e and g["data"] == o, (name, g["err"], e, len(g["data"]), len(o))
    finally:
        s.close()
