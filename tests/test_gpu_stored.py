"""MSPACK_HIP_KIND_STORED (include/mspack_hip.h): CAB method 0 as a batch unit -- min(in_len, out_len) bytes of the unit's input copied
into its place in the output arena, at any alignment of either, nothing written outside it; the segments of all stored units of a
launch one pool of work (libmspack_amd/csrc/hip/stored_kernel.hpp).  Everything goes through the C ABI; the reference for a unit's
bytes is a slice of the input arena.

tests/test_stored_emu.py runs the first groups of this file (the shapes, the list of many units, the order list, the masks) on the
wavefront emulator."""
import hashlib
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import libmspack_amd as M
import test_gpu_crc32 as T
from test_gpu_hostpath import DevBuf
from test_gpu_md5 import GUARD, dev_write

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0xC9
ERR_READ, ERR_ARGS = 3, 1


def stored_units(rows):
    """rows: (in_off, in_len, out_off, out_len) -> a table of stored units"""
    u = np.zeros(len(rows), dtype=M.UNIT_DTYPE)
    u["kind"] = M.KIND_STORED
    for f, k in (("in_off", 0), ("in_len", 1), ("out_off", 2), ("out_len", 3)):
        u[f] = [int(r[k]) for r in rows]
    return u


def expected(units, arena, out_bytes, in_bytes=None):
    """what the output arena and the results must be: the canary everywhere but in the units' regions"""
    in_bytes = arena.size if in_bytes is None else in_bytes
    out = np.full(out_bytes, CANARY, dtype=np.uint8)
    res = np.zeros(len(units), dtype=M.RESULT_DTYPE)
    for i, u in enumerate(units):
        if int(u["kind"]) != M.KIND_STORED:
            continue
        io, il, oo, ol = int(u["in_off"]), int(u["in_len"]), int(u["out_off"]), int(u["out_len"])
        if io + il > in_bytes or oo + ol > out_bytes:
            res[i] = (ERR_ARGS, 0, 0, 0, 0, 0)
            continue
        n = min(il, ol)
        out[oo:oo + n] = arena[io:io + n]
        res[i] = (0 if il >= ol else ERR_READ, 0, n, n, n, 0)
    return out, res


def run_device(units, arena, out_bytes, mask=None, order=None, in_bytes=None):
    """mspack_hip_decode_batch_device over an output buffer of exactly out_bytes of canary inside a larger allocation of guard bytes,
    and an input arena of exactly in_bytes (+ the 8 bytes of slack the ABI asks for): -> (the output arena, the results); the guard
    bytes are checked here"""
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    in_bytes = arena.size if in_bytes is None else in_bytes
    big = DevBuf(out_bytes + 2 * GUARD, 0xA5)
    dev_write(big, GUARD, np.full(out_bytes, CANARY, dtype=np.uint8))
    d_in = DevBuf(arena.size + 8, 0x3C)
    dev_write(d_in, 0, arena)
    d_units, d_res = DevBuf(max(units.nbytes, 16)), DevBuf(max(len(units) * M.RESULT_DTYPE.itemsize, 16), 0x77)
    dev_write(d_units, 0, units.view(np.uint8))
    d_order = None
    if order is not None:
        o = np.ascontiguousarray(order, dtype=np.uint32)
        d_order = DevBuf(o.nbytes)
        dev_write(d_order, 0, o.view(np.uint8))
    L = M.lib()
    n_list = len(units) if order is None else len(order)                   # (n_units of the call is the list's length)
    rc = L.mspack_hip_decode_batch_device(d_units.ptr, d_order.ptr if d_order else None, n_list, d_in.ptr, in_bytes, big.ptr + GUARD,
                                          out_bytes, d_res.ptr, None, 0, M.MASK_STORED if mask is None else mask, None)
    assert rc == 0, L.mspack_hip_last_error()
    if big.emu is None:
        assert big.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(units) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE).copy()
    after = big.to_host()
    assert (after[:GUARD] == 0xA5).all() and (after[GUARD + out_bytes:] == 0xA5).all()
    for b in (big, d_in, d_units, d_res) + ((d_order,) if d_order else ()):
        b.free()
    return after[GUARD:GUARD + out_bytes].copy(), res


def check(units, arena, out_bytes, out, res, in_bytes=None):
    want_out, want_res = expected(units, arena, out_bytes, in_bytes)
    bad = np.nonzero(res != want_res)[0]
    assert not len(bad), [(int(i), units[int(i)], res[int(i)], want_res[int(i)]) for i in bad[:4]]
    diff = np.nonzero(out != want_out)[0]
    assert not len(diff), ("first wrong byte at", int(diff[0]), "of", len(diff), int(out[diff[0]]), int(want_out[diff[0]]))


# ---- lengths and alignments ---------------------------------------------------------------------------------------------------

LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 65535, 65536, 65537, 200003]
ALIGNS = [0, 1, 7, 15]


def shapes_layout(lengths=LENGTHS):
    """every length at every (in_off % 16, out_off % 16) of ALIGNS x ALIGNS, twice: between two small neighbouring units packed against
    it with no padding (so its first and last rows are shared with units other waves write), the group between canary bytes; and
    alone between canary bytes.  The neighbours' sizes move the edges around inside their rows"""
    rows, ipos, opos = [], 0, 0
    for n in lengths:
        for ia in ALIGNS:
            for oa in ALIGNS:
                for left, right in ((5, 3), (0, 0)):
                    opos += 1 + (oa - (opos + 1 + left)) % 16              # >= 1 canary byte, then the group
                    for ln in ([left] if left else []) + [n] + ([right] if right else []):
                        want_ia = ia if ln == n else (ipos + 3) % 16
                        ipos += (want_ia - ipos) % 16
                        rows.append((ipos, ln, opos, ln))
                        ipos += ln; opos += ln
    opos += 5
    return rows, ipos, opos


def test_lengths_and_alignments(built):
    """the edges of the row copy (15 / 16 / 17, 63 / 64 / 65) and of the 64 KiB segment, sources and destinations at 0, 1, 7 and 15 mod 16:
    every byte of the arena is what it must be -- the units' bytes, and the canary everywhere else"""
    assert M.features() & M.FEAT_STORED
    rows, in_bytes, out_bytes = shapes_layout()
    units = stored_units(rows)
    big = [r for r in rows if r[1] >= 15]
    assert set((r[0] % 16, r[2] % 16) for r in big) >= set((a, b) for a in ALIGNS for b in ALIGNS)
    arena = np.random.default_rng(9).integers(0, 256, in_bytes, dtype=np.uint8)
    out, res = run_device(units, arena, out_bytes)
    check(units, arena, out_bytes, out, res)


def test_short_input_and_arena_edges(built):
    """in_len = out_len - 1 and in_len = 0: MSPACK_ERR_READ, every available byte copied, nothing beyond; units that leave either arena:
    MSPACK_ERR_ARGS with zeros, nothing touched -- and the units beside them are served"""
    rng = np.random.default_rng(4)
    arena = rng.integers(0, 256, 200000, dtype=np.uint8)
    out_bytes = 150000
    rows = [(3, 99, 7, 100), (500, 0, 200, 100), (1001, 70000, 1003, 70001), (90000, 5, 80000, 0), (90000, 17, 80001, 16),
            (199990, 10, 149990, 10),                                        # ends exactly at both arenas' ends
            (199990, 11, 100, 5), (100, 5, 149990, 11), (200001, 0, 0, 0), (0, 0, 150001, 0), (10, 2 ** 32 - 1, 90000, 4), (10, 4, 0, 2 ** 32 - 1),
            (2 ** 40, 1, 90010, 1)]
    units = stored_units(rows)
    out, res = run_device(units, arena, out_bytes)
    check(units, arena, out_bytes, out, res)
    assert list(res["err"]) == [ERR_READ, ERR_READ, ERR_READ, 0, 0, 0] + [ERR_ARGS] * 7
    assert list(res["out_len"][:3]) == [99, 0, 70000] and list(res["in_used"][:3]) == [99, 0, 70000]


# ---- many units, one long one among them ----------------------------------------------------------------------------------------

def many_units():
    rng = np.random.default_rng(77)
    lens = [int(rng.integers(0, 301)) for _ in range(150)] + [(1 << 20) + 5] + [int(rng.integers(0, 301)) for _ in range(150)]
    rows, ipos, opos = [], 3, 11
    for n in lens:                                                          # packed: no padding in either arena
        rows.append((ipos, n, opos, n))
        ipos += n; opos += n
    return rows, ipos + 1, opos + 9


def test_many_units_and_a_long_one(built):
    """300 units of 0 to 300 bytes and one of 1 MiB + 5 in the middle, packed with no padding: several blocks of 64 list positions,
    seventeen segments of one unit among single ones; then the same table through an order list that permutes it"""
    rows, in_bytes, out_bytes = many_units()
    units = stored_units(rows)
    arena = np.random.default_rng(5).integers(0, 256, in_bytes, dtype=np.uint8)
    out, res = run_device(units, arena, out_bytes)
    check(units, arena, out_bytes, out, res)
    perm = np.random.default_rng(6).permutation(len(units)).astype(np.uint32)
    out, res = run_device(units, arena, out_bytes, order=perm)
    check(units, arena, out_bytes, out, res)


def test_stored_units_among_other_units_of_the_table(built):
    """whole blocks of 64 positions without a stored unit (kind 0, which nobody touches) in front of the first stored unit and between
    two groups of them; a list that names only some of the table's units"""
    rng = np.random.default_rng(15)
    arena = rng.integers(0, 256, 300000, dtype=np.uint8)
    rows, opos = [], 0
    for _ in range(70):
        n = int(rng.integers(0, 9000))
        rows.append((int(rng.integers(0, 290000)), n, opos, n)); opos += n
    units = np.concatenate([stored_units(rows), np.zeros(400, dtype=M.UNIT_DTYPE)])
    order = np.concatenate([np.arange(70, 270), np.arange(0, 35), np.arange(270, 470), np.arange(35, 70)]).astype(np.uint32)
    out, res = run_device(units, arena, opos + 3, order=order)
    assert (res[70:].view(np.uint8) == 0x77).all()
    check(units[:70], arena, opos + 3, out, res[:70])
    out, res = run_device(units, arena, opos + 3, order=np.arange(10, 20).astype(np.uint32))
    assert (res[:10].view(np.uint8) == 0x77).all() and (res[20:].view(np.uint8) == 0x77).all()
    only = units.copy(); only["kind"][:10] = 0; only["kind"][20:] = 0
    want_out, want_res = expected(only, arena, opos + 3)
    assert np.array_equal(out, want_out) and np.array_equal(res[10:20], want_res[10:20])


# ---- the mask -----------------------------------------------------------------------------------------------------------------------

def test_kind_mask(built):
    """bit 11: copied; no kind named ("all codecs"): copied; only other codecs named: nobody writes the stored unit's result or bytes"""
    arena = np.random.default_rng(1).integers(0, 256, 5000, dtype=np.uint8)
    units = stored_units([(1, 3000, 5, 3000), (3100, 70, 3005, 70)])
    for mask in (M.MASK_STORED, 0, M.MASK_STORED | (1 << M.KIND_MSZIP), 0x80000000):
        out, res = run_device(units, arena, 4000, mask=mask)
        check(units, arena, 4000, out, res)
    for mask in (1 << M.KIND_MSZIP, (1 << M.KIND_LZX) | (1 << M.KIND_XORSUM), M.MASK_MD5):
        out, res = run_device(units, arena, 4000, mask=mask)
        assert (res.view(np.uint8) == 0x77).all() and (out == CANARY).all()


# ---- the host entry points ----------------------------------------------------------------------------------------------------------

def check_host(units, arena, out, res):
    """a host-buffer call: the results and the units' regions (what lies between units inside a copied span is unspecified there)"""
    _o, want_res = expected(units, arena, out.size)
    assert np.array_equal(res, want_res), [(int(i), res[int(i)], want_res[int(i)]) for i in np.nonzero(res != want_res)[0][:4]]
    for u in units:
        io, oo, n = int(u["in_off"]), int(u["out_off"]), min(int(u["in_len"]), int(u["out_len"]))
        assert np.array_equal(out[oo:oo + n], arena[io:io + n]), (io, oo, n)


def host_shapes():
    """the shapes above for a host call: inputs and outputs ascend together"""
    rows, in_bytes, out_bytes = shapes_layout()
    return stored_units(rows), np.random.default_rng(19).integers(0, 256, in_bytes + 64, dtype=np.uint8), out_bytes


def test_decode_batch_shapes(built):
    """the same shapes through mspack_hip_decode_batch: the planner's own list for the kind, the arenas rebased to the spans"""
    units, arena, out_bytes = host_shapes()
    out, res = M.decode_batch(units, arena, out_bytes)
    check_host(units, arena, out, res)
    short = stored_units([(3, 99, 7, 100), (500, 0, 200, 100), (1001, 70000, 1003, 70001)])
    out, res = M.decode_batch(short, arena, 80000)
    check_host(short, arena, out, res)
    assert list(res["err"]) == [ERR_READ] * 3


def test_rejections(built):
    """a stored unit that leaves an arena: the batch is refused up front, the message names the unit, nothing is touched; kinds 9 and
    10 stay unknown"""
    arena = np.zeros(256, dtype=np.uint8)
    good = stored_units([(0, 64, 0, 64), (10, 20, 64, 20)])
    L = M.lib()
    for f, v, msg in (("in_len", 247, "unit 1: a stored unit's input leaves the input arena"), ("in_off", 257, "unit 1: a stored unit's input leaves the input arena"),
                      ("out_len", 37, "unit 1: a stored unit's output leaves the output arena"), ("out_off", 101, "unit 1: a stored unit's output leaves the output arena")):
        u = good.copy(); u[f][1] = v
        out = np.full(100, 0x5A, dtype=np.uint8)
        res = np.zeros(2, dtype=M.RESULT_DTYPE); res["err"] = 0x7777
        before = res.copy()
        rc = L.mspack_hip_decode_batch(u.ctypes.data, 2, arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data)
        assert rc != 0 and msg in L.mspack_hip_last_error().decode(), L.mspack_hip_last_error()
        assert np.array_equal(res, before) and (out == 0x5A).all()
    u = good.copy(); u["kind"][1] = 10
    out = np.zeros(100, dtype=np.uint8); res = np.zeros(2, dtype=M.RESULT_DTYPE)
    assert L.mspack_hip_decode_batch(u.ctypes.data, 2, arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data) != 0
    assert "unit 1: unknown kind 10" in L.mspack_hip_last_error().decode()
    u["kind"][1] = 9
    assert L.mspack_hip_decode_batch(u.ctypes.data, 2, arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data) != 0
    assert "unit 1: unknown kind 9" in L.mspack_hip_last_error().decode()
    # every field and flag the kind ignores, set: the same answer
    u = good.copy()
    u["window_bits"] = 21; u["reset_frames"] = 3; u["e8_base"] = 77; u["ref_len"] = 9; u["in_chunk"] = 12345; u["flags"] = 0x17F & ~M.UF_CRC32
    out, res = M.decode_batch(u, arena + 7, 100)
    check_host(u, arena + 7, out, res)


def mixed_batch():
    """MSZIP and LZX units, stored units between them -- two of them back to back, one in front of an MSZIP unit --, the CRC flag on
    some stored units, and MD5 / SHA-256 / CRC-32 digest units over one stored region, two adjacent ones, and a stored + an MSZIP one"""
    rng = np.random.default_rng(31)
    text = [M.gen_plaintext(900 + i, i % 4, 70000 + 111 * i) for i in range(4)]
    raw = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1000, 70001, 33333, 0, 129)]
    lz = [M.lzx_encode(text[0], 17, 0)[0].tobytes(), M.lzx_encode(text[1], 16, 0)[0].tobytes()]
    zp = [b"".join(T.mszip_deflate(text[2])), b"".join(T.mszip_deflate(text[3]))]
    items = [(M.KIND_LZX, lz[0], text[0].size, 17, 0, b""), (M.KIND_STORED, raw[0], len(raw[0]), 0, 0, b""), (M.KIND_STORED, raw[1], len(raw[1]), 0, 0, b""),
             (M.KIND_MSZIP, zp[0], text[2].size, 0, 0, b""), (M.KIND_STORED, raw[2], len(raw[2]), 0, 0, b""), (M.KIND_MSZIP, zp[1], text[3].size, 0, 0, b""),
             (M.KIND_STORED, raw[3], 0, 0, 0, b""), (M.KIND_LZX, lz[1], text[1].size, 16, 0, b""), (M.KIND_STORED, raw[4], len(raw[4]), 0, 0, b"")]
    units, arena, out_bytes, _refs = T.lay_out(items, residues=[0, 3, 0, 0, 9, 0, 5, 0, 15])
    units["out_off"][2] = units["out_off"][1] + units["out_len"][1]          # back to back with its neighbour (inside its own room)
    units["flags"][[1, 4, 6]] |= M.UF_CRC32
    plain = [text[0].tobytes(), raw[0], raw[1], text[2].tobytes(), raw[2], text[3].tobytes(), raw[3], text[1].tobytes(), raw[4]]
    o = [int(x) for x in units["out_off"]]; n = [int(x) for x in units["out_len"]]
    ranges = [(o[4], n[4]), (o[1] + 1, n[1] + n[2] - 2), (o[4] + 5, o[5] + n[5] - o[4] - 5), (o[8], n[8]), (o[2], n[2])]
    return units, arena, out_bytes, plain, ranges


def check_mixed(units, plain, out, res, ranges, dres, wide):
    assert (res["err"] == 0).all(), res
    for i, p in enumerate(plain):
        oo = int(units["out_off"][i])
        assert res["out_len"][i] == len(p) and out[oo:oo + len(p)].tobytes() == p, i
        if int(units["flags"][i]) & M.UF_CRC32:
            assert int(res["in_used"][i]) == (zlib.crc32(p) ^ 0xFFFFFFFF) & 0xFFFFFFFF, i
    got = M.result_wide_digests(dres[:len(wide)], wide)
    k = 0
    for kind in (M.KIND_MD5, M.KIND_SHA256):
        for (ro, rn) in ranges:
            b = out[ro:ro + rn].tobytes()
            assert got[k] == (hashlib.md5(b) if kind == M.KIND_MD5 else hashlib.sha256(b)).digest(), (kind, ro, rn)
            k += 1
    crcs = dres[len(wide):]
    assert (crcs["err"] == 0).all()
    for j, (ro, rn) in enumerate(ranges):
        assert int(crcs["out_len"][j]) == zlib.crc32(out[ro:ro + rn].tobytes()) & 0xFFFFFFFF, (ro, rn)


def run_mixed(n_devices=1):
    units, arena, out_bytes, plain, ranges = mixed_batch()
    wide, _heads = M.digest_units(ranges + ranges, [M.KIND_MD5] * len(ranges) + [M.KIND_SHA256] * len(ranges))
    both = np.concatenate([units, wide, M.crc32r_units(ranges)])
    out, res = M.decode_batch(both, arena, out_bytes, n_devices=n_devices)
    check_mixed(units, plain, out, res[:len(units)], ranges, res[len(units):], wide)
    # the stored ranges: the digests of the units' own bytes
    assert int(res["out_len"][len(units) + len(wide)]) == zlib.crc32(plain[4]) & 0xFFFFFFFF
    assert M.result_wide_digests(res[len(units):len(units) + len(wide)], wide)[4] == hashlib.md5(plain[2]).digest()


def test_mixed_batch(built):
    run_mixed()


def big_and_small():
    """one unit of 8 MiB beside 1000 units of 64 to 300 bytes, arena order: enough bytes and units for the planner to cut chunks"""
    rng = np.random.default_rng(8)
    lens = [int(rng.integers(64, 301)) for _ in range(500)] + [8 << 20] + [int(rng.integers(64, 301)) for _ in range(500)]
    rows, ipos, opos = [], 5, 0
    for n in lens:
        rows.append((ipos, n, opos, n)); ipos += n; opos += n + (n % 3)
    return stored_units(rows), rng.integers(0, 256, ipos + 64, dtype=np.uint8), opos


def chunked_units():
    """three units of 8 MiB among 1000 small ones: at least 8 MiB of input and 256 units per chunk make three chunks"""
    rng = np.random.default_rng(18)
    small = lambda k: [int(rng.integers(64, 301)) for _ in range(k)]
    lens = small(300) + [8 << 20] + small(300) + [(8 << 20) + 1] + small(300) + [(8 << 20) - 1] + small(100)
    rows, ipos, opos = [], 0, 0
    for n in lens:
        rows.append((ipos, n, opos, n)); ipos += n; opos += n
    return stored_units(rows), rng.integers(0, 256, ipos + 64, dtype=np.uint8), opos


def test_one_big_unit_beside_a_thousand_small_ones(built):
    units, arena, out_bytes = big_and_small()
    out, res = M.decode_batch(units, arena, out_bytes)
    check_host(units, arena, out, res)
    out, res = run_device(units, arena, out_bytes)
    check(units, arena, out_bytes, out, res)


WORKER = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import libmspack_amd as M
import test_gpu_stored as S
mode = sys.argv[1]
if mode == "jobs":
    # a batch the planner cuts: a stored unit of the first and one of the last chunk are waited for, their bytes and results are there
    units, arena, out_bytes = S.chunked_units()
    out = np.zeros(out_bytes, dtype=np.uint8)
    res = np.zeros(len(units), dtype=M.RESULT_DTYPE); res["err"] = 0x7777
    L = M.lib()
    job = L.mspack_hip_decode_batch_begin(units.ctypes.data, len(units), arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data)
    assert job
    for i in (3, len(units) - 2):
        assert L.mspack_hip_job_wait_unit(job, i) == 0
        assert int(res["err"][i]) == 0 and int(res["out_len"][i]) == int(units["out_len"][i])
        io, oo, n = int(units["in_off"][i]), int(units["out_off"][i]), int(units["out_len"][i])
        assert np.array_equal(out[oo:oo + n], arena[io:io + n])
    assert L.mspack_hip_job_end(job) == 0
    S.check_host(units, arena, out, res)
else:
    assert os.environ["MSPACK_HIP_FORCE_SHARDS"] in ("2", "3")
    S.run_mixed(n_devices=2)
    units, arena, out_bytes = S.big_and_small()
    out, res = M.decode_batch(units, arena, out_bytes, n_devices=2)
    S.check_host(units, arena, out, res)
    units, arena, out_bytes = S.host_shapes()
    out, res = M.decode_batch(units, arena, out_bytes, n_devices=2)
    S.check_host(units, arena, out, res)
print("STORED_WORKER_OK")
'''


@pytest.mark.parametrize("mode,env", [("shards", {"MSPACK_HIP_FORCE_SHARDS": "2"}), ("shards", {"MSPACK_HIP_FORCE_SHARDS": "3"}),
                                      ("jobs", {"MSPACK_HIP_TRACE": "1"})])
def test_sharded_and_job_entry_points(built, mode, env, tmp_path):
    """mspack_hip_decode_batch_multi cut into two and three shards, and _begin / _wait_unit on a stored unit of the first and of the
    last chunk / _end -- in a fresh process so that the environment switch is seen"""
    script = tmp_path / "w.py"
    script.write_text(WORKER % (ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script), mode], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0 and b"STORED_WORKER_OK" in p.stdout, p.stdout.decode()[-3000:]
    if mode == "jobs":
        cuts = [int(m.group(2)) for m in re.finditer(rb"(\d+) units in (\d+) chunks", p.stdout) if int(m.group(1)) == 1003]
        assert cuts and max(cuts) >= 2, p.stdout.decode()[-3000:]


def test_feature_bit_and_constants(built):
    assert M.KIND_STORED == 11 and M.FEAT_STORED == 512 and M.MASK_STORED == 1 << 11
    assert M.features() & M.FEAT_STORED
    hdr = open(os.path.join(ROOT, "include", "mspack_hip.h")).read()
    assert re.search(r"#define\s+MSPACK_HIP_KIND_STORED\s+11\b", hdr) and re.search(r"#define\s+MSPACK_HIP_FEAT_STORED\s+512u\b", hdr)
