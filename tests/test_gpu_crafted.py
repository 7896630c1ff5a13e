"""The hand-built streams of tests/crafted_streams.py through the kernels.  Every case in one batch per codec -- LZX and MSZIP
with and without their frame tables -- against the oracle (error, out_len, in_next, flags without FRAMES_ADOPTED, every byte
up to out_len) and against the helper's own plaintext; the multi-frame cases with one block per frame must really take the
frame-parallel path.  Then every valid LZX case 600 times in one batch with its frame table, so that the pipe's tickets no
longer all find a wave at once (frame-slot order -- the cases' frame counts differ, so the launch is not uniform --, speculative
headers, more slots than waves; the ticket orders of uniform launches are tests/test_gpu_lzx_uniform.py's): ~16 000 units, ~900 MB of
output, 2.5 s on an MI355X.  The Quantum cases go in three times each -- in_len exact, in_len extended over 160 zero bytes
(the lean reader), exact with a failing feeder -- and in_used and good_len are held against the oracle too; then every valid
one 200 times in one batch, every third unit with marks (wall time of the Quantum tests on an MI355X: not measured yet).
The LZSS and KWAJ LZH cases go in at every room of theirs (ample, exact, one byte less, inside a match, none) and, the valid
ones, at every residue of in_off and out_off mod 16, in the test's own layout with guard bytes between the units; the same batch
then goes into a device buffer full of 0xA5, in which nothing but the pre-fill's spaces and the decoded bytes may have changed:
check_lzss (7605 units, both passes) takes 0.07 s and check_lzh (5091 units) 0.06 s on an MI355X once the library is warm,
test_crafted_streams_vs_oracle with all codecs 10.1 s; every valid case 300 times in one batch, both kinds interleaved, every
third unit with a CRC-32: 3.0 s."""
import zlib

import numpy as np
import pytest

import crafted_streams as CS
import libmspack_amd as M
from helpers import oracle_kwaj_lzh, oracle_lzss, oracle_lzx, oracle_lzxd, oracle_mszip, oracle_qtm, oracle_qtm_marks, oracle_set_hard_eof
from test_gpu_hostpath import DevBuf
import test_gpu_lzx_frames as T
import test_gpu_lzxd as D
import test_gpu_mszip_blocks as B

pytestmark = pytest.mark.gpu
ADOPTED = M.F_FRAMES_ADOPTED
# several frames, one block per frame, a right table: the frame-parallel parse must adopt them
MUST_ADOPT = {"lzx_fixed_8_bit_literals_w21", "lzx_fixed_8_bit_literals_w15", "lzx_258_byte_matches_over_three_frames",
              "lzx_parse_wave_sub_tables_beyond_their_cap", "lzx_repeats_right_after_resets"}


def check_lzx(cases):
    streams, params, tabs, plains = [], [], [], []
    for c in cases:
        for tab in (np.asarray(c.tab, dtype=np.int64), None):
            streams.append(c.stream); params.append((c.out_len, c.wb, c.reset, 0)); tabs.append(tab); plains.append(c.plain)
    units, out, res = T.run(streams, params, tabs)
    T.check(streams, params, units, out, res)
    for i, p in enumerate(plains):
        if p is not None:
            assert res["err"][i] == 0 and out[units["out_off"][i]:units["out_off"][i] + len(p)].tobytes() == p, i
    for j, c in enumerate(cases):
        if c.name in MUST_ADOPT:
            assert res["flags"][2 * j] & ADOPTED, (c.name, res[2 * j])


def check_lzxd(cases):
    units, out, res = D.run_delta([c.stream for c in cases], [(c.out_len, c.wb) for c in cases], [c.ref for c in cases])
    for i, c in enumerate(cases):
        e, o, r = oracle_lzxd(c.stream, c.out_len, c.wb, c.ref)
        assert res["err"][i] == e == c.err, (c.name, res[i], e)
        assert res["out_len"][i] == r.out_len and res["flags"][i] == r.flags and res["in_next"][i] == r.in_next, (c.name, res[i])
        got = out[units["out_off"][i]:units["out_off"][i] + r.out_len].tobytes()
        assert got == o[:r.out_len], c.name
        assert c.plain is None or got == c.plain, c.name


def check_mszip(cases):
    streams, lens, tabs, plains = [], [], [], []
    for c in cases:
        for tab in (c.tab, None):
            streams.append(c.stream); lens.append(c.out_len); tabs.append(tab); plains.append(c.plain)
    units, out, res = B.run(streams, lens, tabs)
    B.check(streams, lens, units, out, res, plains)
    for i, s in enumerate(streams):
        c = cases[i // 2]
        e, _o, r, _bl = oracle_mszip(s, lens[i])
        assert res["err"][i] == e == c.err, (c.name, res[i])
        assert res["in_next"][i] == r.in_next and (int(res["flags"][i]) & ~ADOPTED) == r.flags, (c.name, res[i], r.in_next, r.flags)


UF_HARD_EOF = 2                    # MSPACK_HIP_UF_HARD_EOF (include/mspack_hip.h)
QTM_PAD = 160                      # zero bytes behind every stream: more than the 96 the lean reader wants ahead of it


def qtm_arena(cases):
    """one copy of every stream, QTM_PAD zero bytes behind each -> (arena, offsets)"""
    offs, pos = [], 0
    for c in cases:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(c.stream) + QTM_PAD
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for c, o in zip(cases, offs):
        arena[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
    return arena, offs


def check_qtm_good_len(name, data, wb, hard, out_len, r):
    """a failing unit's good_len: a request that ends there succeeds, the next longer one fails as the unit did"""
    oracle_set_hard_eof(hard)
    try:
        g = int(r["good_len"])
        assert g <= out_len, (name, r)
        assert oracle_qtm(data, g, wb)[0] == 0, (name, "a request of good_len fails", r)
        if g < out_len:
            e1 = oracle_qtm(data, g + 1, wb)[0]
            assert e1 == r["err"], (name, "a request of good_len + 1 gives", e1, r)
    finally:
        oracle_set_hard_eof(0)


def check_qtm(cases):
    """every case three times: in_len exact (a tiny stream never leaves the exact reader), in_len extended over the zeros behind
    it (the lean reader runs up to the last token), exact with a failing feeder (MSPACK_HIP_UF_HARD_EOF)"""
    arena, offs = qtm_arena(cases)
    variants = [(0, 0), (QTM_PAD, 0), (0, UF_HARD_EOF)]
    rep = lambda v: np.repeat(np.asarray(v), len(variants))
    units, out_bytes = M.make_units(M.KIND_QUANTUM, rep(offs), rep([len(c.stream) for c in cases]), rep([c.out_len for c in cases]),
                                    window_bits=rep([c.wb for c in cases]))
    units["in_len"] += np.tile([v[0] for v in variants], len(cases)).astype(np.uint32)
    units["flags"] |= np.tile([v[1] for v in variants], len(cases)).astype(np.uint32)
    out, res = M.decode_batch(units, arena, out_bytes)
    for j, c in enumerate(cases):
        for k, (pad, flag) in enumerate(variants):
            i = len(variants) * j + k
            data = c.stream + bytes(pad)
            oracle_set_hard_eof(bool(flag))
            try:
                e, o, r = oracle_qtm(data, c.out_len, c.wb)
            finally:
                oracle_set_hard_eof(0)
            what = (c.name, ("exact", "extended", "hard_eof")[k], res[i], e, r.out_len, r.in_used)
            assert res["err"][i] == e and res["out_len"][i] == r.out_len, what
            got = out[units["out_off"][i]:units["out_off"][i] + r.out_len].tobytes()
            assert got == o[:r.out_len], what
            if k == 0:
                assert e == c.err, what
            if c.plain is not None and e == 0:
                assert got == c.plain, what
            assert res["in_used"][i] == r.in_used, what
            if e != 0:
                check_qtm_good_len(what[:2], data, c.wb, bool(flag), c.out_len, res[i])
            else:
                assert res["good_len"][i] == r.out_len, what


LZ_BELOW, LZ_GUARD = 4096, 64       # the window pre-fill below a unit's room; guard bytes between its room and the next unit


def lz_variants(c):
    """(room, in_off mod 16, out_off mod 16): every room of the case; a valid one at every residue of both offsets besides"""
    v = [(room, 0, 0) for room in c.rooms]
    if c.err == 0:
        v += [(c.rooms[0], k, (7 * k + 5) % 16) for k in range(16)]
    return v


def lz_oracle(c, room):
    return oracle_lzss(c.stream, c.wb, room) if c.codec == "lzss" else oracle_kwaj_lzh(c.stream, room)


def lz_batch(items, in_offs=None, arena=None):
    """the test's own layout for LZSS / LZH units.  items: (case, room, in_off mod 16, out_off mod 16).  Every unit gets its own
    copy of the stream at the residue asked for (unless in_offs / arena say where the streams are), LZ_BELOW bytes below its room
    and LZ_GUARD bytes behind it that belong to nobody -> (units, arena, bytes of output)"""
    if in_offs is None:
        in_offs, pos = [], 0
        for c, _room, ri, _ro in items:
            pos = ((pos + 15) & ~15) + ri
            in_offs.append(pos); pos += len(c.stream)
        arena = np.zeros(pos + 64, dtype=np.uint8)
        for (c, _room, _ri, _ro), o in zip(items, in_offs):
            arena[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
    kinds = np.array([M.KIND_LZSS if it[0].codec == "lzss" else M.KIND_KWAJ_LZH for it in items], dtype=np.uint8)
    units, _ = M.make_units(kinds, in_offs, [len(it[0].stream) for it in items], [it[1] for it in items],
                            window_bits=[it[0].wb for it in items])
    pos = LZ_GUARD
    for i, (_c, room, _ri, ro) in enumerate(items):
        base = pos + LZ_BELOW
        units["out_off"][i] = base + ((ro - base) % 16)
        pos = int(units["out_off"][i]) + room + LZ_GUARD
    return units, arena, pos


def to_device(units, arena, out_bytes):
    """the batch through mspack_hip_decode_batch_to_device into a device buffer full of 0xA5 -> (the buffer, results)"""
    d = DevBuf(out_bytes, fill=0xA5)
    res = np.zeros(len(units), dtype=M.RESULT_DTYPE)
    u = np.ascontiguousarray(units)
    rc = M.lib().mspack_hip_decode_batch_to_device(u.ctypes.data, len(u), arena.ctypes.data, arena.size, d.ptr, out_bytes, res.ctypes.data)
    assert rc == 0, M.lib().mspack_hip_last_error()
    out = d.to_host()
    d.free()
    return out, res


def check_lz(cases):
    """every case at every room and every residue, against the oracle: err, out_len (which may exceed the room), in_used, good_len,
    flags, every byte up to min(out_len, room) -- and against the helper's plaintext.  Then the same batch into a device buffer
    full of 0xA5: nothing but the pre-fill's spaces and those bytes may have changed in it."""
    if not cases:
        return
    items = [(c,) + v for c in cases for v in lz_variants(c)]
    units, arena, out_bytes = lz_batch(items)
    out, res = M.decode_batch(units, arena, out_bytes)
    want = np.full(out_bytes, 0xA5, dtype=np.uint8)
    for i, (c, room, ri, ro) in enumerate(items):
        e, o, r = lz_oracle(c, room)
        what = (c.name, "room %d of %d" % (room, c.out_len), (ri, ro), res[i], e, r.out_len, r.in_used)
        assert res["err"][i] == e == c.err and res["out_len"][i] == r.out_len == c.out_len, what
        assert res["in_used"][i] == r.in_used and res["good_len"][i] == r.out_len and res["flags"][i] == r.flags == 0, what
        n, oo = min(r.out_len, room), int(units["out_off"][i])
        assert units["in_off"][i] % 16 == ri and oo % 16 == ro
        assert out[oo:oo + n].tobytes() == o[:n] == c.plain[:n], what
        if not (c.codec == "lzss" and c.wb > 2):          # (a refused mode writes nothing at all)
            want[oo - LZ_BELOW:oo] = 0x20
        want[oo:oo + n] = np.frombuffer(o[:n], dtype=np.uint8)
    dev, res2 = to_device(units, arena, out_bytes)
    assert np.array_equal(res2, res)
    bad = np.flatnonzero(dev != want)
    if bad.size:
        i = int(np.searchsorted(units["out_off"].astype(np.int64) - LZ_BELOW, bad[0], side="right")) - 1
        c, room, ri, ro = items[max(i, 0)]
        raise AssertionError("byte %d of the device buffer is 0x%02X, not 0x%02X: %s, room %d, out_off %d (%d bytes differ)" % (
            bad[0], dev[bad[0]], want[bad[0]], c.name, room, units["out_off"][max(i, 0)], bad.size))


def check_lzss(cases):
    check_lz(cases)


def check_lzh(cases):
    check_lz(cases)


def check_all(cases):
    check_lzx([c for c in cases if c.codec == "lzx"])
    check_lzxd([c for c in cases if c.codec == "lzxd"])
    check_mszip([c for c in cases if c.codec == "mszip"])
    check_qtm([c for c in cases if c.codec == "qtm"])
    check_lzss([c for c in cases if c.codec == "lzss"])
    check_lzh([c for c in cases if c.codec == "lzh"])


def test_crafted_streams_vs_oracle(built):
    check_all(CS.all_cases())


def test_valid_lzx_cases_600_times_in_one_batch(built):
    """(the 600 units of a case share one copy of its stream and its table in the arena)
    What this batch runs: its cases have 1, 2, 3, 4 and 6 frames, so the launch is NOT uniform (entry_kernels.hpp: Fmin != Fmax, F == 0)
    and the ticket order is never consulted -- frame-slot order, one ticket per frame slot, parse and resolve by the same wave, with
    many more slots than the launch has waves, and headers read ahead of the chain (lzx_pipe_task_spec) wherever a frame's task
    starts before the frame below has published.  The three ticket orders of uniform launches, with hand-built, damaged and
    other-mode units in them, are tests/test_gpu_lzx_uniform.py's."""
    cases = [c for c in CS.lzx_cases() if c.err == 0]
    n = 600
    offs, toffs, pos = [], [], 0
    for c in cases:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(c.stream) + 8
        pos = (pos + 3) & ~3
        toffs.append(pos); pos += 4 * len(c.tab)
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for c, o, to in zip(cases, offs, toffs):
        arena[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
        arena[to:to + 4 * len(c.tab)] = np.asarray(c.tab, dtype=np.uint32).view(np.uint8)
    rep = lambda v: np.repeat(np.asarray(v), n)
    units, out_bytes = M.make_units(M.KIND_LZX, rep(offs), rep([len(c.stream) for c in cases]), rep([c.out_len for c in cases]),
                                    window_bits=rep([c.wb for c in cases]), reset_frames=rep([c.reset for c in cases]),
                                    frame_tabs=rep(toffs))
    out, res = M.decode_batch(units, arena, out_bytes)
    for j, c in enumerate(cases):
        e, _o, r = oracle_lzx(c.stream, c.out_len, c.wb, c.reset)
        want = np.frombuffer(c.plain, dtype=np.uint8)
        for i in range(j * n, (j + 1) * n):
            assert res["err"][i] == e == 0 and res["out_len"][i] == r.out_len and res["in_next"][i] == r.in_next, (c.name, i, res[i])
            assert (int(res["flags"][i]) & ~ADOPTED) == r.flags, (c.name, i, res[i])
            assert c.name not in MUST_ADOPT or res["flags"][i] & ADOPTED, (c.name, i, res[i])
            assert np.array_equal(out[units["out_off"][i]:units["out_off"][i] + c.out_len], want), (c.name, i)


def test_valid_qtm_cases_200_times_in_one_batch(built):
    """(the 200 units of a case share one copy of its stream; every third unit carries marks -- every 97th position and around every
    window end -- and so runs in the mark-bearing kernel)"""
    cases = [c for c in CS.qtm_cases() if c.err == 0 and c.out_len > 0]
    n = 200
    arena, offs = qtm_arena(cases)
    marks, toffs, pos = [], [], (len(arena) + 3) & ~3
    for c in cases:
        m = sorted(set(range(97, c.out_len, 97)) |
                   set((k << c.wb) + j for k in range(1, (c.out_len >> c.wb) + 1) for j in range(-4, 2) if 0 < (k << c.wb) + j < c.out_len))
        marks.append(m); toffs.append(pos); pos += 4 * len(m)
    arena = np.concatenate([arena, np.zeros(pos + 64 - len(arena), dtype=np.uint8)])
    for m, o in zip(marks, toffs):
        arena[o:o + 4 * len(m)] = np.asarray(m, dtype=np.uint32).view(np.uint8)
    rep = lambda v: np.repeat(np.asarray(v), n)
    units, _ = M.make_units(M.KIND_QUANTUM, rep(offs), rep([len(c.stream) + QTM_PAD for c in cases]), rep([c.out_len for c in cases]),
                            window_bits=rep([c.wb for c in cases]))
    marked = np.arange(len(units)) % 3 == 0
    units["flags"][marked] |= M.UF_QTM_MARKS
    units["in_chunk"] = np.where(marked, rep(toffs) // 4, 0)
    units["ref_len"] = np.where(marked, rep([len(m) for m in marks]), 0)
    # (room for the logs: 16 bytes of alignment + 4 bytes per mark behind a marked unit's output)
    sizes = ((units["out_len"].astype(np.int64) + 15) & ~15) + np.where(marked, 16 + 4 * units["ref_len"].astype(np.int64), 0)
    units["out_off"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    out, res = M.decode_batch(units, arena, int(sizes.sum()))
    for j, c in enumerate(cases):
        e, _o, r = oracle_qtm(c.stream + bytes(QTM_PAD), c.out_len, c.wb)
        _e, want_log = oracle_qtm_marks(c.stream + bytes(QTM_PAD), c.out_len, c.wb, marks[j])
        want = np.frombuffer(c.plain, dtype=np.uint8)
        for i in range(j * n, (j + 1) * n):
            assert res["err"][i] == e == 0 and res["out_len"][i] == r.out_len and res["in_used"][i] == r.in_used, (c.name, i, res[i])
            o = int(units["out_off"][i])
            assert np.array_equal(out[o:o + c.out_len], want), (c.name, i)
            if marked[i]:
                lo = o + ((c.out_len + 15) & ~15)
                assert out[lo:lo + 4 * len(marks[j])].view(np.uint32).tolist() == want_log, (c.name, i)


def test_valid_lzss_lzh_cases_300_times_in_one_batch(built):
    """(both kinds interleaved in one unit table; the 300 units of a case share one copy of its stream; every third unit has ample room
    and MSPACK_HIP_UF_CRC32 -- its in_used is the digest of tests/test_gpu_crc32.py --, the others the case's rooms in turn)"""
    cases = [c for c in CS.lz_cases() if c.err == 0]
    cases.sort(key=lambda c: int(zlib.crc32(c.name.encode())))          # (LZSS and LZH units mixed through the table)
    n = 300
    offs, pos = [], 0
    for c in cases:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(c.stream)
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for c, o in zip(cases, offs):
        arena[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
    items, in_offs = [], []
    for k in range(n):                                                    # (case-minor: neighbours in the table are of other cases)
        for j, c in enumerate(cases):
            room = c.rooms[0] if (k * len(cases) + j) % 3 == 0 else c.rooms[k % len(c.rooms)]
            items.append((c, room, 0, 0)); in_offs.append(offs[j])
    units, arena, out_bytes = lz_batch(items, in_offs, arena)
    crc = np.arange(len(units)) % 3 == 0
    units["flags"][crc] |= M.UF_CRC32
    assert {M.KIND_LZSS, M.KIND_KWAJ_LZH} == set(units["kind"][:16].tolist())
    out, res = M.decode_batch(units, arena, out_bytes)
    digest = [(zlib.crc32(c.plain) ^ 0xFFFFFFFF) & 0xFFFFFFFF for c in cases]
    plain = [np.frombuffer(c.plain, dtype=np.uint8) for c in cases]
    oo = units["out_off"].astype(np.int64)
    for i, (c, room, _ri, _ro) in enumerate(items):
        j = i % len(cases)
        what = (c.name, i, room, res[i])
        assert res["err"][i] == 0 and res["out_len"][i] == res["good_len"][i] == c.out_len and res["flags"][i] == 0, what
        assert res["in_used"][i] == (digest[j] if crc[i] else c.props["in_used"]), what
        m = min(room, c.out_len)
        assert np.array_equal(out[oo[i]:oo[i] + m], plain[j][:m]), what
