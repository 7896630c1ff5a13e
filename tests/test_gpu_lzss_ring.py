"""LZSS units that carry MSPACK_HIP_UF_LZSS_RING (the window in LDS, nothing owned below out_off; lzss_ring_kernel.hpp) against
helpers.oracle_lzss.  The units of a batch are PACKED: the first at out_off 0, the others at the alignments 1..15 in turn, each right
behind the room of the one before (0 to 15 bytes in between that belong to nobody), the whole through
mspack_hip_decode_batch_to_device into a device buffer full of 0xA5 -- a store below a unit, behind its room or past min(out_len, room)
lands in a neighbour or in the fill and is seen.  Compared: all six result words and every byte of the image that the contract speaks
of (include/mspack_hip.h: the first min(unit.out_len, result.out_len) bytes; nothing outside [out_off, out_off + unit.out_len)).

tests/test_lzss_ring_emu.py runs the first three tests on the wavefront emulator.

Whether the ring kernel was launched for a batch is not observable from outside the library (no launch accounting exists in the
diagnostics); test_batch_without_the_flag therefore checks what IS observable -- the unflagged kernel's footprint, 4096 spaces below
every unit -- and tests/test_host_plan_lzss.py checks the planner's decision (Chunk::has_lzss_ring), which is the launch condition."""
import functools

import numpy as np
import pytest

import crafted_streams as CS
import footprint as F
import libmspack_amd as M
import szdd_kwaj_recipe as R
from helpers import oracle_kwaj_lzh, oracle_lzss
from test_gpu_hostpath import DevBuf
from test_gpu_md5 import dev_write

pytestmark = pytest.mark.gpu
FILL = 0xA5
RING = M.UF_LZSS_RING


def pack(specs, first_align=0):
    """specs: [(stream, mode, room, in_off residue)] -> (units, arena, out_bytes): flagged units, no room below, unit i at alignment
    (first_align + i) mod 16 right behind unit i - 1's room"""
    in_offs, pos = [], 0
    for s, _m, _room, ri in specs:
        pos = ((pos + 15) & ~15) + ri
        in_offs.append(pos); pos += len(s)
    arena = np.full(pos + 64, 0xFF, dtype=np.uint8)
    for (s, _m, _room, _ri), o in zip(specs, in_offs):
        arena[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    u = np.zeros(len(specs), dtype=M.UNIT_DTYPE)
    u["in_off"], u["in_len"] = in_offs, [len(s[0]) for s in specs]
    u["kind"], u["window_bits"], u["flags"] = M.KIND_LZSS, [s[1] for s in specs], RING
    pos = 0
    for i, (_s, _m, room, _ri) in enumerate(specs):
        pos += ((first_align + i) - pos) % 16
        u["out_off"][i], u["out_len"][i] = pos, room
        pos += room
    return u, arena, pos + 64                  # (64 bytes of fill behind the last room)


def to_device(units, arena, out_bytes):
    d = DevBuf(max(out_bytes, 16), fill=FILL)
    res = np.zeros(len(units), dtype=M.RESULT_DTYPE)
    u = np.ascontiguousarray(units)
    rc = M.lib().mspack_hip_decode_batch_to_device(u.ctypes.data, len(u), arena.ctypes.data, arena.size, d.ptr, out_bytes, res.ctypes.data)
    assert rc == 0, M.lib().mspack_hip_last_error()
    out = d.to_host()
    d.free()
    return out, res


def check_packed(specs, names=None, want_err=None, first_align=0):
    """the packed batch against the oracle: six result words, the bytes, and the fill wherever the contract lets nobody write"""
    units, arena, out_bytes = pack(specs, first_align)
    assert units["out_off"][0] == first_align and (len(specs) < 17 or set(int(x) % 16 for x in units["out_off"]) == set(range(16)))
    img, res = to_device(units, arena, out_bytes)
    want = np.full(img.size, FILL, dtype=np.uint8)
    free = np.zeros(img.size, dtype=bool)     # unspecified: the rest of a unit's own room
    for i, (s, mode, room, _ri) in enumerate(specs):
        what = (i, names[i] if names else "", "mode %d, room %d, out_off %d" % (mode, room, units["out_off"][i]), res[i])
        if mode > 2:
            assert tuple(res[i]) == (M.ERR_ARGS, 0, 0, 0, 0, 0), what
            continue
        e, o, r = oracle_lzss(s, mode, room)
        assert want_err is None or e == want_err[i], what
        assert (res["err"][i], res["flags"][i], res["out_len"][i]) == (e, 0, r.out_len), what + (r.out_len,)
        assert (res["in_used"][i], res["good_len"][i], res["in_next"][i]) == (r.in_used, r.out_len, 0), what + (r.in_used,)
        n, oo = min(r.out_len, room), int(units["out_off"][i])
        want[oo:oo + n] = np.frombuffer(o[:n], dtype=np.uint8)
        free[oo + n:oo + room] = True
    bad = np.flatnonzero((img != want) & ~free)
    if bad.size:
        i = max(int(np.searchsorted(units["out_off"].astype(np.int64), bad[0], side="right")) - 1, 0)
        raise AssertionError("byte %d of the image is 0x%02X, not 0x%02X: unit %d (%s) at out_off %d, room %d; %d bytes differ" % (
            bad[0], img[bad[0]], want[bad[0]], i, names[i] if names else "", units["out_off"][i], units["out_len"][i], bad.size))
    return units, res


# ---- the corpus of test_szdd_kwaj.py::test_lzss_kernel_vs_oracle ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus():
    from test_gpu_fuzz import mutations
    rng = np.random.default_rng(31)
    out = []
    for mode in (0, 1, 2):
        for x in R.texts():
            c = R.lzss_encode(x, mode)
            for v in [c] + mutations(c, rng, 12) if len(c) > 4 else [c]:
                out.append((bytes(v), mode))
    return out


def test_corpus_vs_oracle(built):
    specs = [(s, mode, len(s) * 9 + 64, (3 * i) % 16) for i, (s, mode) in enumerate(corpus())]
    check_packed(specs)


# ---- hand-built streams --------------------------------------------------------------------------------------------------------------
def ring_cases():
    """what the ring adds to crafted_streams.lzss_cases() -> [Case]"""
    C = []
    nz = CS._nz
    for m in (0, 1, 2):
        z = CS.Lzss(m); z.lits(nz(40 + m, 4200)); z.match(4096, 18); z.lit(0x31); z.match(4096, 3); z.match(4095, 18)
        C.append(CS._lzss_case("ring_source_exactly_4096_back_mode%d" % m, z))
        z = CS.Lzss(m); z.lit(0x51); z.match(1, 18); z.lit(0x52); z.match(1, 18); z.match(1, 18)
        C.append(CS._lzss_case("ring_distance_1_length_18_mode%d" % m, z))
    for m in (0, 2):                     # out of the space pre-fill, from both start positions
        z = CS.Lzss(m)
        for d in (16, 18, 100, 4096, 1, 17, 19):
            z.match(d, 18); z.lit(0x61 + (d & 15))
        z.raw(0, 18); z.raw(4095, 18); z.raw(4078, 7); z.raw(4080, 7)
        C.append(CS._lzss_case("ring_matches_out_of_the_prefill_mode%d" % m, z))
    for m in (0, 2):                     # the ring wraps at output byte 16 (18), then every 4096
        first = 18 if m == 2 else 16
        for lap in (0, 1):
            z = CS.Lzss(m)
            z.lits(nz(50 + m, first + 4096 * lap - 8))            # 8 bytes in front of the wrap
            z.match(20, 18)                                       # destination crosses the wrap
            z.lits(b"wrapped")
            z.match(30, 18)                                       # source crosses the wrap
            z.match(4096 - 5, 18)                                 # a source that begins 4091 back and crosses the NEXT wrap position
            C.append(CS._lzss_case("ring_wrap_crossed_by_destination_and_source_lap%d_mode%d" % (lap, m), z))
    # more than three ring lengths of output: flushes and wraps interleave; far sources right behind what later items overwrite
    for m in (0, 1, 2):
        z = CS.Lzss(m)
        z.lits(nz(60 + m, 4200))
        r = np.random.default_rng(60 + m)
        while len(z.plain) < 3 * 4096 + 1500:
            k = int(r.integers(0, 6))
            if k == 0:
                z.lits(nz(len(z.plain), int(r.integers(1, 9))))
            elif k == 1:
                z.match(4096 - int(r.integers(0, 40)), int(r.integers(3, 19)))          # old bytes that this group's later items overwrite
            elif k == 2:
                z.match(int(r.integers(1, 20)), 18)
            else:
                z.match(int(r.integers(1, 4097)), int(r.integers(3, 19)))
        C.append(CS._lzss_case("ring_more_than_three_ring_lengths_mode%d" % m, z))
        assert len(z.plain) >= 12289
    # a match 4096 - j back followed by literals of the same group: the source is what those literals overwrite
    z = CS.Lzss(0); z.lits(nz(70, 4300))
    for j in range(1, 60):
        z.match(4096 - j % 17, 3 + j % 16); z.lits(nz(70 + j, 7))
    C.append(CS._lzss_case("ring_far_source_in_front_of_later_literals", z))
    # cut inside a match's two bytes, in_len 0 and 1
    z = CS.Lzss(0); z.lits(b"abcdefg"); z.match(3, 5); z.lits(b"tail")
    s = z.stream()
    for cut in (0, 1, 8, 9, 10):
        C.append(CS._lzss_case("ring_cut_at_%d" % cut, z, cut=cut))
    assert s[8:10] == z.items[7][1] and not z.items[7][0]         # (cut 9: between the match's two bytes)
    return C


def refill_cases():
    """ONE long stream and 16 copies of it with 1..16 literals in front, so that the items meet the refill edges of the input stage
    (16-byte rows of the arena) at every phase"""
    out = []
    for shift in range(17):
        z = CS.Lzss(0)
        z.lits(CS._nz(90, shift))
        r = np.random.default_rng(91)
        while len(z.items) < 8 * 700:                             # about 8 KiB of input: eight refills and more
            if r.random() < 0.5:
                z.lit(int(r.integers(1, 255)) | 1)
            else:
                z.match(int(r.integers(1, min(4096, len(z.plain) + 17) + 1)), int(r.integers(3, 19)))
        out.append(CS._lzss_case("ring_refill_edges_shift_%d" % shift, z))
    return out


def test_crafted_streams(built):
    cases = CS.lzss_cases() + ring_cases()
    specs, names, errs = [], [], []
    for c in cases:
        for room in c.rooms:
            specs.append((c.stream, c.wb, room, (5 * len(specs) + 3) % 16)); names.append(c.name); errs.append(c.err)
    units, res = check_packed(specs, names, errs)
    i = 0
    for c in cases:                      # ... and against the helper's own plaintext and lengths
        for room in c.rooms:
            assert res["out_len"][i] == c.out_len and res["in_used"][i] == c.props["in_used"], (c.name, room, res[i])
            i += 1
    # the refill edges: the unshifted stream at every residue of in_off, the shifted ones at residues of their own
    cases = refill_cases()
    cases = [(cases[0], ri) for ri in range(16)] + [(c, (5 * k + 3) % 16) for k, c in enumerate(cases[1:])]
    specs = [(c.stream, c.wb, c.out_len, ri) for c, ri in cases]
    units, res = check_packed(specs, [c.name for c, _ri in cases], first_align=5)
    assert all(res["out_len"][k] == c.out_len > 12288 for k, (c, _ri) in enumerate(cases))


# ---- the room, cut at every length ---------------------------------------------------------------------------------------------------
def test_room_cut_at_every_length(built):
    """one stream, out_len = 0 .. produced + 1: result.out_len is always the full length, the prefix exact, nothing behind the room"""
    z = CS.Lzss(2)
    z.match(18, 18); z.lits(CS._nz(7, 200))
    for k in range(40):
        z.match(1 + 37 * k % 300, 3 + k % 16); z.lits(CS._nz(k, k % 5))
    c = CS._lzss_case("room_cut", z)
    assert 600 < c.out_len < 1200
    specs = [(c.stream, c.wb, room, room % 16) for room in range(c.out_len + 2)]
    units, res = check_packed(specs)
    assert (res["out_len"] == c.out_len).all() and (res["err"] == 0).all()
    # ... and in the guarded layout of tests/footprint.py: 1024 guard bytes that belong to nobody around every room, out_off at the
    # residues mod 128 of that file; the whole image is compared, only the rest of a unit's own room is unspecified
    items = []
    for room in range(c.out_len + 2):
        e, o, r = oracle_lzss(c.stream, c.wb, room)
        items.append(F.Item("room %d of %d" % (room, c.out_len), M.KIND_LZSS, c.stream, room, wb=c.wb, flags=RING, ri=(5 * room + 3) % 16,
                            ro=F.RESIDUES[room % len(F.RESIDUES)], want=F.Want(e, 0, r.out_len, 0, r.in_used, o)))
    L = F.layout(items)
    wants = [it.want for it in items]
    exp, mask = F.expected_image(L, wants, FILL)
    img, res = to_device(L.units, L.arena, L.out_bytes)
    F.check_results(L, res, wants)
    F.compare(img, exp, mask, L)
    assert all(res["in_used"][i] == len(c.stream) for i in range(len(items)))


# ---- mixed batches -------------------------------------------------------------------------------------------------------------------
def mixed_units():
    t = R.texts()
    lz = [R.lzss_encode(t[2], m) for m in (0, 1, 2)] + [R.lzss_encode(t[3], 0)]
    lzh = [R.lzh_encode(t[2], (3, 3, 3, 3, 3)), R.lzh_encode(t[1][:5000], (1, 2, 3, 1, 2))]
    mz = R.kwaj_mszip(t[1])
    streams = [(M.KIND_LZSS, s, m, RING, len(s) * 9 + 64) for m, s in zip((0, 1, 2, 0), lz)]
    streams += [(M.KIND_LZSS, s, m, 0, len(s) * 9 + 64) for m, s in zip((0, 1, 2, 0), lz)]
    streams += [(M.KIND_KWAJ_LZH, s, 0, 0, len(s) * 18 + 4096) for s in lzh]
    streams += [(M.KIND_MSZIP, mz, 0, 4, 32768)]                  # MSPACK_HIP_UF_MSZIP_KWAJ
    order = [0, 4, 8, 1, 10, 5, 9, 2, 6, 3, 7]                    # kinds and flags interleaved through the table
    return [streams[i] for i in order]


def build(streams):
    offs, pos = [], 0
    for _k, s, _m, _f, _room in streams:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(s)
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for (_k, s, _m, _f, _room), o in zip(streams, offs):
        arena[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    units, out_bytes = M.make_units(np.array([x[0] for x in streams], dtype=np.uint8), offs, [len(x[1]) for x in streams],
                                    [x[4] for x in streams], window_bits=[x[2] for x in streams],
                                    flags=np.array([x[3] for x in streams], dtype=np.uint32), out_slack=32768)
    return units, arena, out_bytes


def region(out, units, i, n):
    o = int(units["out_off"][i])
    return out[o:o + n].tobytes()


def test_mixed_batch(built, monkeypatch):
    """flagged LZSS, unflagged LZSS, LZH and a KWAJ-framed MSZIP unit in one batch: each answers as it does alone -- through the host
    entry, jobs, shards, the device-output entry and the device-resident entry"""
    streams = mixed_units()
    units, arena, out_bytes = build(streams)
    assert units["out_off"][0] == 0 and units["flags"][0] == RING           # (a flagged unit first: nothing below it)
    alone = []
    for x in streams:
        u1, a1, ob1 = build([x])
        o1, r1 = M.decode_batch(u1, a1, ob1)
        alone.append((r1[0], region(o1, u1, 0, min(int(r1["out_len"][0]), x[4]))))
        if x[0] == M.KIND_LZSS:
            e, o, r = oracle_lzss(x[1], x[2], x[4])
            assert (r1["err"][0], r1["out_len"][0], r1["in_used"][0]) == (e, r.out_len, r.in_used) and alone[-1][1] == o
    assert all(a[0]["err"] == 0 and a[0]["out_len"] > 0 for a in alone)

    def same(out, res, what):
        for i, (r1, b1) in enumerate(alone):
            assert tuple(res[i]) == tuple(r1), (what, i, res[i], r1)
            assert region(out, units, i, len(b1)) == b1, (what, i)
    same(*M.decode_batch(units, arena, out_bytes), "host")
    monkeypatch.setenv("MSPACK_PY_VIA_JOBS", "1")
    same(*M.decode_batch(units, arena, out_bytes), "jobs")
    monkeypatch.delenv("MSPACK_PY_VIA_JOBS")
    monkeypatch.setenv("MSPACK_HIP_FORCE_SHARDS", "3")
    same(*M.decode_batch(units, arena, out_bytes, n_devices=2), "shards")
    monkeypatch.delenv("MSPACK_HIP_FORCE_SHARDS")
    same(*to_device(units, arena, out_bytes), "to_device")
    # the device-resident entry: the mask names the kinds and says that LZSS units may carry the flag
    lib = M.lib()
    d_units, d_in, d_out = DevBuf(units.nbytes), DevBuf(arena.size + 64, 0xFF), DevBuf(out_bytes, FILL)
    d_res = DevBuf(len(units) * M.RESULT_DTYPE.itemsize, 0x77)
    dev_write(d_units, 0, np.ascontiguousarray(units).view(np.uint8))
    dev_write(d_in, 0, arena)
    mask = (1 << M.KIND_LZSS) | (1 << M.KIND_KWAJ_LZH) | (1 << M.KIND_MSZIP) | M.MASK_LZSS_RING
    rc = lib.mspack_hip_decode_batch_device(d_units.ptr, None, len(units), d_in.ptr, arena.size, d_out.ptr, out_bytes, d_res.ptr, None, 0, mask, None)
    assert rc == 0, lib.mspack_hip_last_error()
    if d_out.emu is None:
        assert d_out.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(units) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE).copy()
    same(d_out.to_host(), res, "device")
    for b in (d_units, d_in, d_out, d_res):
        b.free()


def test_batch_without_the_flag(built):
    """no unit carries the flag: results and bytes are the oracle's (what the parent gave), and every unit has the unflagged kernel's
    footprint -- 4096 spaces below it.  (That the ring kernel was not launched cannot be seen from outside: see the module's text.)"""
    streams = [x for x in mixed_units() if x[3] != RING]
    units, arena, out_bytes = build(streams)
    img, res = to_device(units, arena, out_bytes)
    for i, x in enumerate(streams):
        if x[0] == M.KIND_MSZIP:
            continue
        e, o, r = oracle_lzss(x[1], x[2], x[4]) if x[0] == M.KIND_LZSS else oracle_kwaj_lzh(x[1], x[4])
        assert (res["err"][i], res["out_len"][i], res["in_used"][i], res["good_len"][i]) == (e, r.out_len, r.in_used, r.out_len), (i, res[i])
        assert region(img, units, i, r.out_len) == o, i
        oo = int(units["out_off"][i])
        assert (img[oo - 4096:oo] == 0x20).all(), i


def test_feature_bit(built):
    assert M.features() & M.FEAT_LZSS_RING and M.FEAT_LZSS_RING == 32 and M.UF_LZSS_RING == 256
