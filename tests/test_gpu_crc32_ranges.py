"""MSPACK_HIP_KIND_CRC32 (include/mspack_hip.h): digest units -- zlib's CRC-32 of a byte range of the output arena at any length, the
segments of all ranges of a batch one ticket space, behind everything else of the batch.  Everything goes through the C ABI; the
reference for a checksum is zlib.crc32 over the bytes that lie in the range, the reference for everything else is the same batch
without the range units.

tests/test_crc32_ranges_emu.py runs the first two groups of this file (lengths and alignments, one table of mixed sizes) on the
wavefront emulator."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import libmspack_amd as M
import test_gpu_crc32 as T
import test_gpu_md5 as D
from test_gpu_hostpath import DevBuf
from test_gpu_md5 import GUARD, dev_write

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 65536


def crc(b):
    return zlib.crc32(bytes(b)) & 0xFFFFFFFF


def run_device(data, ranges, order=None, extra_units=None, mask=None, expect_err=None):
    """range units over a device buffer that is exactly len(data) bytes long, inside a larger allocation of 0xA5: the call through
    mspack_hip_decode_batch_device (no decoding units), the results, and the checks that nothing but the results was written"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    units = M.crc32r_units(ranges)
    if extra_units is not None:
        units = np.concatenate([units, extra_units])
    big = DevBuf(n + 2 * GUARD, 0xA5)
    dev_write(big, GUARD, data)
    d_units, d_res = DevBuf(max(units.nbytes, 16)), DevBuf(max(len(units) * M.RESULT_DTYPE.itemsize, 16), 0x77)
    dev_write(d_units, 0, units.view(np.uint8))
    d_order = None
    if order is not None:
        o = np.ascontiguousarray(order, dtype=np.uint32)
        d_order = DevBuf(o.nbytes)
        dev_write(d_order, 0, o.view(np.uint8))
    L = M.lib()
    rc = L.mspack_hip_decode_batch_device(d_units.ptr, d_order.ptr if d_order else None, len(units), None, 0, big.ptr + GUARD, n,
                                          d_res.ptr, None, 0, M.MASK_CRC32R if mask is None else mask, None)
    assert rc == 0, L.mspack_hip_last_error()
    if big.emu is None:
        assert big.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(units) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE).copy()
    after = big.to_host()
    assert (after[:GUARD] == 0xA5).all() and (after[GUARD + n:] == 0xA5).all()          # the guard bytes
    assert np.array_equal(after[GUARD:GUARD + n], data)                                   # the arena after the call is the arena before it
    for b in (big, d_units, d_res) + ((d_order,) if d_order else ()):
        b.free()
    r = res[:len(ranges)]
    if expect_err is None:
        assert (r["err"] == 0).all()
    # the spare words are 0 when the pass has ended, whatever it kept in them meanwhile
    for f in ("flags", "in_used", "good_len", "in_next"):
        assert (r[f] == 0).all(), (f, r[r[f] != 0][:4])
    return res


def check(data, ranges, res):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    want = np.array([crc(data[o:o + n]) for o, n in ranges], dtype=np.uint32)
    got = res["out_len"][:len(ranges)]
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(int(i), ranges[int(i)], hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]


# ---- lengths and alignments ---------------------------------------------------------------------------------------------------

LENGTHS = [0, 1, 3, 15, 16, 17, 1023, 1024, 65535, 65536, 65537, 131072 + 5, 196608 - 1]


def lengths_layout():
    """every length at every out_off % 16: the slots start on multiples of 64, so the head bytes (out_off & 15) push 65536 - r .. 65536
    over a segment boundary"""
    ranges, pos = [], 0
    for n in LENGTHS:
        for r in range(16):
            pos = (pos + 63) & ~63
            ranges.append((pos + r, n))
            pos += r + n
    return ranges, pos


def test_lengths_and_alignments(built):
    """the edges of the row loader (15 / 16 / 17), of the lane slices (1023 / 1024) and of the 64 KiB segment, at out_off % 16 = 0 .. 15"""
    assert M.features() & M.FEAT_CRC32_RANGES
    ranges, total = lengths_layout()
    assert sorted(set(o % 16 for o, _n in ranges)) == list(range(16))
    data = np.random.default_rng(32).integers(0, 256, total, dtype=np.uint8)
    res = run_device(data, ranges)
    check(data, ranges, res)
    assert (res["out_len"][:16] == 0).all()                              # zlib.crc32(b"") == 0


# ---- one table, mixed sizes -----------------------------------------------------------------------------------------------------

def mixed_table():
    rng = np.random.default_rng(2020)
    long_n = 3 * (1 << 20) + 7
    total = long_n + 5000
    data = rng.integers(0, 256, total, dtype=np.uint8)
    ranges = [(int(rng.integers(0, total - 300)), int(rng.integers(1, 301))) for _ in range(1500)]
    ranges.append((1234 + 5, long_n))                                    # the long one: 49 segments beside 3000 of one
    ranges += [(int(rng.integers(0, total - 300)), int(rng.integers(1, 301))) for _ in range(1500)]
    ranges += [(1000, 200), (1100, 200), (1150, 70000), (1234 + 5 + 65536 * 3 - 9, 65536 + 30)]      # overlap each other and the long one
    ranges += [(777, 333), (777, 333)]                                   # two identical ranges
    ranges += [(5, 0), (total, 0)]
    return data, ranges


def test_mixed_sizes_in_one_table(built):
    """about 3000 ranges of 1 - 300 bytes, one of 3 MiB + 7 among them, overlapping and identical ranges: with d_order == NULL and
    with d_order shuffled; the spare result words of every range unit are 0 afterwards (run_device)"""
    data, ranges = mixed_table()
    check(data, ranges, run_device(data, ranges))
    perm = np.random.default_rng(9).permutation(len(ranges)).astype(np.uint32)
    check(data, ranges, run_device(data, ranges, order=perm))


def test_range_units_among_other_units_of_the_table(built):
    """a list in which whole blocks of 64 positions hold no range unit (units of kind 0, which no pass touches): in front of the
    first range unit, and between two groups of them"""
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 200000, dtype=np.uint8)
    ranges = [(int(rng.integers(0, 100000)), int(rng.integers(0, 90000))) for _ in range(70)]
    filler = np.zeros(400, dtype=M.UNIT_DTYPE)
    order = np.concatenate([np.arange(70, 270), np.arange(0, 35), np.arange(270, 470), np.arange(35, 70)]).astype(np.uint32)
    res = run_device(data, ranges, order=order, extra_units=filler)
    check(data, ranges, res)
    assert (res[70:].view(np.uint8) == 0x77).all()                       # the other units' results are nobody's here


# ---- arena edges ------------------------------------------------------------------------------------------------------------------

def test_arena_edges_and_guards(built):
    """ranges that end exactly at out_bytes, inside guard bytes (run_device checks them); a range one byte beyond it answers
    MSPACK_ERR_ARGS with zeros and costs the others nothing"""
    for n in (1, 61, 1027, 70001):
        data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        ranges = [(n - min(n, 37), min(n, 37)), (0, n), (n, 0), (n - 1, 1), (0, 1)]
        check(data, ranges, run_device(data, ranges))
        bad = [(0, n + 1), (n, 1), (n + 1, 0)]
        res = run_device(data, bad + ranges, expect_err=True)
        assert (res["err"][:3] == 1).all() and (res["out_len"][:3] == 0).all()
        assert (res["err"][3:] == 0).all()
        check(data, ranges, res[3:])


# ---- behind the decoders ----------------------------------------------------------------------------------------------------------

def mixed_batch(seed=3, n_each=1):
    """test_gpu_md5's batch: units of all six decoding kinds + one damaged LZX stream; per unit a range over its output, a ragged
    part of it, and one from the middle of the unit to the middle of the next one (the padding between them included)"""
    return D.mixed_batch(seed=seed, n_each=n_each)


def check_mixed(units, out, res, rres, ranges, plain_out, plain_res):
    assert np.array_equal(res, plain_res)
    for i in range(len(units)):
        o, n = int(units["out_off"][i]), int(plain_res["out_len"][i])
        assert np.array_equal(out[o:o + n], plain_out[o:o + n]), i
    assert (rres["err"] == 0).all()
    for f in ("flags", "in_used", "good_len", "in_next"):
        assert (rres[f] == 0).all(), f
    check(out, ranges, rres)


def test_behind_the_decoders(built):
    """one mixed batch through mspack_hip_decode_batch: the pass sees what every decoder stored (E8 and resume passes included), also
    what the damaged stream left -- the checksum is of the bytes that came back"""
    units, arena, out_bytes, refs, ranges = mixed_batch()
    assert sorted(set(int(k) for k in units["kind"])) == [1, 2, 3, 4, 5, 6]
    plain_out, plain_res = M.decode_batch(units, arena, out_bytes, refs=refs)
    assert plain_res["err"][-1] != 0 and (plain_res["err"][:-1] == 0).all()
    out, res, rres = M.decode_batch_crc32r(units, arena, out_bytes, ranges, refs=refs)
    check_mixed(units, out, res, rres, ranges, plain_out, plain_res)


def test_device_resident_entry_behind_the_decoders(built):
    """mspack_hip_decode_batch_device with decoding units of all six kinds (one stream damaged), range units and MD5 / SHA units in
    one table: without bit 20 no range unit's result is touched; with it the checksums are those of the bytes the call left, beside
    the MSPACK_HIP_MASK_CRC32 pass and the MD5 / SHA bits, and every other result and byte is that of the run without the new units"""
    units, arena, out_bytes, refs, ranges = mixed_batch(seed=21)
    nd, nr = len(units), len(ranges)
    wide, heads = M.digest_units(ranges[:6], [M.KIND_MD5, M.KIND_SHA1, M.KIND_SHA256] * 2)
    both = np.concatenate([units, M.crc32r_units(ranges), wide])
    fr = M.frames_of(both)
    both["frame_base"] = np.concatenate([[0], np.cumsum(fr)[:-1]])
    n_frames = int(fr.sum())
    L = M.lib()
    scratch = DevBuf(max(L.mspack_hip_frame_scratch_bytes(n_frames), 16))
    d_units, d_in = DevBuf(both.nbytes), DevBuf(arena.size + 64)
    dev_write(d_in, 0, arena)
    codecs = 0xFE

    def call(mask, flags=0):
        u = both.copy(); u["flags"][:nd] |= flags
        dev_write(d_units, 0, u.view(np.uint8))
        d_out, d_res = DevBuf(out_bytes + 64, 0xA5), DevBuf(len(both) * M.RESULT_DTYPE.itemsize, 0x77)
        for x, r in zip(units, refs):
            if len(r):
                dev_write(d_out, int(x["out_off"]) - len(r), np.frombuffer(r, dtype=np.uint8))
        rc = L.mspack_hip_decode_batch_device(d_units.ptr, None, len(both), d_in.ptr, arena.size, d_out.ptr, out_bytes, d_res.ptr,
                                              scratch.ptr, n_frames, mask, None)
        assert rc == 0, L.mspack_hip_last_error()
        if d_out.emu is None:
            assert d_out.hip.hipDeviceSynchronize() == 0
        out, res = d_out.to_host(), d_res.to_host().view(M.RESULT_DTYPE).copy()
        d_out.free(); d_res.free()
        return out, res

    digests = M.MASK_MD5 | M.MASK_SHA1 | M.MASK_SHA256
    out0, res0 = call(codecs | digests)
    assert res0["err"][nd - 1] != 0 and (res0["err"][:nd - 1] == 0).all()
    assert (res0[nd:nd + nr].view(np.uint8) == 0x77).all()                  # no bit 20: the range units' results are untouched
    out1, res1 = call(codecs | digests | M.MASK_CRC32R)
    assert np.array_equal(res1[:nd], res0[:nd]) and np.array_equal(res1[nd + nr:], res0[nd + nr:])
    check_mixed(units, out1, res1[:nd], res1[nd:nd + nr], ranges, out0, res0[:nd])
    # bit 20 alone: that pass only, over the buffer as it is
    out2, res2 = call(M.MASK_CRC32R)
    assert (res2[:nd].view(np.uint8) == 0x77).all() and (res2[nd + nr:].view(np.uint8) == 0x77).all()
    check(out2, ranges, res2[nd:nd + nr])
    # ... and beside the MSPACK_HIP_UF_CRC32 pass: both conventions of the same bytes
    out3, res3 = call(codecs | digests | M.MASK_CRC32R | M.MASK_CRC32, flags=M.UF_CRC32)
    check(out3, ranges, res3[nd:nd + nr])
    T.check_digests(units, out3, res3[:nd])
    for f in ("err", "flags", "out_len", "good_len", "in_next"):
        assert np.array_equal(res3[f][:nd], res0[f][:nd]), f
    assert np.array_equal(res3[nd + nr:], res0[nd + nr:])
    for i in range(nd - 1):
        if res0["out_len"][i] == units["out_len"][i] and units["out_len"][i]:
            o, n = int(units["out_off"][i]), int(units["out_len"][i])
            assert int(res3["in_used"][i]) == int(res3["out_len"][nd + ranges.index((o, n))]) ^ 0xFFFFFFFF, i
    for b in (scratch, d_units, d_in):
        b.free()


def test_to_device(built):
    """host input, device output: checksums of bytes that never came back -- compared after a copy of the test's own"""
    units, arena, out_bytes, refs, ranges = mixed_batch(seed=8)
    d_out = DevBuf(out_bytes + 64)
    for u, r in zip(units, refs):
        if len(r):
            dev_write(d_out, int(u["out_off"]) - len(r), np.frombuffer(r, dtype=np.uint8))
    both = np.concatenate([units, M.crc32r_units(ranges)])
    res = np.zeros(len(both), dtype=M.RESULT_DTYPE)
    rc = M.lib().mspack_hip_decode_batch_to_device(both.ctypes.data, len(both), arena.ctypes.data, arena.size, d_out.ptr, out_bytes + 64,
                                                   res.ctypes.data)
    assert rc == 0, M.lib().mspack_hip_last_error()
    assert (res["err"][len(units):] == 0).all()
    check(d_out.to_host(), ranges, res[len(units):])
    d_out.free()


def test_chunked_host_path(built):
    """a batch the planner cuts into chunks (test_gpu_md5's: 640 LZX units back to back): ranges that straddle every possible cut, one
    long range over 300 units, and the whole arena"""
    units, comp, out_bytes, plain, ranges = D.chunked_batch()
    ranges = ranges + [(0, out_bytes)]
    assert not [k for k in os.environ if k.startswith("MSPACK_HIP_CHUNK") or k == "MSPACK_HIP_NCHUNKS"]
    assert min(4, int(units["in_len"].sum()) // (8 << 20), len(units) // 256) >= 2
    out, res, rres = M.decode_batch_crc32r(units, comp, out_bytes, ranges)
    assert (res["err"] == 0).all() and np.array_equal(out[:plain.size], plain)
    assert (rres["err"] == 0).all()
    check(plain, ranges, rres)


WORKER = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import libmspack_amd as M
import test_gpu_md5 as D
import test_gpu_crc32_ranges as R
mode = sys.argv[1]
units, arena, out_bytes, refs, ranges = R.mixed_batch(seed=12, n_each=3)
if mode == "jobs":
    assert os.environ["MSPACK_PY_VIA_JOBS"] == "1"
    # waiting on a range unit FIRST: it returns when the batch is through, with the checksum written
    both = np.concatenate([units, M.crc32r_units(ranges)])
    out = np.zeros(out_bytes, dtype=np.uint8)
    for u, r in zip(units, refs):
        if len(r):
            out[int(u["out_off"]) - len(r):int(u["out_off"])] = np.frombuffer(r, dtype=np.uint8)
    res = np.zeros(len(both), dtype=M.RESULT_DTYPE); res["err"] = 0x7777
    L = M.lib()
    job = L.mspack_hip_decode_batch_begin(both.ctypes.data, len(both), arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data)
    assert job
    assert L.mspack_hip_job_wait_unit(job, len(units) + 1) == 0
    assert (res["err"] != 0x7777).all()
    first = res[len(units):].copy()
    assert L.mspack_hip_job_end(job) == 0
    R.check(out, ranges, first)
    n_dev = 1
else:
    assert os.environ["MSPACK_HIP_FORCE_SHARDS"] in ("2", "3")
    n_dev = 2
plain_out, plain_res = M.decode_batch(units, arena, out_bytes, refs=refs, n_devices=n_dev)
out, res, rres = M.decode_batch_crc32r(units, arena, out_bytes, ranges, refs=refs, n_devices=n_dev)
R.check_mixed(units, out, res, rres, ranges, plain_out, plain_res)
# a batch of equal units: the even cuts fall behind unit n / 2 (n / 3, 2 n / 3) -- with a range across each of them: never cut
units, comp, out_bytes, plain, ranges = D.chunked_batch()
n, ub = len(units), 65536
ranges = ranges + [(k * ub - 5000, 10000) for k in (n // 2, n // 3, 2 * n // 3, n // 2 + 1, n // 3 + 1, 2 * n // 3 + 1)]
out, res, rres = M.decode_batch_crc32r(units, comp, out_bytes, ranges, n_devices=n_dev)
assert (res["err"] == 0).all() and np.array_equal(out[:plain.size], plain)
assert (rres["err"] == 0).all()
R.check(plain, ranges, rres)
print("CRC32R_WORKER_OK")
'''


@pytest.mark.parametrize("mode,env", [("shards", {"MSPACK_HIP_FORCE_SHARDS": "2"}), ("shards", {"MSPACK_HIP_FORCE_SHARDS": "3"}),
                                      ("jobs", {"MSPACK_PY_VIA_JOBS": "1", "MSPACK_HIP_TRACE": "1"})])
def test_sharded_and_job_entry_points(built, mode, env, tmp_path):
    """mspack_hip_decode_batch_multi cut into two and three shards with ranges where the even cuts would fall, and _begin /
    _wait_unit / _end waiting on a range unit first -- in a fresh process so that the environment switch is seen"""
    script = tmp_path / "w.py"
    script.write_text(WORKER % (ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script), mode], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0 and b"CRC32R_WORKER_OK" in p.stdout, p.stdout.decode()[-3000:]
    if mode == "jobs":
        # the library's own trace: the chunked batch (640 units beside its range units) was cut into at least two chunks
        cuts = [int(m.group(2)) for m in re.finditer(rb"(\d+) units in (\d+) chunks", p.stdout) if int(m.group(1)) > 640]
        assert cuts and max(cuts) >= 2, p.stdout.decode()[-3000:]


# ---- rejections, the feature bit, the constants ---------------------------------------------------------------------------------------

def test_rejections(built):
    """a range one byte beyond out_bytes, in_len = 1, the CRC flag: an error return with the unit's index in the message, before
    anything is touched; every other flag is ignored"""
    arena = np.zeros(256, dtype=np.uint8)
    good = M.crc32r_units([(0, 64), (10, 20)])
    for change, msg in ((lambda u: u["out_len"].__setitem__(1, 55), "unit 1: a digest unit's range leaves the output arena"),
                        (lambda u: u["out_off"].__setitem__(1, 65), "unit 1: a digest unit's range leaves the output arena"),
                        (lambda u: u["in_len"].__setitem__(1, 1), "unit 1: a digest unit reads no input"),
                        (lambda u: u["flags"].__setitem__(1, M.UF_CRC32), "unit 1: a digest unit decodes nothing to take a CRC-32 of")):
        u = good.copy()
        change(u)
        out = np.full(64, 0x5A, dtype=np.uint8)
        res = np.zeros(2, dtype=M.RESULT_DTYPE); res["err"] = 0x7777; res["in_next"] = 0x1234
        before = res.copy()
        rc = M.lib().mspack_hip_decode_batch(u.ctypes.data, 2, arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data)
        assert rc != 0 and msg in M.lib().mspack_hip_last_error().decode(), M.lib().mspack_hip_last_error()
        assert np.array_equal(res, before) and (out == 0x5A).all()
    u = good.copy(); u["flags"][1] = 0x7F
    out = np.zeros(64, dtype=np.uint8)
    res = np.zeros(2, dtype=M.RESULT_DTYPE)
    assert M.lib().mspack_hip_decode_batch(u.ctypes.data, 2, arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data) == 0
    assert (res["err"] == 0).all() and (res["flags"] == 0).all()
    # kind 19 stays unknown
    u = good.copy(); u["kind"][0] = 19
    assert M.lib().mspack_hip_decode_batch(u.ctypes.data, 2, arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data) != 0
    assert "unknown kind 19" in M.lib().mspack_hip_last_error().decode()


def test_feature_bit_and_constants(built):
    assert M.KIND_CRC32R == 20 and M.FEAT_CRC32_RANGES == 64 and M.MASK_CRC32R == 1 << 20
    assert M.features() & M.FEAT_CRC32_RANGES
    hdr = open(os.path.join(ROOT, "include", "mspack_hip.h")).read()
    assert re.search(r"#define\s+MSPACK_HIP_KIND_CRC32\s+20\b", hdr) and re.search(r"#define\s+MSPACK_HIP_FEAT_CRC32_RANGES\s+64u\b", hdr)
