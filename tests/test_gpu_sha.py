"""MSPACK_HIP_KIND_SHA1 / _SHA256 (include/mspack_hip.h): wide digest units -- the SHA-1 / SHA-256 of a byte range of the output arena,
one lane per range, one pass per algorithm behind everything else of the batch; bytes 16 .. of a digest come back in the result of
the MSPACK_HIP_KIND_DIGEST_MORE unit behind the head.  Everything goes through the C ABI; the reference for a digest is hashlib over
the bytes that lie in the range, the reference for everything else is the same batch without the SHA units.

tests/test_sha_emu.py runs the first three groups of this file (lengths and alignments, the FIPS strings, batch shapes) on the
wavefront emulator."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libmspack_amd as M
import test_gpu_crc32 as T
import test_gpu_md5 as G5
from test_gpu_hostpath import DevBuf
from test_gpu_md5 import dev_write

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
HASH = {M.KIND_MD5: hashlib.md5, M.KIND_SHA1: hashlib.sha1, M.KIND_SHA256: hashlib.sha256}
MASK = {M.KIND_MD5: M.MASK_MD5, M.KIND_SHA1: M.MASK_SHA1, M.KIND_SHA256: M.MASK_SHA256}
SHA = [M.KIND_SHA1, M.KIND_SHA256]

# FIPS 180-4's example messages: empty, "abc", the 448-bit and the 896-bit one
FIPS = [b"", b"abc", b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq",
        b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu"]
FIPS_SHA1 = ["da39a3ee5e6b4b0d3255bfef95601890afd80709", "a9993e364706816aba3e25717850c26c9cd0d89d",
             "84983e441c3bd26ebaae4aa1f95129e5e54670f1", "a49b2446a02c645bf419f995b67091253a04a259"]
FIPS_SHA256 = ["e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
               "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad",
               "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1",
               "cf5b16a778af8380036ce59e7b0492370b249b11e8f07a51afac45037afee9d1"]


def kinds_of(kinds, n):
    return [kinds] * n if isinstance(kinds, int) else list(kinds)


def check(data, ranges, kinds, got):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    assert len(got) == len(ranges)
    for (o, n), k, d in zip(ranges, kinds_of(kinds, len(ranges)), got):
        assert d == HASH[k](data[o:o + n].tobytes()).digest(), (k, o, n, d.hex())


def check_tails(units, res):
    """a tail's result: err 0, flags 0, the words the digest does not use 0 (SHA-1: everything behind out_len)"""
    for i in np.flatnonzero(units["kind"] == M.KIND_DIGEST_MORE):
        assert res["err"][i] == 0 and res["flags"][i] == 0, res[i]
        if units["kind"][i - 1] == M.KIND_SHA1:
            assert res["in_used"][i] == 0 and res["good_len"][i] == 0 and res["in_next"][i] == 0, res[i]


def run_device_raw(data, units, mask, order=None):
    """a unit table over a device buffer that is exactly len(data) bytes long, inside a larger allocation of 0xA5, through
    mspack_hip_decode_batch_device (no decoding units) -> the results (0x77 where nothing was written); checks that nothing but the
    results was written"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
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
                                          d_res.ptr, None, 0, mask, None)
    assert rc == 0, L.mspack_hip_last_error()
    if big.emu is None:
        assert big.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(units) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE).copy()
    after = big.to_host()
    assert (after[:GUARD] == 0xA5).all() and (after[GUARD + n:] == 0xA5).all()          # the guard bytes
    assert np.array_equal(after[GUARD:GUARD + n], data)                                   # the arena after the call is the arena before it
    for b in (big, d_units, d_res) + ((d_order,) if d_order else ()):
        b.free()
    return res


def run_device(data, ranges, kinds, order=None):
    """digest units of `kinds` over the ranges -> the digests in range order"""
    kinds = kinds_of(kinds, len(ranges))
    units, _heads = M.digest_units(ranges, kinds)
    mask = 0
    for k in set(kinds):
        mask |= MASK[k]
    res = run_device_raw(data, units, mask, order)
    assert (res["err"] == 0).all() and (res["flags"] == 0).all(), res
    check_tails(units, res)
    return M.result_wide_digests(res, units)


LENGTHS = [0, 1, 3, 4, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 191, 1000]


def lengths_layout(lengths):
    ranges, pos = [], 0
    for n in lengths:
        for r in range(16):
            pos = (pos + 63) & ~63
            ranges.append((pos + r, n))
            pos += r + n
    return ranges, pos


@pytest.mark.parametrize("kind", SHA)
def test_lengths_and_alignments(built, kind):
    """every length at which the pad changes its path (55 / 56 / 57 and 119 / 120: one final block or two; 63 / 64 / 65, 127 / 128 /
    129, 191: the block edges) at every out_off mod 16: the row, dword and funnel-shift loaders' first and last words"""
    assert M.features() & (M.FEAT_SHA1 if kind == M.KIND_SHA1 else M.FEAT_SHA256)
    ranges, total = lengths_layout(LENGTHS)
    assert sorted(set(o % 16 for o, _n in ranges)) == list(range(16)) and len(ranges) == 16 * len(LENGTHS)
    data = np.random.default_rng(1804).integers(0, 256, total, dtype=np.uint8)
    check(data, ranges, kind, run_device(data, ranges, kind))


def test_fips_strings(built):
    """FIPS 180-4's example messages back to back in one arena (so at four different alignments), both algorithms in one table"""
    data = np.frombuffer(b"".join(FIPS), dtype=np.uint8)
    ranges, pos = [], 0
    for s in FIPS:
        ranges.append((pos, len(s))); pos += len(s)
    got = run_device(data, ranges * 2, [M.KIND_SHA1] * 4 + [M.KIND_SHA256] * 4)
    assert [d.hex() for d in got] == FIPS_SHA1 + FIPS_SHA256


@pytest.mark.parametrize("n_units", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", SHA)
def test_batch_shapes(built, kind, n_units):
    """n heads of one algorithm and n different lengths, shuffled and descending: a last wave with one live lane, loops that end at a
    different count in every lane; the same batch again through a d_order permutation of the whole table (tails included)"""
    rng = np.random.default_rng(200 + n_units)
    lens = [(11 * i + 5) % 1499 + (i == 0) * 2000 for i in range(n_units)]
    assert len(set(lens)) == n_units
    data = rng.integers(0, 256, 4096, dtype=np.uint8)
    shuffled = [(int(rng.integers(0, 4096 - n)), n) for n in (lens[k] for k in rng.permutation(n_units))]
    descending = sorted(shuffled, key=lambda r: -r[1])
    for ranges in (shuffled, descending):
        check(data, ranges, kind, run_device(data, ranges, kind))
    perm = rng.permutation(2 * n_units).astype(np.uint32)
    check(data, shuffled, kind, run_device(data, shuffled, kind, order=perm))


def test_mixed_algorithms_in_table_order(built):
    """MD5, SHA-1 and SHA-256 heads in arbitrary table order, through a d_order permutation: every digest is right, and every MD5
    result is that of the same batch without the SHA units"""
    rng = np.random.default_rng(77)
    n = 150
    data = rng.integers(0, 256, 8192, dtype=np.uint8)
    kinds = [int(k) for k in rng.choice([M.KIND_MD5, M.KIND_SHA1, M.KIND_SHA256], n)]
    ranges = [(int(rng.integers(0, 8192 - ln)), ln) for ln in (int(x) for x in rng.integers(0, 1500, n))]
    units, heads = M.digest_units(ranges, kinds)
    got = run_device(data, ranges, kinds, order=rng.permutation(len(units)).astype(np.uint32))
    check(data, ranges, kinds, got)
    md5_ranges = [r for r, k in zip(ranges, kinds) if k == M.KIND_MD5]
    alone = G5.run_device(data, md5_ranges)
    assert alone == [d for d, k in zip(got, kinds) if k == M.KIND_MD5] and len(alone) > 30


@pytest.mark.parametrize("kind", SHA)
def test_arena_edges_and_guards(built, kind):
    """one range ends on the arena's last byte, one begins on its first, one is the whole arena, one is empty at its end -- the arena
    is exactly out_bytes long inside an allocation of 0xA5 whose other bytes are checked (run_device_raw)"""
    for n in (1, 61, 64, 1000, 1027):
        data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        ranges = [(n - min(n, 37), min(n, 37)), (0, min(n, 70)), (0, n), (n, 0), (n - 1, 1), (0, 1)]
        check(data, ranges, kind, run_device(data, ranges, kind))


def test_device_side_argument_errors(built):
    """the device-resident entry cannot refuse a table it has not read: MSPACK_ERR_ARGS in the unit's result instead, nothing read.
    A head that is the table's last unit, a head followed by a unit of another kind, a head followed by a tail that names bytes, a tail
    without a head, a range that leaves out_bytes -- beside good units, whose digests are right"""
    data = np.random.default_rng(5).integers(0, 256, 1000, dtype=np.uint8)
    rows = [(M.KIND_SHA256, 0, 100), (M.KIND_DIGEST_MORE, 0, 0),           # 0, 1: good
            (M.KIND_DIGEST_MORE, 0, 0),                                   # 2: behind a tail: no head in front of it
            (M.KIND_SHA1, 10, 50), (M.KIND_MD5, 10, 50),                  # 3: followed by another kind; 4: good
            (M.KIND_DIGEST_MORE, 0, 0),                                   # 5: behind an MD5 unit
            (M.KIND_SHA1, 990, 11), (M.KIND_DIGEST_MORE, 0, 0),           # 6: leaves out_bytes; 7: its tail
            (M.KIND_SHA256, 1001, 0), (M.KIND_DIGEST_MORE, 0, 0),         # 8: begins beyond out_bytes
            (M.KIND_SHA256, 5, 5), (M.KIND_DIGEST_MORE, 0, 4),            # 10: its tail names bytes
            (M.KIND_SHA1, 900, 100), (M.KIND_DIGEST_MORE, 0, 0),          # 12, 13: good, ends on the arena's last byte
            (M.KIND_SHA256, 0, 10)]                                       # 14: the table's last unit
    units = np.zeros(len(rows), dtype=M.UNIT_DTYPE)
    units["kind"] = [r[0] for r in rows]; units["out_off"] = [r[1] for r in rows]; units["out_len"] = [r[2] for r in rows]
    res = run_device_raw(data, units, M.MASK_MD5 | M.MASK_SHA1 | M.MASK_SHA256)
    raw = res.view(np.uint8).reshape(len(rows), -1)
    assert [int(e) for e in res["err"][[0, 1, 4, 12, 13]]] == [0] * 5
    assert [int(e) for e in res["err"][[2, 3, 5, 6, 8, 10, 14]]] == [M.ERR_ARGS] * 7, res["err"]
    for i in (2, 3, 5, 6, 8, 10, 14):
        assert res["flags"][i] == 0 and (raw[i, 8:] == 0).all(), res[i]
    assert (raw[[7, 9]] == 0).all()                                        # the tail of a head whose range is refused: all 0
    assert (raw[11] == 0x77).all()                                         # a tail that is not one: nobody's to write
    got = M.result_wide_digests(res, units)
    heads = [i for i, r in enumerate(rows) if r[0] in M.DIGEST_BYTES]
    for i in (0, 4, 12):
        k, o, n = rows[i]
        assert got[heads.index(i)] == HASH[k](data[o:o + n].tobytes()).digest(), i


# ---- behind the decoders --------------------------------------------------------------------------------------------------

def three_kinds(ranges):
    """every range three times: MD5, SHA-1, SHA-256, interleaved in the table"""
    rr, kk = [], []
    for i, r in enumerate(ranges):
        for k in (M.KIND_SHA256, M.KIND_MD5, M.KIND_SHA1)[i % 3:] + (M.KIND_SHA256, M.KIND_MD5, M.KIND_SHA1)[:i % 3]:
            rr.append(r); kk.append(k)
    return rr, kk


def decode_with_digests(units, arena, out_bytes, ranges, kinds, n_devices=1, refs=None):
    n = len(units)
    dg, _heads = M.digest_units(ranges, kinds)
    both = np.concatenate([np.ascontiguousarray(units, dtype=M.UNIT_DTYPE), dg])
    out, res = M.decode_batch(both, arena, out_bytes, n_devices=n_devices, refs=refs)
    assert (res["err"][n:] == 0).all() and (res["flags"][n:] == 0).all(), res[n:]
    check_tails(dg, res[n:])
    return out, res[:n], M.result_wide_digests(res[n:], dg)


def check_mixed(units, out, res, digests, ranges, kinds, plain_out, plain_res):
    """the digests are those of the bytes the call left in the arena; every decoding unit's result and bytes are those of the batch
    without digest units"""
    assert np.array_equal(res, plain_res)
    for i in range(len(units)):
        o, n = int(units["out_off"][i]), int(plain_res["out_len"][i])
        assert np.array_equal(out[o:o + n], plain_out[o:o + n]), i
    check(out, ranges, kinds, digests)


def test_behind_the_decoders(built):
    """one mixed batch through mspack_hip_decode_batch: units of all six decoding kinds and one damaged LZX stream, and per range an
    MD5, a SHA-1 and a SHA-256 unit: the passes see what every decoder stored, also what the damaged stream left"""
    units, arena, out_bytes, refs, ranges = G5.mixed_batch()
    assert sorted(set(int(k) for k in units["kind"])) == [1, 2, 3, 4, 5, 6]
    plain_out, plain_res = M.decode_batch(units, arena, out_bytes, refs=refs)
    assert plain_res["err"][-1] != 0 and (plain_res["err"][:-1] == 0).all()
    rr, kk = three_kinds(ranges)
    out, res, digests = decode_with_digests(units, arena, out_bytes, rr, kk, refs=refs)
    check_mixed(units, out, res, digests, rr, kk, plain_out, plain_res)


def test_device_resident_entry_behind_the_decoders(built):
    """mspack_hip_decode_batch_device with decoding units of all six kinds (one stream damaged) AND digest units of the three
    algorithms in one table: with each mask bit that algorithm's digests are right and the other algorithms' results (tails
    included) untouched; without any no digest unit's result is touched; beside the CRC pass both digests are of the same bytes"""
    units, arena, out_bytes, refs, ranges = G5.mixed_batch(seed=21)
    nd = len(units)
    rr, kk = three_kinds(ranges[:12])
    dg, heads = M.digest_units(rr, kk)
    both = np.concatenate([units, dg])
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

    def owner(i):                                                           # the algorithm a digest unit's result belongs to
        return int(dg["kind"][i]) if dg["kind"][i] != M.KIND_DIGEST_MORE else int(dg["kind"][i - 1])

    out0, res0 = call(codecs)
    assert res0["err"][nd - 1] != 0 and (res0["err"][:nd - 1] == 0).all()
    assert (res0[nd:].view(np.uint8) == 0x77).all()                         # no digest bit: no digest unit's result is touched
    for kind in (M.KIND_SHA1, M.KIND_SHA256):
        out1, res1 = call(codecs | MASK[kind])
        assert np.array_equal(res1[:nd], res0[:nd])
        for i in range(nd):
            o, n = int(units["out_off"][i]), int(res0["out_len"][i])
            assert np.array_equal(out1[o:o + n], out0[o:o + n]), i
        raw = res1[nd:].view(np.uint8).reshape(len(dg), -1)
        for i in range(len(dg)):
            if owner(i) != kind:
                assert (raw[i] == 0x77).all(), (kind, i)                    # without its bit: no pass, head and tail untouched
            else:
                assert res1["err"][nd + i] == 0 and res1["flags"][nd + i] == 0
        mine = [j for j, k in enumerate(kk) if k == kind]
        sub = M.result_wide_digests(res1[nd:], dg)
        check(out1, [rr[j] for j in mine], kind, [sub[j] for j in mine])
    # ... all three and the CRC pass: every digest of the same bytes
    out2, res2 = call(codecs | M.MASK_MD5 | M.MASK_SHA1 | M.MASK_SHA256 | M.MASK_CRC32, flags=M.UF_CRC32)
    check_tails(dg, res2[nd:])
    check(out2, rr, kk, M.result_wide_digests(res2[nd:], dg))
    T.check_digests(units, out2, res2[:nd])
    for f in ("err", "flags", "out_len", "good_len", "in_next"):
        assert np.array_equal(res2[f][:nd], res0[f][:nd]), f
    for b in (scratch, d_units, d_in):
        b.free()


def test_to_device(built):
    """host input, device output: digests of bytes that never came back -- compared after a copy of the test's own"""
    units, arena, out_bytes, refs, ranges = G5.mixed_batch(seed=8)
    d_out = DevBuf(out_bytes + 64)
    for u, r in zip(units, refs):
        if len(r):
            dev_write(d_out, int(u["out_off"]) - len(r), np.frombuffer(r, dtype=np.uint8))
    rr, kk = three_kinds(ranges)
    dg, _h = M.digest_units(rr, kk)
    both = np.concatenate([units, dg])
    res = np.zeros(len(both), dtype=M.RESULT_DTYPE)
    rc = M.lib().mspack_hip_decode_batch_to_device(both.ctypes.data, len(both), arena.ctypes.data, arena.size, d_out.ptr, out_bytes + 64,
                                                   res.ctypes.data)
    assert rc == 0, M.lib().mspack_hip_last_error()
    assert (res["err"][len(units):] == 0).all() and (res["flags"][len(units):] == 0).all()
    check_tails(dg, res[len(units):])
    check(d_out.to_host(), rr, kk, M.result_wide_digests(res[len(units):], dg))
    d_out.free()


WORKER = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import libmspack_amd as M
import test_gpu_md5 as G5
import test_gpu_sha as S
mode = sys.argv[1]
units, arena, out_bytes, refs, ranges = G5.mixed_batch(seed=12, n_each=3)
rr, kk = S.three_kinds(ranges)
if mode == "jobs":
    assert os.environ["MSPACK_PY_VIA_JOBS"] == "1"
    # waiting on a TAIL first: it returns when the batch is through, with head and tail written
    dg, heads = M.digest_units(rr, kk)
    both = np.concatenate([units, dg])
    out = np.zeros(out_bytes, dtype=np.uint8)
    for u, r in zip(units, refs):
        if len(r):
            out[int(u["out_off"]) - len(r):int(u["out_off"])] = np.frombuffer(r, dtype=np.uint8)
    res = np.zeros(len(both), dtype=M.RESULT_DTYPE); res["err"] = 0x7777
    L = M.lib()
    job = L.mspack_hip_decode_batch_begin(both.ctypes.data, len(both), arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data)
    assert job
    tail = len(units) + int(np.flatnonzero(dg["kind"] == M.KIND_DIGEST_MORE)[-1])
    assert L.mspack_hip_job_wait_unit(job, tail) == 0
    assert (res["err"] != 0x7777).all()
    first = M.result_wide_digests(res[len(units):], dg)
    assert L.mspack_hip_job_end(job) == 0
    S.check(out, rr, kk, first)
    n_dev = 1
else:
    assert os.environ["MSPACK_HIP_FORCE_SHARDS"] in ("2", "3")
    n_dev = 2
plain_out, plain_res = M.decode_batch(units, arena, out_bytes, refs=refs, n_devices=n_dev)
out, res, digests = S.decode_with_digests(units, arena, out_bytes, rr, kk, n_devices=n_dev, refs=refs)
S.check_mixed(units, out, res, digests, rr, kk, plain_out, plain_res)
# a batch of equal units: the even cuts fall behind unit n / 2 (n / 3, 2 n / 3) -- with a digest range across each of them
units, comp, out_bytes, plain, ranges = G5.chunked_batch()
n, ub = len(units), 65536
ranges = ranges[::9] + ranges[-3:] + [(k * ub - 5000, 10000) for k in (n // 2, n // 3, 2 * n // 3, n // 2 + 1, n // 3 + 1, 2 * n // 3 + 1)]
rr, kk = S.three_kinds(ranges)
out, res, digests = S.decode_with_digests(units, comp, out_bytes, rr, kk, n_devices=n_dev)
assert (res["err"] == 0).all() and np.array_equal(out[:plain.size], plain)
S.check(plain, rr, kk, digests)
print("SHA_WORKER_OK")
'''


@pytest.mark.parametrize("mode,env", [("shards", {"MSPACK_HIP_FORCE_SHARDS": "2"}), ("shards", {"MSPACK_HIP_FORCE_SHARDS": "3"}),
                                      ("jobs", {"MSPACK_PY_VIA_JOBS": "1", "MSPACK_HIP_TRACE": "1"})])
def test_chunked_sharded_and_job_entry_points(built, mode, env, tmp_path):
    """a batch the planner cuts into chunks (the library's trace says so) with ranges across the cuts, one of them over 300 units;
    mspack_hip_decode_batch_multi cut into two and three shards with ranges where the even cuts would fall; _begin / _wait_unit /
    _end waiting on a tail first -- in a fresh process so that the environment switch is seen"""
    script = tmp_path / "w.py"
    script.write_text(WORKER % (ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script), mode], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0 and b"SHA_WORKER_OK" in p.stdout, p.stdout.decode()[-3000:]
    if mode == "jobs":
        cuts = [int(m.group(2)) for m in re.finditer(rb"(\d+) units in (\d+) chunks", p.stdout) if int(m.group(1)) > 640]
        assert cuts and max(cuts) >= 2, p.stdout.decode()[-3000:]


def test_rejections(built):
    """the host entry points refuse a bad table with the message, before anything is touched"""
    arena = np.zeros(256, dtype=np.uint8)

    def table(rows):
        u = np.zeros(len(rows), dtype=M.UNIT_DTYPE)
        u["kind"] = [r[0] for r in rows]; u["out_off"] = [r[1] for r in rows]; u["out_len"] = [r[2] for r in rows]
        return u
    more = (M.KIND_DIGEST_MORE, 0, 0)
    cases = [
        (table([(M.KIND_MD5, 0, 10), (M.KIND_SHA1, 0, 10)]), "unit 1: a wide digest unit is the table's last unit"),
        (table([(M.KIND_SHA256, 0, 10), (M.KIND_MD5, 0, 10), more]), "unit 0: a wide digest unit must be followed by an MSPACK_HIP_KIND_DIGEST_MORE unit"),
        (table([(M.KIND_MD5, 0, 10), more]), "unit 1: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it"),
        (table([(M.KIND_SHA1, 0, 10), (M.KIND_DIGEST_MORE, 0, 1)]), "unit 1: an MSPACK_HIP_KIND_DIGEST_MORE unit names no bytes"),
        (table([(M.KIND_SHA256, 60, 5), more]), "unit 0: a digest unit's range leaves the output arena"),
    ]
    u = table([(M.KIND_SHA1, 0, 10), more]); u["flags"][0] = M.UF_CRC32
    cases.append((u, "unit 0: a digest unit decodes nothing to take a CRC-32 of"))
    u = table([(M.KIND_SHA256, 0, 10), more]); u["in_len"][0] = 1
    cases.append((u, "unit 0: a digest unit reads no input"))
    u = table([(M.KIND_MD5, 0, 10), more]); u["kind"][1] = 9
    cases.append((u, "unit 1: unknown kind 9"))
    for u, msg in cases:
        out = np.full(64, 0x5A, dtype=np.uint8)
        res = np.zeros(len(u), dtype=M.RESULT_DTYPE); res["err"] = 0x7777; res["in_next"] = 0x1234
        before = res.copy()
        for entry in ("mspack_hip_decode_batch", "multi"):
            if entry == "multi":
                rc = M.lib().mspack_hip_decode_batch_multi(u.ctypes.data, len(u), arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data, 1)
            else:
                rc = M.lib().mspack_hip_decode_batch(u.ctypes.data, len(u), arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data)
            assert rc != 0 and msg in M.lib().mspack_hip_last_error().decode(), (msg, M.lib().mspack_hip_last_error())
            assert np.array_equal(res, before) and (out == 0x5A).all()


def test_cabinet_driver_takes_the_digests_on_the_device(built):
    """one cabinet of 256 MSZIP folders, one file of 2 KiB each, MSCABD_PARAM_HIP_DIGESTS = 7: every digest of the three algorithms is
    right and mspack_cabd_digest_counts says they came from the device; MSCABD_PARAM_HIP_MD5 = 0 behind it takes bit 1 away again"""
    from libmspack_amd import api, apibench as A
    n, ub = 256, 2048
    image, plain = A.build_config2_cab(M, n, ub)
    algs = ((api.MSPACK_DIGEST_MD5, hashlib.md5), (api.MSPACK_DIGEST_SHA1, hashlib.sha1), (api.MSPACK_DIGEST_SHA256, hashlib.sha256))
    for alg, _h in algs:
        api.cabd_digest_counts(alg, reset=True)
    with api.Cab(bytes(image), mem=True) as c:
        assert len(c._files) == n
        assert c.set_param(api.MSCABD_PARAM_HIP_DIGESTS, 7) == 0 and c.get_param(api.MSCABD_PARAM_HIP_MD5) == (0, 1)
        for i in range(n):
            for alg, h in algs:
                err, d = c.digest(i, alg)
                assert err == 0 and d == h(plain[i * ub:(i + 1) * ub].tobytes()).digest(), (i, alg)
        assert not c.mem.outputs
    for alg, _h in algs:
        assert api.cabd_digest_counts(alg) == (n, 0), alg
    with api.Cab(bytes(image), mem=True) as c:
        assert c.set_param(api.MSCABD_PARAM_HIP_DIGESTS, 7) == 0 and c.set_param(api.MSCABD_PARAM_HIP_MD5, 0) == 0
        assert c.get_param(api.MSCABD_PARAM_HIP_DIGESTS) == (0, 6)
        api.cabd_digest_counts(api.MSPACK_DIGEST_MD5, reset=True); api.cabd_digest_counts(api.MSPACK_DIGEST_SHA1, reset=True)
        assert c.digest(3, api.MSPACK_DIGEST_MD5) == (0, hashlib.md5(plain[3 * ub:4 * ub].tobytes()).digest())
        assert c.digest(3, api.MSPACK_DIGEST_SHA1) == (0, hashlib.sha1(plain[3 * ub:4 * ub].tobytes()).digest())
        assert api.cabd_digest_counts(api.MSPACK_DIGEST_MD5) == (0, 1) and api.cabd_digest_counts(api.MSPACK_DIGEST_SHA1) == (1, 0)
