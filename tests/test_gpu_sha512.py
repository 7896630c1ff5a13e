"""MSPACK_HIP_KIND_SHA384 / _SHA512 (include/mspack_hip.h): the digest units with 64-bit words -- the SHA-384 / SHA-512 of a byte range
of the output arena, one lane per range, one pass for both algorithms behind everything else of the batch; bytes 16 k .. of a digest
come back in the result of the k-th MSPACK_HIP_KIND_DIGEST_MORE unit behind the head (two for SHA-384, three for SHA-512).  Everything
goes through the C ABI; the reference for a digest is hashlib over the bytes that lie in the range, the reference for everything else
is the same batch without the new units.

tests/test_sha512_emu.py runs the first four groups of this file (lengths and alignments, the FIPS strings, 65 ranges in one table,
the arena's edges inside guard bytes) on the wavefront emulator."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import libmspack_amd as M
import test_gpu_md5 as G5
import test_gpu_sha as S
from test_gpu_hostpath import DevBuf
from test_gpu_md5 import dev_write

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH = {M.KIND_MD5: hashlib.md5, M.KIND_SHA1: hashlib.sha1, M.KIND_SHA256: hashlib.sha256, M.KIND_SHA384: hashlib.sha384,
        M.KIND_SHA512: hashlib.sha512}
MASK = {M.KIND_MD5: M.MASK_MD5, M.KIND_SHA1: M.MASK_SHA1, M.KIND_SHA256: M.MASK_SHA256, M.KIND_SHA384: M.MASK_SHA384,
        M.KIND_SHA512: M.MASK_SHA512}
TAILS = {M.KIND_MD5: 0, M.KIND_SHA1: 1, M.KIND_SHA256: 1, M.KIND_SHA384: 2, M.KIND_SHA512: 3}
NEW = [M.KIND_SHA384, M.KIND_SHA512]
ALL5 = (M.KIND_SHA512, M.KIND_MD5, M.KIND_SHA384, M.KIND_SHA1, M.KIND_SHA256)

# FIPS 180-4's example messages: empty, "abc", the 896-bit one
FIPS = [b"", b"abc", b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu"]
FIPS_SHA384 = ["38b060a751ac96384cd9327eb1b1e36a21fdb71114be07434c0cc7bf63f6e1da274edebfe76f65fbd51ad2f14898b95b",
               "cb00753f45a35e8bb5a03d699ac65007272c32ab0eded1631a8b605a43ff5bed8086072ba1e7cc2358baeca134c825a7",
               "09330c33f71147e83d192fc782cd1b4753111b173b3b05d22fa08086e3b0f712fcc7c71a557e2db966c3e9fa91746039"]
FIPS_SHA512 = ["cf83e1357eefb8bdf1542850d66d8007d620e4050b5715dc83f4a921d36ce9ce47d0d13c5d85f2b0ff8318d2877eec2f63b931bd47417a81a538327af927da3e",
               "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
               "8e959b75dae313da8cf4f72814fc143f8f7779c6eb9f7fa17299aeadb6889018501d289e4900f7e4331b99dec4b5433ac7d329eeb6dd26545e96e55b874be909"]


def check(data, ranges, kinds, got):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    assert len(got) == len(ranges)
    for (o, n), k, d in zip(ranges, S.kinds_of(kinds, len(ranges)), got):
        assert d == HASH[k](data[o:o + n].tobytes()).digest(), (k, o, n, d.hex())


def owner_of(units, i):
    """the index of the head a digest unit's result belongs to (its own, or for a tail the first unit in front of it that is none)"""
    while units["kind"][i] == M.KIND_DIGEST_MORE:
        i -= 1
    return i


def check_tails(units, res):
    """a tail's result: err 0, flags 0, the words the digest does not use 0 (SHA-1: everything behind out_len); every head has as many
    tails behind it as its digest needs"""
    for i in np.flatnonzero(units["kind"] != M.KIND_DIGEST_MORE):
        nt = TAILS[int(units["kind"][i])]
        assert (units["kind"][i + 1:i + 1 + nt] == M.KIND_DIGEST_MORE).all() and len(units) >= i + 1 + nt
        assert i + 1 + nt == len(units) or units["kind"][i + 1 + nt] != M.KIND_DIGEST_MORE
    for i in np.flatnonzero(units["kind"] == M.KIND_DIGEST_MORE):
        assert res["err"][i] == 0 and res["flags"][i] == 0, res[i]
        if units["kind"][i - 1] == M.KIND_SHA1:
            assert res["in_used"][i] == 0 and res["good_len"][i] == 0 and res["in_next"][i] == 0, res[i]


def run_device(data, ranges, kinds, order=None):
    """digest units of `kinds` over the ranges through the device-resident entry -> the digests in range order (the arena is exactly
    len(data) bytes inside guard bytes that are checked: test_gpu_sha.run_device_raw)"""
    kinds = S.kinds_of(kinds, len(ranges))
    units, _heads = M.digest_units(ranges, kinds)
    mask = 0
    for k in set(kinds):
        mask |= MASK[k]
    res = S.run_device_raw(data, units, mask, order)
    assert (res["err"] == 0).all() and (res["flags"] == 0).all(), res
    check_tails(units, res)
    return M.result_wide_digests(res, units)


# the lengths at which the pad changes its path (111 / 112 / 113: one final block or two; 127 / 128 / 129, 239 / 240, 255 / 256 / 257:
# the block edges), and one long enough for 781 blocks
LENGTHS = [0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 255, 256, 257, 1000, 100003]
ALIGNS = [0, 1, 3, 4, 8, 15]


def lengths_layout():
    ranges, pos = [], 0
    for n in LENGTHS:
        for r in ALIGNS:
            pos = (pos + 63) & ~63
            ranges.append((pos + r, n))
            pos += r + n
    return ranges, pos


@pytest.mark.parametrize("kind", NEW)
def test_lengths_and_alignments(built, kind):
    """every length of LENGTHS at out_off mod 16 in {0, 1, 3, 4, 8, 15}: the row, dword and funnel-shift loaders' first and last words"""
    assert M.features() & (M.FEAT_SHA384 if kind == M.KIND_SHA384 else M.FEAT_SHA512)
    ranges, total = lengths_layout()
    assert sorted(set(o % 16 for o, _n in ranges)) == ALIGNS and len(ranges) == len(ALIGNS) * len(LENGTHS)
    data = np.random.default_rng(3840).integers(0, 256, total, dtype=np.uint8)
    check(data, ranges, kind, run_device(data, ranges, kind))


def test_fips_strings(built):
    """FIPS 180-4's example messages back to back in one arena (so at different alignments), both algorithms in one table and one launch"""
    data = np.frombuffer(b"".join(FIPS), dtype=np.uint8)
    ranges, pos = [], 0
    for s in FIPS:
        ranges.append((pos, len(s))); pos += len(s)
    got = run_device(data, ranges * 2, [M.KIND_SHA384] * 3 + [M.KIND_SHA512] * 3)
    assert [d.hex() for d in got] == FIPS_SHA384 + FIPS_SHA512
    assert [len(d) for d in got] == [48] * 3 + [64] * 3


def test_65_ranges_of_different_lengths(built):
    """65 heads of 65 different lengths, the two algorithms alternating, shuffled and descending: two waves, the second with one live
    lane, loops that end at a different count in every lane (finished lanes masked); again through a d_order permutation of the
    whole table, tails included"""
    n_units = 65
    rng = np.random.default_rng(512)
    lens = [(11 * i + 5) % 1499 + (i == 0) * 2000 for i in range(n_units)]
    assert len(set(lens)) == n_units
    data = rng.integers(0, 256, 4096, dtype=np.uint8)
    shuffled = [(int(rng.integers(0, 4096 - n)), n) for n in (lens[k] for k in rng.permutation(n_units))]
    kinds = [NEW[i % 2] for i in range(n_units)]
    descending = sorted(shuffled, key=lambda r: -r[1])
    for ranges in (shuffled, descending):
        check(data, ranges, kinds, run_device(data, ranges, kinds))
    units, _h = M.digest_units(shuffled, kinds)
    perm = rng.permutation(len(units)).astype(np.uint32)
    check(data, shuffled, kinds, run_device(data, shuffled, kinds, order=perm))


@pytest.mark.parametrize("kind", NEW)
def test_arena_edges_and_guards(built, kind):
    """one range ends on the arena's last byte, one begins on its first, one is the whole arena, one is empty at its end -- the arena
    is exactly out_bytes long inside an allocation of 0xA5 whose other bytes are checked (run_device_raw)"""
    for n in (1, 125, 128, 1000, 1027):
        data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        ranges = [(n - min(n, 37), min(n, 37)), (0, min(n, 130)), (0, n), (n, 0), (n - 1, 1), (0, 1)]
        check(data, ranges, kind, run_device(data, ranges, kind))


def test_all_digest_kinds_in_table_order(built):
    """MD5, SHA-1, SHA-256, SHA-384 and SHA-512 heads in arbitrary table order, through a shuffled d_order: every digest is right, and
    the results of the three older kinds are those of the same batch without the new units"""
    rng = np.random.default_rng(384)
    n = 200
    data = rng.integers(0, 256, 8192, dtype=np.uint8)
    kinds = [int(k) for k in rng.choice(list(ALL5), n)]
    ranges = [(int(rng.integers(0, 8192 - ln)), ln) for ln in (int(x) for x in rng.integers(0, 1500, n))]
    units, _heads = M.digest_units(ranges, kinds)
    got = run_device(data, ranges, kinds, order=rng.permutation(len(units)).astype(np.uint32))
    check(data, ranges, kinds, got)
    old = [j for j, k in enumerate(kinds) if k not in NEW]
    alone = S.run_device(data, [ranges[j] for j in old], [kinds[j] for j in old])
    assert alone == [got[j] for j in old] and len(old) > 60 and n - len(old) > 40


def test_device_side_argument_errors(built):
    """the device-resident entry cannot refuse a table it has not read: MSPACK_ERR_ARGS in the unit's result instead, nothing read.
    Too few tails (SHA-384 with 1, SHA-512 with 2, a head that ends the table), a tail that names bytes, more tails than the head
    needs (SHA-256 with 2, SHA-384 with 3, SHA-512 with 4), a lone tail, ranges that leave out_bytes -- beside good units, whose
    digests are right"""
    data = np.random.default_rng(6).integers(0, 256, 1000, dtype=np.uint8)
    more = (M.KIND_DIGEST_MORE, 0, 0)
    rows = [(M.KIND_SHA512, 0, 100), more, more, more,                     # 0 .. 3: good
            more,                                                          # 4: a fourth tail
            (M.KIND_SHA384, 10, 50), more, (M.KIND_MD5, 10, 50),           # 5: one tail only; 6: its tail (nobody's to write); 7: good
            more,                                                          # 8: behind an MD5 unit
            (M.KIND_SHA512, 990, 11), more, more, more,                    # 9: leaves out_bytes; 10 .. 12: its tails: all 0
            (M.KIND_SHA384, 1001, 0), more, more,                          # 13: begins beyond out_bytes; 14, 15: all 0
            (M.KIND_SHA512, 5, 5), more, (M.KIND_DIGEST_MORE, 0, 4), more,  # 16: its second tail names bytes
            (M.KIND_SHA384, 900, 100), more, more,                         # 20 .. 22: good, ends on the arena's last byte
            more,                                                          # 23: a third tail
            (M.KIND_SHA256, 3, 7), more, more,                             # 24, 25: good (unchanged); 26: a second tail
            (M.KIND_SHA512, 0, 10), more, more,                            # 27: two tails, then the table's end
            ]
    units = np.zeros(len(rows), dtype=M.UNIT_DTYPE)
    units["kind"] = [r[0] for r in rows]; units["out_off"] = [r[1] for r in rows]; units["out_len"] = [r[2] for r in rows]
    res = S.run_device_raw(data, units, M.MASK_MD5 | M.MASK_SHA256 | M.MASK_SHA384 | M.MASK_SHA512)
    raw = res.view(np.uint8).reshape(len(rows), -1)
    good = [0, 1, 2, 3, 7, 20, 21, 22, 24, 25]
    bad = [4, 5, 8, 9, 13, 16, 23, 26, 27]
    assert [int(e) for e in res["err"][good]] == [0] * len(good), res["err"]
    assert [int(e) for e in res["err"][bad]] == [M.ERR_ARGS] * len(bad), res["err"]
    for i in bad:
        assert res["flags"][i] == 0 and (raw[i, 8:] == 0).all(), res[i]
    assert (raw[[10, 11, 12, 14, 15]] == 0).all()                          # the tails of a head whose range is refused: all 0
    assert (raw[[6, 17, 18, 19, 28, 29]] == 0x77).all()                    # the tails of a head that lacks some: nobody's to write
    for i, nb in ((0, 64), (7, 16), (20, 48), (24, 32)):
        k, o, n = rows[i]
        d = b"".join(raw[i + t, 8:24].tobytes() for t in range((nb + 15) // 16))[:nb]
        assert d == HASH[k](data[o:o + n].tobytes()).digest(), i


# ---- behind the decoders --------------------------------------------------------------------------------------------------

def five_kinds(ranges):
    """every range five times -- all digest kinds --, interleaved in the table in a rotating order"""
    rr, kk = [], []
    for i, r in enumerate(ranges):
        for k in ALL5[i % 5:] + ALL5[:i % 5]:
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
    """one mixed batch through mspack_hip_decode_batch: units of all six decoding kinds (LZX and MSZIP among them) and one damaged LZX
    stream, and per range a unit of every digest kind: the passes see what every decoder stored, also what the damaged stream left
    -- the digest is of whatever lies there, compared with the returned bytes"""
    units, arena, out_bytes, refs, ranges = G5.mixed_batch()
    assert sorted(set(int(k) for k in units["kind"])) == [1, 2, 3, 4, 5, 6]
    plain_out, plain_res = M.decode_batch(units, arena, out_bytes, refs=refs)
    assert plain_res["err"][-1] != 0 and (plain_res["err"][:-1] == 0).all()
    rr, kk = five_kinds(ranges)
    out, res, digests = decode_with_digests(units, arena, out_bytes, rr, kk, refs=refs)
    check_mixed(units, out, res, digests, rr, kk, plain_out, plain_res)


def test_device_resident_entry_with_and_without_the_bits(built):
    """mspack_hip_decode_batch_device with decoding units of all six kinds (one stream damaged) AND digest units of the five kinds in
    one table.  Without bits 24 and 25 no new unit's result (tails included) is touched, whatever other digest bits are set; with
    one of them that algorithm's digests are right and the other's untouched; with both and every other pass every digest is of
    the same bytes"""
    units, arena, out_bytes, refs, ranges = G5.mixed_batch(seed=21)
    nd = len(units)
    rr, kk = five_kinds(ranges[:10])
    dg, _heads = M.digest_units(rr, kk)
    both = np.concatenate([units, dg])
    fr = M.frames_of(both)
    both["frame_base"] = np.concatenate([[0], np.cumsum(fr)[:-1]])
    n_frames = int(fr.sum())
    L = M.lib()
    scratch = DevBuf(max(L.mspack_hip_frame_scratch_bytes(n_frames), 16))
    d_units, d_in = DevBuf(both.nbytes), DevBuf(arena.size + 64)
    dev_write(d_in, 0, arena)
    dev_write(d_units, 0, both.view(np.uint8))
    codecs = 0xFE

    def call(mask):
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

    owner = [int(dg["kind"][owner_of(dg, i)]) for i in range(len(dg))]
    out0, res0 = call(codecs)
    assert res0["err"][nd - 1] != 0 and (res0["err"][:nd - 1] == 0).all()
    assert (res0[nd:].view(np.uint8) == 0x77).all()                         # no digest bit: no digest unit's result is touched
    for mask_kinds in ([M.KIND_MD5, M.KIND_SHA1, M.KIND_SHA256], [M.KIND_SHA384], [M.KIND_SHA512], NEW):
        mask = codecs
        for k in mask_kinds:
            mask |= MASK[k]
        out1, res1 = call(mask)
        assert np.array_equal(res1[:nd], res0[:nd])
        for i in range(nd):
            o, n = int(units["out_off"][i]), int(res0["out_len"][i])
            assert np.array_equal(out1[o:o + n], out0[o:o + n]), i
        raw = res1[nd:].view(np.uint8).reshape(len(dg), -1)
        for i in range(len(dg)):
            if owner[i] not in mask_kinds:
                assert (raw[i] == 0x77).all(), (mask_kinds, i)              # without its bit: head and tails untouched
            else:
                assert res1["err"][nd + i] == 0 and res1["flags"][nd + i] == 0
        mine = [j for j, k in enumerate(kk) if k in mask_kinds]
        sub = M.result_wide_digests(res1[nd:], dg)
        check(out1, [rr[j] for j in mine], [kk[j] for j in mine], [sub[j] for j in mine])
    out2, res2 = call(codecs | M.MASK_MD5 | M.MASK_SHA1 | M.MASK_SHA256 | M.MASK_SHA384 | M.MASK_SHA512)
    check_tails(dg, res2[nd:])
    check(out2, rr, kk, M.result_wide_digests(res2[nd:], dg))
    assert np.array_equal(res2[:nd], res0[:nd])
    for b in (scratch, d_units, d_in):
        b.free()


def test_to_device(built):
    """host input, device output: digests of bytes that never came back -- compared after a copy of the test's own"""
    units, arena, out_bytes, refs, ranges = G5.mixed_batch(seed=8)
    d_out = DevBuf(out_bytes + 64)
    for u, r in zip(units, refs):
        if len(r):
            dev_write(d_out, int(u["out_off"]) - len(r), np.frombuffer(r, dtype=np.uint8))
    rr, kk = five_kinds(ranges)
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
import test_gpu_sha512 as S
mode = sys.argv[1]
units, arena, out_bytes, refs, ranges = G5.mixed_batch(seed=12, n_each=3)
rr, kk = S.five_kinds(ranges)
if mode == "jobs":
    assert os.environ["MSPACK_PY_VIA_JOBS"] == "1"
    # waiting on a SHA-512 head's LAST tail first: it returns when the batch is through, with the head and all tails written
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
    h512 = int(np.flatnonzero(dg["kind"] == M.KIND_SHA512)[-1])
    assert (dg["kind"][h512 + 1:h512 + 4] == M.KIND_DIGEST_MORE).all()
    assert L.mspack_hip_job_wait_unit(job, len(units) + h512 + 3) == 0
    assert (res["err"] != 0x7777).all()
    first = M.result_wide_digests(res[len(units):], dg)
    assert L.mspack_hip_job_wait_unit(job, len(units) + int(np.flatnonzero(dg["kind"] == M.KIND_SHA384)[0])) == 0
    assert L.mspack_hip_job_end(job) == 0
    S.check(out, rr, kk, first)
    n_dev = 1
else:
    assert os.environ["MSPACK_HIP_FORCE_SHARDS"] == "2"
    n_dev = 2
plain_out, plain_res = M.decode_batch(units, arena, out_bytes, refs=refs, n_devices=n_dev)
out, res, digests = S.decode_with_digests(units, arena, out_bytes, rr, kk, n_devices=n_dev, refs=refs)
S.check_mixed(units, out, res, digests, rr, kk, plain_out, plain_res)
# a batch of equal units: the even cut falls behind unit n / 2 -- with a digest range across it and across the chunks' cuts
units, comp, out_bytes, plain, ranges = G5.chunked_batch()
n, ub = len(units), 65536
ranges = ranges[::9] + ranges[-3:-1] + [(k * ub - 5000, 10000) for k in (n // 2, n // 4, n // 2 + 1)]
rr = ranges * 2
kk = [M.KIND_SHA384] * len(ranges) + [M.KIND_SHA512] * len(ranges)
out, res, digests = S.decode_with_digests(units, comp, out_bytes, rr, kk, n_devices=n_dev)
assert (res["err"] == 0).all() and np.array_equal(out[:plain.size], plain)
S.check(plain, rr, kk, digests)
print("SHA512_WORKER_OK")
'''


@pytest.mark.parametrize("mode,env", [("shards", {"MSPACK_HIP_FORCE_SHARDS": "2"}),
                                      ("jobs", {"MSPACK_PY_VIA_JOBS": "1", "MSPACK_HIP_TRACE": "1"})])
def test_chunked_sharded_and_job_entry_points(built, mode, env, tmp_path):
    """a batch the planner cuts into chunks (the library's trace says so) with ranges across the cuts; mspack_hip_decode_batch_multi cut
    into two forced shards with ranges where the even cut would fall; _begin / _wait_unit / _end waiting on a SHA-512 head's last
    tail first -- in a fresh process so that the environment switch is seen"""
    script = tmp_path / "w.py"
    script.write_text(WORKER % (ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script), mode], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0 and b"SHA512_WORKER_OK" in p.stdout, p.stdout.decode()[-3000:]
    if mode == "jobs":
        cuts = [int(m.group(2)) for m in re.finditer(rb"(\d+) units in (\d+) chunks", p.stdout) if int(m.group(1)) > 640]
        assert cuts and max(cuts) >= 2, p.stdout.decode()[-3000:]


def test_rejections(built):
    """the host entry points refuse a bad table with the unit's index in the message, before anything is touched"""
    arena = np.zeros(256, dtype=np.uint8)

    def table(rows):
        u = np.zeros(len(rows), dtype=M.UNIT_DTYPE)
        u["kind"] = [r[0] for r in rows]; u["out_off"] = [r[1] for r in rows]; u["out_len"] = [r[2] for r in rows]
        return u
    more = (M.KIND_DIGEST_MORE, 0, 0)
    cases = [
        (table([(M.KIND_MD5, 0, 10), (M.KIND_SHA384, 0, 10), more]), "unit 1: a SHA-384 unit must be followed by 2 MSPACK_HIP_KIND_DIGEST_MORE units"),
        (table([(M.KIND_SHA512, 0, 10), more, more, (M.KIND_MD5, 0, 10)]), "unit 0: a SHA-512 unit must be followed by 3 MSPACK_HIP_KIND_DIGEST_MORE units"),
        (table([(M.KIND_MD5, 0, 10), (M.KIND_SHA512, 0, 10)]), "unit 1: a wide digest unit is the table's last unit"),
        (table([(M.KIND_SHA256, 0, 10), more, more]), "unit 2: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it"),
        (table([(M.KIND_SHA384, 0, 10), more, more, more]), "unit 3: an MSPACK_HIP_KIND_DIGEST_MORE unit without"),
        (table([(M.KIND_SHA512, 0, 10), more, more, more, more]), "unit 4: an MSPACK_HIP_KIND_DIGEST_MORE unit without"),
        (table([(M.KIND_SHA384, 0, 10), more, (M.KIND_DIGEST_MORE, 0, 1)]), "unit 2: an MSPACK_HIP_KIND_DIGEST_MORE unit names no bytes"),
        (table([(M.KIND_MD5, 0, 10), more]), "unit 1: an MSPACK_HIP_KIND_DIGEST_MORE unit without"),
        (table([(M.KIND_SHA512, 60, 5), more, more, more]), "unit 0: a digest unit's range leaves the output arena"),
    ]
    u = table([(M.KIND_SHA384, 0, 10), more, more]); u["flags"][0] = M.UF_CRC32
    cases.append((u, "unit 0: a digest unit decodes nothing to take a CRC-32 of"))
    u = table([(M.KIND_SHA512, 0, 10), more, more, more]); u["in_len"][0] = 1
    cases.append((u, "unit 0: a digest unit reads no input"))
    for bad in (21, 22, 23):
        u = table([(M.KIND_MD5, 0, 10), more]); u["kind"][1] = bad
        cases.append((u, "unit 1: unknown kind %d" % bad))
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
