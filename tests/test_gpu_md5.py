"""MSPACK_HIP_KIND_MD5 (include/mspack_hip.h): digest units -- the MD5 of a byte range of the output arena, one lane per range, behind
everything else of the batch.  Everything goes through the C ABI; the reference for a digest is hashlib.md5 over the bytes that lie
in the range, the reference for everything else is the same batch without digest units.

tests/test_md5_emu.py runs the first three groups of this file (lengths and alignments, batch shapes, edges and guards) on the
wavefront emulator; the 1 MiB range stays with the GPU."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import libmspack_amd as M
import test_gpu_crc32 as T
from test_gpu_hostpath import DevBuf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096

RFC1321 = [(b"", "d41d8cd98f00b204e9800998ecf8427e"), (b"a", "0cc175b9c0f1b6a831c399e269772661"),
           (b"abc", "900150983cd24fb0d6963f7d28e17f72"), (b"message digest", "f96b697d7cb7938d525a2f31aaf161d0"),
           (b"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"),
           (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"),
           (b"1234567890" * 8, "57edf4a22be3c955ac49da2e2107b67a")]


def md5(b):
    return hashlib.md5(bytes(b)).digest()


def dev_write(buf, off, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    if not arr.size:
        return
    if buf.emu is not None:
        C.memmove(buf.ptr + off, arr.ctypes.data, arr.size)              # (the emulator's device memory is host memory)
    else:
        assert buf.hip.hipMemcpy(buf.ptr + off, arr.ctypes.data, arr.size, 1) == 0


def run_device(data, ranges, order=None, extra_mask=0):
    """digest units over a device buffer that is exactly len(data) bytes long, inside a larger allocation of 0xA5: the call through
    mspack_hip_decode_batch_device (no decoding units), the digests, and the checks that nothing but the results was written"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n = data.size
    units = M.md5_units(ranges)
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
                                          d_res.ptr, None, 0, M.MASK_MD5 | extra_mask, None)
    assert rc == 0, L.mspack_hip_last_error()
    if big.emu is None:
        assert big.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(units) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE)
    after = big.to_host()
    assert (after[:GUARD] == 0xA5).all() and (after[GUARD + n:] == 0xA5).all()          # the guard bytes
    assert np.array_equal(after[GUARD:GUARD + n], data)                                   # the arena after the call is the arena before it
    for b in (big, d_units, d_res) + ((d_order,) if d_order else ()):
        b.free()
    assert (res["err"] == 0).all() and (res["flags"] == 0).all(), res
    return M.result_digests(res)


def check(data, ranges, got):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    for (o, n), d in zip(ranges, got):
        assert d == md5(data[o:o + n]), (o, n, d.hex())


LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 4095, 4096, 4097]
RESIDUES = list(range(16)) + [63]        # out_off mod 16 = 0 .. 15; mod 64 = 0, 1 (the first two: every slot starts on a multiple of 64) and 63


def lengths_layout(lengths):
    ranges, pos = [], 0
    for n in lengths:
        for r in RESIDUES:
            pos = (pos + 63) & ~63
            ranges.append((pos + r, n))
            pos += r + n
    return ranges, pos


def test_lengths_and_alignments(built):
    """every length at which the pad or the loader changes its path (55 / 56 / 57: one final block or two; 63 / 64 / 65: the block
    edge; the row, dword and funnel-shift loaders' first and last words) at every out_off mod 16 and at out_off mod 64 = 0, 1, 63"""
    assert M.features() & M.FEAT_MD5
    ranges, total = lengths_layout(LENGTHS)
    assert sorted(set(o % 16 for o, _n in ranges)) == list(range(16)) and {0, 1, 63} <= set(o % 64 for o, _n in ranges)
    data = np.random.default_rng(1321).integers(0, 256, total, dtype=np.uint8)
    check(data, ranges, run_device(data, ranges))


def test_rfc1321_strings(built):
    """the test suite of RFC 1321, appendix A.5, back to back in one arena (so at seven different alignments)"""
    data = np.frombuffer(b"".join(s for s, _h in RFC1321), dtype=np.uint8)
    ranges, pos = [], 0
    for s, _h in RFC1321:
        ranges.append((pos, len(s))); pos += len(s)
    got = run_device(data, ranges)
    assert [d.hex() for d in got] == [h for _s, h in RFC1321]


def test_one_long_range(built):
    """1 MiB + 3 bytes: the loop count (16385 blocks), at three alignments beside short neighbours in the same wave"""
    n = (1 << 20) + 3
    data = np.random.default_rng(7).integers(0, 256, 3 * n + 300, dtype=np.uint8)
    ranges = [(0, n), (n + 1, n), (2 * n + 7, n), (5, 100), (3 * n + 200, 64)]
    check(data, ranges, run_device(data, ranges))


@pytest.mark.parametrize("n_units", [1, 63, 64, 65, 130])
def test_batch_shapes(built, n_units):
    """n units of n different lengths, shuffled and descending: a last wave with one live lane, loops that end at a different
    count in every lane; the same batch again through a d_order permutation; identical and overlapping ranges"""
    rng = np.random.default_rng(100 + n_units)
    lens = [(11 * i + 5) % 1499 + (i == 0) * 2000 for i in range(n_units)]
    assert len(set(lens)) == n_units
    data = rng.integers(0, 256, 4096, dtype=np.uint8)
    shuffled = [(int(rng.integers(0, 4096 - n)), n) for n in (lens[k] for k in rng.permutation(n_units))]
    descending = sorted(shuffled, key=lambda r: -r[1])
    for ranges in (shuffled, descending):
        check(data, ranges, run_device(data, ranges))
    perm = rng.permutation(n_units).astype(np.uint32)
    check(data, shuffled, run_device(data, shuffled, order=perm))
    same = [(77, 333), (77, 333), (100, 200), (150, 200), (77, 333)]
    check(data, same, run_device(data, same))


def test_arena_edges_and_guards(built):
    """one range ends on the arena's last byte, one begins on its first, one is the whole arena, one is empty at its end -- the arena
    is exactly out_bytes long inside an allocation of 0xA5 whose other bytes are checked (run_device)"""
    for n in (1, 61, 64, 1000, 1027):
        data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        ranges = [(n - min(n, 37), min(n, 37)), (0, min(n, 70)), (0, n), (n, 0), (n - 1, 1), (0, 1)]
        check(data, ranges, run_device(data, ranges))


# ---- behind the decoders --------------------------------------------------------------------------------------------------

def damaged_item():
    d = M.gen_plaintext(5, M.TEXT_MIX, 70000)
    lz = bytearray(M.lzx_encode(d, 17, 0, M.lzx_opts(mode=4, block_size=12345))[0].tobytes())
    lz[len(lz) // 2] ^= 0x10
    return (M.KIND_LZX, bytes(lz[:len(lz) - 900]), d.size, 17, 0, b"")


def mixed_batch(seed=3, n_each=2):
    """units of all six decoding kinds + one damaged LZX stream; per unit a digest range over its whole output room, one over a ragged
    part of it, and one from the middle of the unit to the middle of the next one (the padding and slack between them included)"""
    items = T.six_kinds(seed=seed, n_each=n_each) + [damaged_item()]
    units, arena, out_bytes, refs = T.lay_out(items)
    ranges = []
    for i, u in enumerate(units):
        o, n = int(u["out_off"]), int(u["out_len"])
        ranges.append((o, n))
        ranges.append((o + min(n, 1 + 3 * i), max(0, n - 1 - 3 * i - min(n // 3, 5 * i + 2))))
        if i + 1 < len(units):
            o2, n2 = int(units["out_off"][i + 1]), int(units["out_len"][i + 1])
            ranges.append((o + n // 2, o2 + n2 // 2 - (o + n // 2)))
    return units, arena, out_bytes, refs, ranges


def check_mixed(units, out, res, digests, ranges, plain_out, plain_res):
    """the digests are those of the bytes the call left in the arena; every decoding unit's result and bytes are those of the batch
    without digest units"""
    assert np.array_equal(res, plain_res)
    for i in range(len(units)):
        o, n = int(units["out_off"][i]), int(plain_res["out_len"][i])
        assert np.array_equal(out[o:o + n], plain_out[o:o + n]), i
    check(out, ranges, digests)


def test_behind_the_decoders(built):
    """one mixed batch through mspack_hip_decode_batch: the digest pass sees what every decoder stored (E8 and resume passes included),
    also what the damaged stream left"""
    units, arena, out_bytes, refs, ranges = mixed_batch()
    assert sorted(set(int(k) for k in units["kind"])) == [1, 2, 3, 4, 5, 6]
    plain_out, plain_res = M.decode_batch(units, arena, out_bytes, refs=refs)
    assert plain_res["err"][-1] != 0 and (plain_res["err"][:-1] == 0).all()
    out, res, digests = M.decode_batch_md5(units, arena, out_bytes, ranges, refs=refs)
    check_mixed(units, out, res, digests, ranges, plain_out, plain_res)
    # whole-unit ranges of the good units: the digest of the decoded bytes as the run without digest units has them
    for i in range(len(units) - 1):
        if plain_res["out_len"][i] == units["out_len"][i]:
            o, n = int(units["out_off"][i]), int(units["out_len"][i])
            assert digests[ranges.index((o, n))] == md5(plain_out[o:o + n]), i


def test_device_resident_entry_behind_the_decoders(built):
    """mspack_hip_decode_batch_device with decoding units of all six kinds (one stream damaged) AND digest units in one table:
    kind_mask = every codec, with and without the MD5 bit, and with MSPACK_HIP_MASK_CRC32 beside it.  Without the bit no digest unit's
    result is touched; with it the digests are those of the bytes the call left in the device buffer (behind the codecs, the E8
    and the resume pass, and the CRC pass), and every decoding unit's result and bytes are those of the call without the bit"""
    units, arena, out_bytes, refs, ranges = mixed_batch(seed=21)
    nd = len(units)
    both = np.concatenate([units, M.md5_units(ranges)])
    fr = M.frames_of(both)
    both["frame_base"] = np.concatenate([[0], np.cumsum(fr)[:-1]])
    n_frames = int(fr.sum())
    L = M.lib()
    scratch = DevBuf(max(L.mspack_hip_frame_scratch_bytes(n_frames), 16))
    d_units, d_in = DevBuf(both.nbytes), DevBuf(arena.size + 64)
    dev_write(d_units, 0, both.view(np.uint8))
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

    out0, res0 = call(codecs)
    assert res0["err"][nd - 1] != 0 and (res0["err"][:nd - 1] == 0).all()
    assert (res0[nd:].view(np.uint8) == 0x77).all()                         # no MD5 bit: the digest units' results are untouched
    out1, res1 = call(codecs | M.MASK_MD5)
    assert np.array_equal(res1[:nd], res0[:nd])
    for i in range(nd):
        o, n = int(units["out_off"][i]), int(res0["out_len"][i])
        assert np.array_equal(out1[o:o + n], out0[o:o + n]), i
    assert (res1["err"][nd:] == 0).all() and (res1["flags"][nd:] == 0).all()
    check(out1, ranges, M.result_digests(res1[nd:]))
    # ... and beside the CRC pass: both digests of the same bytes
    out2, res2 = call(codecs | M.MASK_MD5 | M.MASK_CRC32, flags=M.UF_CRC32)
    check(out2, ranges, M.result_digests(res2[nd:]))
    T.check_digests(units, out2, res2[:nd])
    for f in ("err", "flags", "out_len", "good_len", "in_next"):
        assert np.array_equal(res2[f][:nd], res0[f][:nd]), f
    for b in (scratch, d_units, d_in):
        b.free()


def test_to_device(built):
    """host input, device output: digests of bytes that never came back -- compared after a copy of the test's own"""
    units, arena, out_bytes, refs, ranges = mixed_batch(seed=8)
    d_out = DevBuf(out_bytes + 64)
    for u, r in zip(units, refs):
        if len(r):
            dev_write(d_out, int(u["out_off"]) - len(r), np.frombuffer(r, dtype=np.uint8))
    both = np.concatenate([units, M.md5_units(ranges)])
    res = np.zeros(len(both), dtype=M.RESULT_DTYPE)
    rc = M.lib().mspack_hip_decode_batch_to_device(both.ctypes.data, len(both), arena.ctypes.data, arena.size, d_out.ptr, out_bytes + 64,
                                                   res.ctypes.data)
    assert rc == 0, M.lib().mspack_hip_last_error()
    assert (res["err"][len(units):] == 0).all() and (res["flags"][len(units):] == 0).all()
    check(d_out.to_host(), ranges, M.result_digests(res[len(units):]))
    d_out.free()


def chunked_batch():
    """enough units and bytes for the planner to cut chunks (>= 8 MiB of input, >= 256 units each); the output regions lie back to back
    (65536 bytes each), so a range may straddle a cut without padding that no copy brings back"""
    n, ub = 640, 65536
    plain, comp, off, ln, tab = M.corpus_lzx_units(0xCC32, M.TEXT_RANDOM, n, ub, 17, frame_tables=True)
    units, out_bytes = M.make_units(M.KIND_LZX, off, ln + 4, np.full(n, ub), window_bits=17, reset_frames=2, frame_tabs=tab)
    ranges = [(i * ub - 1000 - i, 2000 + 3 * i) for i in range(1, n, 7)] + [(0, 5 * ub + 1), (out_bytes - 77, 77), (100 * ub + 3, 300 * ub)]
    return units, comp, out_bytes, plain, ranges


def test_chunked_host_path(built):
    """a batch the planner cuts into chunks: ranges that straddle every possible cut (one begins a little before every seventh unit's
    region and ends in it), and one long range over 300 units"""
    units, comp, out_bytes, plain, ranges = chunked_batch()
    # the planner's rule for this table (host_plan.hpp: plan_chunks; the knobs' defaults, which no variable may have changed): as
    # many chunks as 8 MiB of input and 256 units each allow, four at most -- at least two here.  The job worker below sees the count
    assert not [k for k in os.environ if k.startswith("MSPACK_HIP_CHUNK") or k == "MSPACK_HIP_NCHUNKS"]
    assert min(4, int(units["in_len"].sum()) // (8 << 20), len(units) // 256) >= 2
    out, res, digests = M.decode_batch_md5(units, comp, out_bytes, ranges)
    assert (res["err"] == 0).all() and np.array_equal(out[:plain.size], plain)
    check(plain, ranges, digests)


WORKER = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import libmspack_amd as M
import test_gpu_md5 as T
mode = sys.argv[1]
units, arena, out_bytes, refs, ranges = T.mixed_batch(seed=12, n_each=3)
if mode == "jobs":
    assert os.environ["MSPACK_PY_VIA_JOBS"] == "1"
    # waiting on a digest unit FIRST: it returns when the batch is through, with the digest written
    both = np.concatenate([units, M.md5_units(ranges)])
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
    first = M.result_digests(res[len(units):])
    assert L.mspack_hip_job_end(job) == 0
    T.check(out, ranges, first)
    n_dev = 1
else:
    assert os.environ["MSPACK_HIP_FORCE_SHARDS"] in ("2", "3")
    n_dev = 2
plain_out, plain_res = M.decode_batch(units, arena, out_bytes, refs=refs, n_devices=n_dev)
out, res, digests = M.decode_batch_md5(units, arena, out_bytes, ranges, refs=refs, n_devices=n_dev)
T.check_mixed(units, out, res, digests, ranges, plain_out, plain_res)
# a batch of equal units: the even cuts fall behind unit n / 2 (n / 3, 2 n / 3) -- with a digest range across each of them
units, comp, out_bytes, plain, ranges = T.chunked_batch()
n, ub = len(units), 65536
ranges = ranges + [(k * ub - 5000, 10000) for k in (n // 2, n // 3, 2 * n // 3, n // 2 + 1, n // 3 + 1, 2 * n // 3 + 1)]
out, res, digests = M.decode_batch_md5(units, comp, out_bytes, ranges, n_devices=n_dev)
assert (res["err"] == 0).all() and np.array_equal(out[:plain.size], plain)
T.check(plain, ranges, digests)
print("MD5_WORKER_OK")
'''


@pytest.mark.parametrize("mode,env", [("shards", {"MSPACK_HIP_FORCE_SHARDS": "2"}), ("shards", {"MSPACK_HIP_FORCE_SHARDS": "3"}),
                                      ("jobs", {"MSPACK_PY_VIA_JOBS": "1", "MSPACK_HIP_TRACE": "1"})])
def test_sharded_and_job_entry_points(built, mode, env, tmp_path):
    """mspack_hip_decode_batch_multi cut into two and three shards with digest ranges where the even cuts would fall, and
    _begin / _wait_unit / _end waiting on a digest unit first -- in a fresh process so that the environment switch is seen"""
    script = tmp_path / "w.py"
    script.write_text(WORKER % (ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script), mode], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0 and b"MD5_WORKER_OK" in p.stdout, p.stdout.decode()[-3000:]
    if mode == "jobs":
        # the library's own trace: the chunked batch (640 units beside its digest units) was cut into at least two chunks
        import re
        cuts = [int(m.group(2)) for m in re.finditer(rb"(\d+) units in (\d+) chunks", p.stdout) if int(m.group(1)) > 640]
        assert cuts and max(cuts) >= 2, p.stdout.decode()[-3000:]


def test_rejections(built):
    """a range one byte beyond out_bytes, in_len = 1, the CRC flag: an error return with the message, before anything is touched"""
    assert M.features() & M.FEAT_MD5
    arena = np.zeros(256, dtype=np.uint8)
    good = M.md5_units([(0, 64), (10, 20)])
    for change, msg in ((lambda u: u["out_len"].__setitem__(1, 55), "unit 1: a digest unit's range leaves the output arena"),
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
    u = good.copy(); u["flags"][1] = 0x7F                                    # every other flag is ignored
    out = np.zeros(64, dtype=np.uint8)
    res = np.zeros(2, dtype=M.RESULT_DTYPE)
    assert M.lib().mspack_hip_decode_batch(u.ctypes.data, 2, arena.ctypes.data, arena.size, out.ctypes.data, out.size, res.ctypes.data) == 0
    assert (res["err"] == 0).all() and (res["flags"] == 0).all()
