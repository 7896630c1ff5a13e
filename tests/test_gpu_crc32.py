"""MSPACK_HIP_UF_CRC32 (include/mspack_hip.h): the CRC-32 of every flagged unit's decoded bytes, computed on the device behind
the decode and returned in result.in_used -- the OAB block check: reflected 0xEDB88320 from 0xFFFFFFFF, not inverted, i.e.
zlib.crc32(out[:out_len]) ^ 0xFFFFFFFF.  Everything goes through the C ABI; the reference for the digest is zlib, the reference
for everything else is the same batch without the flag.

tests/test_crc32_emu.py runs the first three tests of this file on the wavefront emulator."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import libmspack_amd as M
import szdd_kwaj_recipe as SK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 65536                      # CRC_SEG of csrc/hip/crc32_kernel.hpp: one wavefront's share of a unit


def want_digest(out, off, n):
    return (zlib.crc32(out[int(off):int(off) + int(n)].tobytes()) ^ 0xFFFFFFFF) & 0xFFFFFFFF


def check_digests(units, out, res):
    for i in range(len(units)):
        assert res["out_len"][i] <= units["out_len"][i], (i, res[i])
        assert int(res["in_used"][i]) == want_digest(out, units["out_off"][i], res["out_len"][i]), \
            (i, int(units["kind"][i]), res[i], hex(int(res["in_used"][i])))


def same_but_in_used(units, out_a, res_a, out_b, res_b):
    """two runs of one batch: identical results but for in_used, identical decoded bytes"""
    for f in ("err", "flags", "out_len", "good_len", "in_next"):
        assert np.array_equal(res_a[f], res_b[f]), f
    for i in range(len(units)):
        o, n = int(units["out_off"][i]), int(res_a["out_len"][i])
        assert np.array_equal(out_a[o:o + n], out_b[o:o + n]), i


def mszip_stored(data):
    """an MSZIP folder of stored deflate blocks: every length decodes exactly"""
    data = bytes(data)
    out = []
    for k in range(0, len(data), 32768):
        b = data[k:k + 32768]
        out.append(b"CK\x01" + len(b).to_bytes(2, "little") + (len(b) ^ 0xFFFF).to_bytes(2, "little") + b)
    return b"".join(out)


def mszip_deflate(d):
    blocks, prev = [], None
    for k in range(0, len(d), 32768):
        b = bytes(d[k:k + 32768])
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, 0, prev) if prev else zlib.compressobj(6, zlib.DEFLATED, -15)
        blocks.append(b"CK" + c.compress(b) + c.flush()); prev = b
    return blocks


def lay_out(items, residues=None):
    """items: (kind, stream, out_len, window_bits, reset_frames, ref bytes) -> (units, arena, out_bytes, refs); output regions back to
    back with room for everything a kind owns, out_off = a multiple of 16 plus the item's residue"""
    offs, pos = [], 0
    for it in items:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(it[1])
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for it, o in zip(items, offs):
        arena[o:o + len(it[1])] = np.frombuffer(it[1], dtype=np.uint8)
    units, _ = M.make_units(np.array([it[0] for it in items], dtype=np.uint8), offs, [len(it[1]) for it in items],
                            [it[2] for it in items], window_bits=[it[3] for it in items], reset_frames=[it[4] for it in items],
                            ref_lens=[len(it[5]) for it in items])
    pos = 0
    for i, it in enumerate(items):
        below = 4096 if it[0] in (M.KIND_LZSS, M.KIND_KWAJ_LZH) else (len(it[5]) + 15) & ~15
        above = 32768 if it[0] == M.KIND_MSZIP else 0
        units["out_off"][i] = pos + below + (residues[i] if residues is not None else 0)
        pos += (below + it[2] + above + 16 + 15) & ~15
    return units, arena, pos, [it[5] for it in items]


def six_kinds(seed=3, n_each=3):
    rng = np.random.default_rng(seed)
    items = []
    for i in range(n_each):
        d = M.gen_plaintext(seed * 100 + i, int(rng.integers(0, 4)), 65536 + 777 * i)
        lz, _fo = M.lzx_encode(d, 17, 0)
        items.append((M.KIND_LZX, lz.tobytes(), d.size, 17, 0, b""))
        ref = M.gen_plaintext(seed * 200 + i, 0, 20000).tobytes()
        d = np.frombuffer(ref[:9000] + M.gen_plaintext(seed * 300 + i, 1, 30000 + i).tobytes() + ref[5000:], dtype=np.uint8)
        items.append((M.KIND_LZX_DELTA, M.lzxd_encode(d, 17, ref).tobytes(), d.size, 17, 0, ref))
        d = M.gen_plaintext(seed * 400 + i, 0, 32768 * (i + 1) + 11 * i)
        items.append((M.KIND_MSZIP, b"".join(mszip_deflate(d)), d.size, 0, 0, b""))
        d = M.gen_plaintext(seed * 500 + i, 0, 40000 + i)
        qs, _fs = M.qtm_encode(d, 17)
        items.append((M.KIND_QUANTUM, bytes(qs), d.size, 17, 0, b""))
        x = M.gen_plaintext(seed * 600 + i, 1, 5000 + 13 * i).tobytes()
        c = SK.lzss_encode(x, i % 3)
        items.append((M.KIND_LZSS, c, len(c) * 9 + 64, i % 3, 0, b""))
        c = SK.lzh_encode(x)
        items.append((M.KIND_KWAJ_LZH, c, len(c) * 18 + 4096, 0, 0, b""))
    return [items[k] for k in rng.permutation(len(items))]


def run_both(items, residues=None):
    units, arena, out_bytes, refs = lay_out(items, residues)
    out0, res0 = M.decode_batch(units, arena, out_bytes, refs=refs)
    flagged = units.copy(); flagged["flags"] |= M.UF_CRC32
    out1, res1 = M.decode_batch(flagged, arena, out_bytes, refs=refs)
    same_but_in_used(units, out0, res0, out1, res1)
    check_digests(flagged, out1, res1)
    return units, arena, out_bytes, refs, res0, res1


def test_mixed_batch_of_all_six_kinds(built):
    """units of every decoding kind in one batch: with the flag every in_used is zlib's answer for the unit's bytes; without it the same
    batch gives the same results and bytes, and in_used is the diagnostic count -- the same one whatever the run (a second unflagged
    run, and units whose NEIGHBOURS carry the flag)"""
    assert M.features() & M.FEAT_CRC32
    assert b"0.4" in M.lib().mspack_hip_version()
    items = six_kinds()
    assert sorted(set(it[0] for it in items)) == [1, 2, 3, 4, 5, 6]
    units, arena, out_bytes, refs, res0, res1 = run_both(items)
    assert (res1["err"] == 0).all()
    _out, again = M.decode_batch(units, arena, out_bytes, refs=refs)
    assert np.array_equal(again["in_used"], res0["in_used"])
    half = units.copy(); half["flags"][::2] |= M.UF_CRC32
    out2, res2 = M.decode_batch(half, arena, out_bytes, refs=refs)
    assert np.array_equal(res2["in_used"][1::2], res0["in_used"][1::2])
    check_digests(half[::2], out2, res2[::2])
    # the diagnostic count is no digest: the flag is what makes the difference
    assert not np.array_equal(res0["in_used"], res1["in_used"])


LENGTHS = [0, 1, 3, 4, 63, 64, 65, 32767, 32768, SEG - 1, SEG, SEG + 1, 3 * SEG + 5]


def test_lengths_and_alignments(built):
    """exact lengths (stored MSZIP blocks; literal-only LZSS streams for the short ones) at every residue of out_off mod 16: ragged heads
    and tails, the segment boundary from both sides, more than one segment per unit"""
    rng = np.random.default_rng(9)
    items, residues = [], []
    for n in LENGTHS:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for r in range(16):
            if n <= 65 and r % 2:
                body = b"".join(b"\xff" + data[k:k + 8] for k in range(0, n, 8))        # LZSS: a control byte of eight literals
                items.append((M.KIND_LZSS, body, n + 32, 0, 0, b"", data))
            else:
                items.append((M.KIND_MSZIP, mszip_stored(data), n, 0, 0, b"", data))
            residues.append(r)
    units, arena, out_bytes, refs, res0, res1 = run_both(items, residues)
    assert sorted(set(int(o) % 16 for o in units["out_off"])) == list(range(16))
    for i, it in enumerate(items):
        assert res1["err"][i] == 0 and res1["out_len"][i] == len(it[6]), (i, res1[i])
        assert int(res1["in_used"][i]) == (zlib.crc32(it[6]) ^ 0xFFFFFFFF) & 0xFFFFFFFF, (i, len(it[6]), residues[i])
    assert (res1["in_used"][:16] == 0xFFFFFFFF).all()                    # out_len == 0


def test_damaged_streams(built):
    """bit flips and truncations of an LZX, an MSZIP and a Quantum stream: the digest covers exactly result.out_len bytes of what the
    failing unit left in its output region, and nothing else of the result changes"""
    rng = np.random.default_rng(1)
    d = M.gen_plaintext(5, M.TEXT_MIX, 70000)
    lz = M.lzx_encode(d, 17, 0, M.lzx_opts(mode=4, block_size=12345))[0].tobytes()
    zs = b"".join(mszip_deflate(d))
    qs = bytes(M.qtm_encode(d[:40000], 17)[0])
    items = []
    for kind, s, n in ((M.KIND_LZX, lz, d.size), (M.KIND_MSZIP, zs, d.size), (M.KIND_QUANTUM, qs, 40000)):
        for cut in [0, 1, 2, 3, 17, 1000, len(s) // 2, len(s) - 2, len(s) - 1]:
            items.append((kind, s[:cut], n, 17, 0, b""))
        for _ in range(14):
            b = bytearray(s)
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
            items.append((kind, bytes(b), n, 17, 0, b""))
    units, arena, out_bytes, refs, res0, res1 = run_both(items)
    assert (res1["err"] != 0).sum() >= len(items) // 3
    assert len(set(int(x) for x in res1["out_len"])) > 5                 # (failures at many different points)


def test_long_units(built):
    """one LZX folder with a frame table and one MSZIP folder with a block table, 64 MiB each: 1024 segments per unit"""
    n = 64 << 20
    d = np.tile(M.gen_plaintext(77, M.TEXT_MIX, 1 << 20), 64)
    d[::4099] ^= np.arange(d[::4099].size, dtype=np.uint64).astype(np.uint8)           # (no two MiB alike)
    lz, fo = M.lzx_encode(d, 21, 0)
    blocks = mszip_deflate(d)
    ztab = np.cumsum([0] + [len(b) for b in blocks[:-1]]).astype(np.uint32)
    ltab = fo.astype(np.uint32)[:-1]
    zs = b"".join(blocks)
    pos = [0]

    def put(nbytes, align=16):
        pos[0] = (pos[0] + align - 1) & ~(align - 1)
        o = pos[0]; pos[0] += nbytes
        return o
    o_lz, o_zs, o_lt, o_zt = put(lz.size), put(len(zs)), put(4 * ltab.size), put(4 * ztab.size)
    arena = np.zeros(pos[0] + 64, dtype=np.uint8)
    arena[o_lz:o_lz + lz.size] = lz
    arena[o_zs:o_zs + len(zs)] = np.frombuffer(zs, dtype=np.uint8)
    arena[o_lt:o_lt + 4 * ltab.size] = ltab.view(np.uint8)
    arena[o_zt:o_zt + 4 * ztab.size] = ztab.view(np.uint8)
    units, out_bytes = M.make_units(np.array([M.KIND_LZX, M.KIND_MSZIP], dtype=np.uint8), [o_lz, o_zs], [lz.size, len(zs)], [n, n],
                                    window_bits=21, out_slack=32768, frame_tabs=[o_lt, o_zt])
    units["flags"] |= M.UF_CRC32
    units["out_off"][1] += 5; out_bytes += 16                             # (and not aligned)
    out, res = M.decode_batch(units, arena, out_bytes)
    assert (res["err"] == 0).all() and (res["out_len"] == n).all(), res
    for i in range(2):
        o = int(units["out_off"][i])
        assert np.array_equal(out[o:o + n], d), i
    check_digests(units, out, res)


def test_large_batch(built):
    """4096 small flagged units (the digest pass's one-wave-per-unit shape)"""
    n, ub = 4096, 4096 + 37
    plain, comp, off, ln = M.corpus_lzx_units(0xC4C, M.TEXT_MIX, n, ub, 17)
    units, out_bytes = M.make_units(M.KIND_LZX, off, ln + 4, np.full(n, ub), window_bits=17, reset_frames=1, flags=M.UF_CRC32)
    out, res = M.decode_batch(units, comp, out_bytes)
    assert (res["err"] == 0).all() and (res["out_len"] == ub).all()
    want = np.array([(zlib.crc32(plain[i * ub:(i + 1) * ub].tobytes()) ^ 0xFFFFFFFF) & 0xFFFFFFFF for i in range(n)], dtype=np.uint32)
    assert np.array_equal(res["in_used"], want)
    check_digests(units[:64], out, res[:64])


def test_checksum_units_reject_the_flag(built):
    arena = np.zeros(256, dtype=np.uint8)
    u = np.zeros(1, dtype=M.UNIT_DTYPE)
    u["kind"] = 7; u["in_len"] = 100; u["flags"] = M.UF_CRC32
    with pytest.raises(M.MspackHipError, match="checksum unit"):
        M.decode_batch(u, arena, 64)
    u["flags"] = 0
    M.decode_batch(u, arena, 64)


def test_to_device(built):
    """host input, device output: the digest of bytes that never came back -- compared after a copy of the test's own"""
    from test_gpu_hostpath import DevBuf
    units, arena, out_bytes, refs = lay_out(six_kinds(seed=8, n_each=4))
    units["flags"] |= M.UF_CRC32
    d_out = DevBuf(out_bytes + 64)
    for u, r in zip(units, refs):                                        # (LZX DELTA reference data must already be there)
        if len(r):
            h = np.frombuffer(r, dtype=np.uint8)
            assert d_out.hip.hipMemcpy(d_out.ptr + int(u["out_off"]) - len(r), h.ctypes.data, len(r), 1) == 0
    res = np.zeros(len(units), dtype=M.RESULT_DTYPE)
    u = np.ascontiguousarray(units)
    rc = M.lib().mspack_hip_decode_batch_to_device(u.ctypes.data, len(u), arena.ctypes.data, arena.size, d_out.ptr, out_bytes + 64,
                                                   res.ctypes.data)
    assert rc == 0, M.lib().mspack_hip_last_error()
    assert (res["err"] == 0).all()
    check_digests(units, d_out.to_host(), res)
    d_out.free()


def big_batch(flag):
    """enough units and bytes for the host path to cut chunks (>= 8 MiB of input and >= 256 units each): LZX with frame tables + MSZIP"""
    n, ub = 640, 65536
    plain, comp, off, ln, tab = M.corpus_lzx_units(0xCC32, M.TEXT_RANDOM, n, ub, 17, frame_tables=True)
    units, out_bytes = M.make_units(M.KIND_LZX, off, ln + 4, np.full(n, ub), window_bits=17, reset_frames=2, frame_tabs=tab,
                                    flags=flag)
    return units, comp, out_bytes, plain.reshape(n, ub)


WORKER = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import libmspack_amd as M
import test_gpu_crc32 as T
mode = sys.argv[1]
units, arena, out_bytes, refs = T.lay_out(T.six_kinds(seed=12, n_each=6))
units["flags"] |= M.UF_CRC32
if mode == "shards":
    assert os.environ["MSPACK_HIP_FORCE_SHARDS"] == "3"
    out, res = M.decode_batch(units, arena, out_bytes, n_devices=2, refs=refs)
    assert (res["err"] == 0).all()
    T.check_digests(units, out, res)
    # the shards' output spans interleave: the copies back go unit by unit (the non-monotone path)
    out, res = M.decode_batch(units[::-1].copy(), arena, out_bytes, n_devices=2, refs=refs[::-1])
    T.check_digests(units[::-1].copy(), out, res)
else:
    assert os.environ["MSPACK_PY_VIA_JOBS"] == "1"
    out, res = M.decode_batch(units, arena, out_bytes, refs=refs)
    T.check_digests(units, out, res)
units, comp, out_bytes, plain = T.big_batch(M.UF_CRC32)
out, res = M.decode_batch(units, comp, out_bytes, n_devices=2 if mode == "shards" else 1)
assert (res["err"] == 0).all() and np.array_equal(out[:plain.size].reshape(plain.shape), plain)
T.check_digests(units, out, res)
print("CRC_WORKER_OK")
'''


@pytest.mark.parametrize("mode,env", [("shards", {"MSPACK_HIP_FORCE_SHARDS": "3"}), ("jobs", {"MSPACK_PY_VIA_JOBS": "1"})])
def test_sharded_and_job_entry_points(built, mode, env, tmp_path):
    """mspack_hip_decode_batch_multi cut into three shards, and _begin / _wait_unit / _end: a mixed batch, and a batch large enough to
    be cut into chunks (LZX units with frame tables) -- in a fresh process so that the environment switch is seen"""
    script = tmp_path / "w.py"
    script.write_text(WORKER % (ROOT, ROOT))
    p = subprocess.run([sys.executable, str(script), mode], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0 and b"CRC_WORKER_OK" in p.stdout, p.stdout.decode()[-3000:]


def test_chunked_host_path_and_interleaved_outputs(built):
    """the chunked pipeline (one digest launch per chunk) and the per-unit copy-back of outputs that do not ascend with the inputs"""
    units, comp, out_bytes, plain = big_batch(M.UF_CRC32)
    out, res = M.decode_batch(units, comp, out_bytes)
    assert (res["err"] == 0).all() and np.array_equal(out[:plain.size].reshape(plain.shape), plain)
    check_digests(units, out, res)
    units, arena, out_bytes, refs = lay_out(six_kinds(seed=4, n_each=2))
    units["flags"] |= M.UF_CRC32
    rev = units[::-1].copy()                                              # inputs now descend while the outputs ascend
    out, res = M.decode_batch(rev, arena, out_bytes, refs=refs[::-1])
    assert (res["err"] == 0).all()
    check_digests(rev, out, res)


def test_device_resident_entry(built):
    """mspack_hip_decode_batch_device: the unit table lives on the device, so the digest pass runs only when the caller sets
    MSPACK_HIP_MASK_CRC32 -- present with the bit, absent (in_used as without the flag) without it"""
    from test_gpu_hostpath import DevBuf
    items = [it for it in six_kinds(seed=6, n_each=4) if it[0] in (M.KIND_LZX, M.KIND_MSZIP, M.KIND_QUANTUM)]
    units, arena, out_bytes, refs = lay_out(items)
    _o, plain_res = M.decode_batch(units, arena, out_bytes)
    units["flags"] |= M.UF_CRC32
    fr = M.frames_of(units)
    units["frame_base"] = np.concatenate([[0], np.cumsum(fr)[:-1]])
    n_frames = int(fr.sum())
    L = M.lib()
    scratch = DevBuf(L.mspack_hip_frame_scratch_bytes(n_frames))
    d_units, d_in, d_out = DevBuf(units.nbytes), DevBuf(arena.size + 64), DevBuf(out_bytes + 64)
    d_res = DevBuf(len(units) * M.RESULT_DTYPE.itemsize)
    hip = d_out.hip
    u = np.ascontiguousarray(units)
    assert hip.hipMemcpy(d_units.ptr, u.ctypes.data, u.nbytes, 1) == 0
    assert hip.hipMemcpy(d_in.ptr, arena.ctypes.data, arena.size, 1) == 0
    mask = (1 << M.KIND_LZX) | (1 << M.KIND_MSZIP) | (1 << M.KIND_QUANTUM)
    for m, digest in ((mask, False), (mask | M.MASK_CRC32, True)):
        rc = L.mspack_hip_decode_batch_device(d_units.ptr, None, len(u), d_in.ptr, arena.size, d_out.ptr, out_bytes, d_res.ptr,
                                              scratch.ptr, n_frames, m, None)
        assert rc == 0, L.mspack_hip_last_error()
        hip.hipDeviceSynchronize()
        res = d_res.to_host().view(M.RESULT_DTYPE)
        assert (res["err"] == 0).all()
        if digest:
            check_digests(units, d_out.to_host(), res)
        else:
            assert np.array_equal(res["in_used"], plain_res["in_used"])
    for b in (scratch, d_units, d_in, d_out, d_res):
        b.free()
