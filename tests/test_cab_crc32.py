"""mspack_cabd_crc32() (include/mspack.h): extract() with the writes replaced by zlib's CRC-32.
  * `-m "not gpu"`: the driver on the CPU stand-in for the batch ABI, which reports no MSPACK_HIP_FEAT_CRC32_RANGES -- so every
    checksum is the host fallback's (csrc/host/crc32.h) whatever MSCABD_PARAM_HIP_CRC32 says: params, arguments, crc32() against
    zlib.crc32 of what extract() of a second, fresh decompressor wrote, and the sticky-state and Quantum-carry sequences of
    tests/test_cab_sticky.py with every second call replaced by crc32().
  * `-m gpu`: the param on, on the real library: 256 MSZIP folders of one 2 KiB file; an LZX folder of 40 frames whose largest file
    (about 90 % of the folder) the digest ratio sends to the host -- its crc32() is the device's; prefetch over four cabinets."""
import hashlib
import struct
import zlib

import pytest

import libmspack_amd as M
from libmspack_amd import api
import cab_recipe as R
import test_cab_md5 as T5
import test_cab_sticky as S
import test_gpu_drivers as GD

P = api.MSCABD_PARAM_HIP_CRC32


def crc(b):
    return zlib.crc32(bytes(b)) & 0xFFFFFFFF


def goldens(L, param, vecs):
    n_ok = 0
    for v in vecs:
        if v["open_err"] or not v["files"]:
            continue
        cab, p = GD.cab_bytes(v), v["params"]
        kw = dict(fix_mszip=p.get("fix_mszip", 0), salvage=p.get("salvage", 0), mem=True, L=L)
        for order in T5.orders(len(v["files"]), len(cab))[:3]:
            with api.Cab(cab, **kw) as a, api.Cab(cab, **kw) as b:
                assert a.set_param(P, param) == 0
                for i in order:
                    b.mem.outputs.clear()
                    err_x, data = b.extract(i)
                    a.mem.outputs.clear()
                    err, val = a.crc32(i)
                    assert err == err_x and val == (crc(data) if err_x == 0 else 0), (v["tag"], order, i, err, err_x)
                    assert not a.mem.outputs and a.d.contents.last_error(a.d) == err
                    n_ok += err == 0
    return n_ok


@pytest.mark.parametrize("param", [0, 1])
@pytest.mark.parametrize("half", [0, 1])
def test_crc32_is_extract_with_a_checksum_host_fallback_cpu(built, hostlogic, half, param):
    assert goldens(hostlogic, param, GD.CPU_VECS[half::2]) >= 30


def alternate(cab, run, L, param, tag):
    """a recorded all-extract() sequence on two decompressors: b extracts every file, a answers every second call with crc32() -- the
    codes are the recorded ones on both, a's checksum is that of the bytes b wrote (0 when the call fails), a's extract() writes
    what b's wrote: a crc32() call leaves the decompressor in the state an extract() leaves it in"""
    with api.Cab(cab, mem=True, L=L, salvage=run["salvage"]) as a, api.Cab(cab, mem=True, L=L, salvage=run["salvage"]) as b:
        assert a.set_param(P, param) == 0
        n_failed = 0
        for k, (i, exp) in enumerate(zip(run["order"], run["results"])):
            b.mem.outputs.clear()
            err_x, data = b.extract(i)
            assert err_x == exp["err"] and hashlib.md5(data).hexdigest() == exp["md5"], (tag, k, i)
            a.mem.outputs.clear()
            if k % 2:
                err, val = a.crc32(i)
                assert err == err_x and val == (crc(data) if err == 0 else 0), (tag, k, i, err, err_x)
                assert not a.mem.outputs
                n_failed += err != 0
            else:
                err, mine = a.extract(i)
                assert err == err_x and mine == data, (tag, k, i)
        return n_failed


@pytest.mark.parametrize("param", [0, 1])
def test_sticky_state_and_quantum_carry_cpu(built, hostlogic, param):
    n_failed = 0
    for v in S.GOLD:
        cab = R.base_cab(v["seed"], v["cut"])
        if v["victim"] is not None:
            struct.pack_into("<I", cab, R.file_entry_offsets(cab)[v["victim"]] + 4, 4521984)
        else:
            cab[v["flip"]] ^= v.get("flip_mask", 0x10)
        cab = bytes(cab)
        assert hashlib.md5(cab).hexdigest() == v["cab_md5"]
        for run in v["runs"]:
            n_failed += alternate(cab, run, hostlogic, param, ("sticky", v["seed"], run["order"]))
    for v in S.CARRY_GOLD[::3]:
        cab, _ = R.qtm_cab(v["seed"], v["wb"], v["cuts"], v["n"], v["kind"])
        if v["flip"] is not None:
            cab[v["flip"]] ^= 0x08
        for run in v["runs"]:
            n_failed += alternate(bytes(cab), run, hostlogic, param, ("carry", v["seed"], run["order"]))
    assert n_failed >= 10                                                 # failing calls give the code and 0


def test_params_and_arguments_cpu(built, hostlogic):
    v = [v for v in GD.VECS if "cab_b64" in v and not v["open_err"] and v["files"]][0]
    with api.Cab(GD.cab_bytes(v), mem=True, L=hostlogic) as c:
        assert c.get_param(P) == (0, 0)                                   # the default
        for value in (1, 0, 1):
            assert c.set_param(P, value) == 0 and c.get_param(P) == (0, value)
        for value in (2, -1, 8, 255):
            assert c.set_param(P, value) == api.MSPACK_ERR_ARGS and c.get_param(P) == (0, 1)
        assert c.get_param(api.MSCABD_PARAM_HIP_DIGESTS) == (0, 0)        # a param of its own: no bit of the digest mask
        assert c.set_param(104, 1) == api.MSPACK_ERR_ARGS and c.get_param(104)[0] == api.MSPACK_ERR_ARGS
        val = api.C.c_uint(0x55555555)
        assert c.L.mspack_cabd_crc32(None, c._files[0], api.C.byref(val)) == api.MSPACK_ERR_ARGS
        assert c.L.mspack_cabd_crc32(c.d, None, api.C.byref(val)) == api.MSPACK_ERR_ARGS and val.value == 0
        assert c.d.contents.last_error(c.d) == api.MSPACK_ERR_ARGS
        assert c.L.mspack_cabd_crc32(c.d, c._files[0], None) == api.MSPACK_ERR_ARGS
        b = api.Cab(GD.cab_bytes(v), mem=True, L=hostlogic)
        err_x, data = b.extract(0)
        b.close()
        assert c.crc32(0) == (err_x, crc(data)) and err_x == 0


def test_host_fallback_is_counted_cpu(built, hostlogic):
    api.cabd_crc32_counts(reset=True, L=hostlogic)
    v = [v for v in GD.VECS if "cab_b64" in v and not v["open_err"] and len(v["files"]) >= 2 and not v["params"].get("salvage")][0]
    with api.Cab(GD.cab_bytes(v), mem=True, L=hostlogic) as c:
        assert c.set_param(P, 1) == 0
        good = [i for i in range(len(v["files"])) if c.crc32(i)[0] == 0]
        assert good
    assert api.cabd_crc32_counts(L=hostlogic) == (0, len(good))
    assert api.cabd_crc32_counts(reset=True, L=hostlogic) == (0, len(good)) and api.cabd_crc32_counts(L=hostlogic) == (0, 0)


def test_prefetched_cabinets_cpu(built, hostlogic):
    vs = [v for v in GD.VECS if "cab_b64" in v and not v["open_err"] and v["files"] and not v["params"].get("fix_mszip")
          and not v["params"].get("salvage")]
    images = [GD.cab_bytes(v) for v in vs]
    with api.CabSet(images, mem=True, L=hostlogic) as a, api.CabSet(images, mem=True, L=hostlogic) as b:
        assert a.set_param(P, 1) == 0 and a.prefetch() == 0
        n = 0
        for c in reversed(range(len(images))):
            for fa, fb in zip(a.file_ptrs(c), b.file_ptrs(c)):
                err_x, data = b.extract(fb)
                assert a.crc32(fa) == (err_x, crc(data) if err_x == 0 else 0)
                n += err_x == 0
        assert n >= 8


# ---- the device ----------------------------------------------------------------------------------------------------------------------

def mszip_block(b):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return b"CK" + co.compress(bytes(b)) + co.flush()


@pytest.mark.gpu
def test_256_mszip_folders_are_answered_from_the_device_gpu(built):
    n, ub = 256, 2048
    plain = M.gen_plaintext(0xC32, 0, n * ub)
    cab = M.cab_write([(1, [mszip_block(plain[i * ub:(i + 1) * ub])], [ub]) for i in range(n)],
                      [(b"f%03d.bin" % i, ub, 0, i) for i in range(n)])
    api.cabd_crc32_counts(reset=True)
    with api.Cab(cab, mem=True) as c:
        assert c.set_param(P, 1) == 0
        for i in range(n):
            assert c.crc32(i) == (0, crc(plain[i * ub:(i + 1) * ub])), i
        assert not c.mem.outputs
    assert api.cabd_crc32_counts() == (n, 0)


def lzx_cab(seed, frames, cuts):
    n = frames * 32768
    data = M.gen_plaintext(seed, 0, n)
    lz, fo = M.lzx_encode(data, 17, 0)
    blocks = [lz[int(fo[i]):int(fo[i + 1])].tobytes() for i in range(len(fo) - 1)]
    sizes = [32768] * frames
    edges = [0] + list(cuts) + [n]
    files = [(b"part%d.bin" % k, edges[k + 1] - edges[k], edges[k], 0) for k in range(len(edges) - 1)]
    return M.cab_write([(3 | (17 << 8), blocks, sizes)], files), data.tobytes(), files


@pytest.mark.gpu
def test_the_file_the_digest_ratio_sends_to_the_host_gpu(built):
    """one LZX folder of 40 frames, three files, the middle one about 90 % of the folder: crc32() of it comes from the device, a
    digest() of the same file is still hashed on the host -- the counts of both calls say so"""
    n = 40 * 32768
    cab, data, files = lzx_cab(0x90, 40, [n // 20 + 3, n // 20 + 3 + (n * 9) // 10])
    assert files[1][1] > 0.89 * n
    api.cabd_crc32_counts(reset=True)
    api.cabd_digest_counts(api.MSPACK_DIGEST_MD5, reset=True)
    with api.Cab(cab, mem=True) as c:
        assert c.set_param(P, 1) == 0 and c.set_param(api.MSCABD_PARAM_HIP_DIGESTS, api.MSPACK_DIGEST_MD5) == 0
        for i, (_name, ln, off, _fo) in enumerate(files):
            assert c.crc32(i) == (0, crc(data[off:off + ln])), i
        assert api.cabd_crc32_counts() == (3, 0)
        assert c.digest(1, api.MSPACK_DIGEST_MD5) == (0, hashlib.md5(data[files[1][2]:files[1][2] + files[1][1]]).digest())
        assert api.cabd_digest_counts(api.MSPACK_DIGEST_MD5) == (0, 1)
        assert c.digest(0, api.MSPACK_DIGEST_MD5) == (0, hashlib.md5(data[:files[0][1]]).digest())
        assert api.cabd_digest_counts(api.MSPACK_DIGEST_MD5) == (1, 1)
        assert not c.mem.outputs


@pytest.mark.gpu
def test_prefetch_over_four_cabinets_gpu(built):
    made = [lzx_cab(0x40 + k, 2 + k, [1000 * (k + 1), 40000 + k]) for k in range(4)]
    api.cabd_crc32_counts(reset=True)
    M.lib().mspack_hip_host_path_stats(None, 1)
    with api.CabSet([m[0] for m in made], mem=True) as s:
        assert s.set_param(P, 1) == 0 and s.prefetch() == 0
        n = 0
        for k, (_cab, data, files) in enumerate(made):
            for fp, (_name, ln, off, _fo) in zip(s.file_ptrs(k), files):
                assert s.crc32(fp) == (0, crc(data[off:off + ln])), (k, off)
                n += 1
    assert api.cabd_crc32_counts() == (n, 0) and n == 12
    ms = (api.C.c_double * 4)()
    M.lib().mspack_hip_host_path_stats(ms, 0)
    assert int(ms[3]) == 1                                                # one batch
