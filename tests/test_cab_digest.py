"""mspack_cabd_digest() (include/mspack.h): extract() with the writes replaced by a hash, by algorithm.  The driver on the CPU stand-in
for the batch ABI, which has no feature word -- so every digest is the host fallback's (the plain-C SHA-1 / SHA-256 of
csrc/host/sha.c, the MD5 of csrc/host/md5.c) whatever MSCABD_PARAM_HIP_DIGESTS says.  The reference for a digest is hashlib over what
extract() of a second, fresh decompressor wrote; for codes it is that extract().  The device side is tests/test_gpu_sha.py's; here
only the cabinet whose file list runs in descending offset order, on both: the folder's table of kept digests
(csrc/host/host_digest.h) must answer every call from the device although its units arrive descending."""
import hashlib
import os

import pytest

from libmspack_amd import api
import test_cab_md5 as T5
import test_gpu_drivers as GD

ALGS = {api.MSPACK_DIGEST_MD5: hashlib.md5, api.MSPACK_DIGEST_SHA1: hashlib.sha1, api.MSPACK_DIGEST_SHA256: hashlib.sha256}


def goldens(L, param, vecs):
    """the driver-golden cabinets: digest(f, alg) against extract(f) of a second, fresh decompressor, every file, the algorithms in
    turn on one decompressor each, in list order and reversed"""
    n_ok = n_failed = 0
    for v in vecs:
        if v["open_err"] or not v["files"]:
            continue
        cab, p = GD.cab_bytes(v), v["params"]
        kw = dict(fix_mszip=p.get("fix_mszip", 0), salvage=p.get("salvage", 0), mem=True, L=L)
        for alg, h in ALGS.items():
            for order in T5.orders(len(v["files"]), len(cab))[:2]:
                with api.Cab(cab, **kw) as a, api.Cab(cab, **kw) as b:
                    assert a.set_param(api.MSCABD_PARAM_HIP_DIGESTS, param) == 0
                    for i in order:
                        b.mem.outputs.clear()
                        err_x, data = b.extract(i)
                        a.mem.outputs.clear()
                        err, dg = a.digest(i, alg)
                        want = h(data).digest() if err_x == 0 else bytes(api.DIGEST_BYTES[alg])
                        assert err == err_x and dg == want, (v["tag"], alg, order, i, err, err_x)
                        assert not a.mem.outputs                              # no output file was opened, nothing written
                        assert a.d.contents.last_error(a.d) == err
                        n_ok += err == 0
                        n_failed += err != 0
    return n_ok, n_failed


@pytest.mark.parametrize("param", [0, 7])
@pytest.mark.parametrize("half", [0, 1])
def test_digest_is_extract_with_a_hash_host_fallback_cpu(built, hostlogic, half, param):
    n_ok, _n_failed = goldens(hostlogic, param, GD.CPU_VECS[half::2])
    assert n_ok >= 30


def test_failing_and_partial_files_give_the_code_and_no_digest_cpu(built, hostlogic):
    """damaged folders: the code is extract()'s, the digest bytes are zeros (whatever the call hashed on its way)"""
    n_failed = 0
    for v in GD.CPU_VECS:
        if "mutation" not in v or v["open_err"] or not v["runs"]:
            continue
        for alg in ALGS:
            with api.Cab(GD.cab_bytes(v), salvage=v["params"].get("salvage", 0), mem=True, L=hostlogic) as c:
                assert c.set_param(api.MSCABD_PARAM_HIP_DIGESTS, 7) == 0
                run = v["runs"][0]
                for i, exp in zip(run["order"], run["results"]):
                    n = api.DIGEST_BYTES[alg]
                    d = (api.C.c_ubyte * n)(*([0x55] * n))
                    err = c.L.mspack_cabd_digest(c.d, c._files[i], alg, d, n)
                    assert err == exp["err"]
                    if err:
                        assert bytes(d) == bytes(n)
                        n_failed += 1
                    else:
                        assert bytes(d) != bytes(n)
                        if alg == api.MSPACK_DIGEST_MD5:
                            assert bytes(d).hex() == exp["md5"]
    assert n_failed >= 15


def test_params_and_arguments_cpu(built, hostlogic):
    v = [v for v in GD.VECS if "cab_b64" in v and not v["open_err"] and v["files"]][0]
    P, P5 = api.MSCABD_PARAM_HIP_DIGESTS, api.MSCABD_PARAM_HIP_MD5
    with api.Cab(GD.cab_bytes(v), mem=True, L=hostlogic) as c:
        assert c.get_param(P) == (0, 0) and c.get_param(P5) == (0, 0)          # the defaults
        for value in (0, 1, 2, 4, 7, 3, 5, 6):
            assert c.set_param(P, value) == 0 and c.get_param(P) == (0, value)
            assert c.get_param(P5) == (0, value & 1)                          # MSCABD_PARAM_HIP_MD5 reads bit 1 ...
        for value in (8, -1, 15, 255, 1 << 16):
            assert c.set_param(P, value) == api.MSPACK_ERR_ARGS and c.get_param(P) == (0, 6)
        assert c.set_param(P5, 1) == 0 and c.get_param(P) == (0, 7)           # ... and writes it, leaving the others
        assert c.set_param(P5, 0) == 0 and c.get_param(P) == (0, 6)
        assert c.set_param(P5, 2) == api.MSPACK_ERR_ARGS and c.get_param(P) == (0, 6)
        assert c.set_param(P, 1) == 0 and c.get_param(P5) == (0, 1)
        assert c.get_param(999)[0] == api.MSPACK_ERR_ARGS
        # an unknown algorithm, room below the algorithm's length: refused, nothing written
        for alg, cap in ((0, 32), (3, 32), (8, 32), (7, 32), (-1, 32), (api.MSPACK_DIGEST_MD5, 15), (api.MSPACK_DIGEST_SHA1, 19),
                         (api.MSPACK_DIGEST_SHA1, 16), (api.MSPACK_DIGEST_SHA256, 31), (api.MSPACK_DIGEST_SHA256, 20), (api.MSPACK_DIGEST_SHA256, 0)):
            d = (api.C.c_ubyte * 32)(*([0x55] * 32))
            assert c.L.mspack_cabd_digest(c.d, c._files[0], alg, d, cap) == api.MSPACK_ERR_ARGS, (alg, cap)
            assert bytes(d) == b"\x55" * 32 and c.d.contents.last_error(c.d) == api.MSPACK_ERR_ARGS
        d = (api.C.c_ubyte * 32)(*([0x55] * 32))
        assert c.L.mspack_cabd_digest(None, c._files[0], api.MSPACK_DIGEST_SHA1, d, 32) == api.MSPACK_ERR_ARGS and bytes(d) == bytes(20) + b"\x55" * 12
        assert c.L.mspack_cabd_digest(c.d, None, api.MSPACK_DIGEST_SHA256, d, 32) == api.MSPACK_ERR_ARGS and bytes(d) == bytes(32)
        assert c.L.mspack_cabd_digest(c.d, c._files[0], api.MSPACK_DIGEST_SHA256, None, 32) == api.MSPACK_ERR_ARGS
        # more room than needed: the algorithm's bytes, the rest untouched
        b = api.Cab(GD.cab_bytes(v), mem=True, L=hostlogic)
        err_x, data = b.extract(0)
        b.close()
        d = (api.C.c_ubyte * 32)(*([0x55] * 32))
        assert c.L.mspack_cabd_digest(c.d, c._files[0], api.MSPACK_DIGEST_SHA1, d, 32) == err_x == 0
        assert bytes(d) == hashlib.sha1(data).digest() + b"\x55" * 12
        # md5() is digest(MD5)
        assert c.md5(0) == c.digest(0, api.MSPACK_DIGEST_MD5) == (0, hashlib.md5(data).digest())


def test_host_fallback_is_counted_per_algorithm_cpu(built, hostlogic):
    """the stand-in for the batch ABI has no feature word: with every bit on every digest is the host's, and the counters say so per
    algorithm; mspack_cabd_md5_counts is the MD5 pair"""
    for alg in ALGS:
        api.cabd_digest_counts(alg, reset=True, L=hostlogic)
    v = [v for v in GD.VECS if "cab_b64" in v and not v["open_err"] and len(v["files"]) >= 2 and not v["params"].get("salvage")][0]
    with api.Cab(GD.cab_bytes(v), mem=True, L=hostlogic) as c:
        assert c.set_param(api.MSCABD_PARAM_HIP_DIGESTS, 7) == 0
        good = [i for i in range(len(v["files"])) if c.digest(i, api.MSPACK_DIGEST_SHA256)[0] == 0]
        assert good
        assert c.digest(good[0], api.MSPACK_DIGEST_SHA1)[0] == 0
    assert api.cabd_digest_counts(api.MSPACK_DIGEST_SHA256, L=hostlogic) == (0, len(good))
    assert api.cabd_digest_counts(api.MSPACK_DIGEST_SHA1, L=hostlogic) == (0, 1)
    assert api.cabd_digest_counts(api.MSPACK_DIGEST_MD5, L=hostlogic) == api.cabd_md5_counts(L=hostlogic) == (0, 0)
    assert api.cabd_digest_counts(3, L=hostlogic) == (0, 0)


# ---- a file list in descending offset order: the folder's table of kept digests is made from units that arrive descending -----------------
N_DESC, LEN_DESC = 32, 256

_desc = []


def descending_cabinet():
    """one MSZIP folder of 32 files of 256 bytes, the file list in descending offset order -> (cabinet, [the files' bytes in list
    order]).  Equal sizes: every file is 1/32 of the batch's digest bytes, below all three compiled ratios (0.10, 0.05, 0.04)"""
    if not _desc:
        import zlib
        import libmspack_amd as M
        data = M.gen_plaintext(11, 0, N_DESC * LEN_DESC).tobytes()
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        block = b"CK" + co.compress(data) + co.flush()
        offs = [LEN_DESC * i for i in reversed(range(N_DESC))]
        cab = M.cab_write([(1, [block], [len(data)])], [(b"f%02d.bin" % (o // LEN_DESC), LEN_DESC, o, 0) for o in offs])
        _desc.append((cab, [data[o:o + LEN_DESC] for o in offs]))
    return _desc[0]


def digest_descending(L):
    """digest() of every file and every algorithm in list order, against hashlib -> the counts per algorithm"""
    assert 1.0 / N_DESC < 0.04
    cab, want = descending_cabinet()
    for alg in ALGS:
        api.cabd_digest_counts(alg, reset=True, L=L)
    with api.Cab(cab, mem=True, L=L) as c:
        assert [(ln, off) for _n, ln, off, _ct in c.files] == [(LEN_DESC, LEN_DESC * i) for i in reversed(range(N_DESC))]
        assert c.set_param(api.MSCABD_PARAM_HIP_DIGESTS, 7) == 0
        for i in range(N_DESC):
            for alg, h in ALGS.items():
                assert c.digest(i, alg) == (0, h(want[i]).digest()), (i, alg)
        assert not c.mem.outputs
    return [api.cabd_digest_counts(alg, L=L) for alg in ALGS]


def test_descending_file_list_host_fallback_cpu(built, hostlogic):
    assert digest_descending(hostlogic) == [(0, N_DESC)] * 3


@pytest.mark.gpu
def test_descending_file_list_is_answered_from_the_device_gpu(built):
    """all 96 calls are answered from the digests the batch took: the table sorts what the descending list made, and loses none"""
    assert not any(os.environ.get(k) for k in ("MSPACK_HIP_MD5_RATIO", "MSPACK_HIP_SHA1_RATIO", "MSPACK_HIP_SHA256_RATIO"))
    assert digest_descending(None) == [(N_DESC, 0)] * 3
