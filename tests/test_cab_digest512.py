"""mspack_cabd_digest() with MSPACK_DIGEST_SHA384 / _SHA512 and MSCABD_PARAM_HIP_DIGESTS64 (include/mspack.h).  On the CPU stand-in for
the batch ABI the provider has no feature word, so every digest is the host fallback's (the plain-C SHA-384 / SHA-512 of
csrc/host/sha512.c) whatever the param says, and the counters say so.  On the GPU the batch carries a head and two / three
MSPACK_HIP_KIND_DIGEST_MORE tails per file and algorithm and the digests come from the device.  The reference for a digest is
hashlib.sha384 / hashlib.sha512 over what extract() of a second, fresh decompressor wrote; for codes it is that extract()."""
import hashlib
import os
import subprocess
import sys

import pytest

from libmspack_amd import api
import test_cab_md5 as T5
import test_gpu_drivers as GD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGS = {api.MSPACK_DIGEST_SHA384: hashlib.sha384, api.MSPACK_DIGEST_SHA512: hashlib.sha512}
P64, P, P5 = api.MSCABD_PARAM_HIP_DIGESTS64, api.MSCABD_PARAM_HIP_DIGESTS, api.MSCABD_PARAM_HIP_MD5
N_FILES, FILE_BYTES = 256, 2048


def goldens(L, param, vecs):
    """the driver-golden cabinets: digest(f, alg) against extract(f) of a second, fresh decompressor, every file, the two algorithms in
    turn on one decompressor each, in list order and reversed -> (calls that succeeded, calls that failed)"""
    n_ok = n_failed = 0
    for v in vecs:
        if v["open_err"] or not v["files"]:
            continue
        cab, p = GD.cab_bytes(v), v["params"]
        kw = dict(fix_mszip=p.get("fix_mszip", 0), salvage=p.get("salvage", 0), mem=True, L=L)
        for alg, h in ALGS.items():
            for order in T5.orders(len(v["files"]), len(cab))[:2]:
                with api.Cab(cab, **kw) as a, api.Cab(cab, **kw) as b:
                    assert a.set_param(P64, param) == 0
                    for i in order:
                        b.mem.outputs.clear()
                        err_x, data = b.extract(i)
                        a.mem.outputs.clear()
                        err, dg = a.digest(i, alg)
                        want = h(data).digest() if err_x == 0 else bytes(api.DIGEST_BYTES[alg])
                        assert err == err_x and dg == want and len(dg) == api.DIGEST_BYTES[alg], (v["tag"], alg, order, i, err, err_x)
                        assert not a.mem.outputs                              # no output file was opened, nothing written
                        assert a.d.contents.last_error(a.d) == err
                        n_ok += err == 0
                        n_failed += err != 0
    return n_ok, n_failed


@pytest.mark.parametrize("param", [0, 48])
def test_digest_is_extract_with_a_hash_host_fallback_cpu(built, hostlogic, param):
    """every third golden cabinet, stored folders and damaged (failing and partial) ones among them: the code is extract()'s, the digest
    hashlib's over extract()'s bytes or zeros; every successful call is counted as the host's"""
    for alg in ALGS:
        api.cabd_digest_counts(alg, reset=True, L=hostlogic)
    n_ok, n_failed = goldens(hostlogic, param, GD.CPU_VECS[::3])
    assert n_ok >= 20 and n_failed >= 4, (n_ok, n_failed)
    counts = [api.cabd_digest_counts(alg, L=hostlogic) for alg in ALGS]
    assert all(c[0] == 0 for c in counts) and sum(c[1] for c in counts) == n_ok, counts


def test_params_and_arguments_cpu(built, hostlogic):
    v = [v for v in GD.VECS if "cab_b64" in v and not v["open_err"] and v["files"]][0]
    with api.Cab(GD.cab_bytes(v), mem=True, L=hostlogic) as c:
        assert c.get_param(P64) == (0, 0) and c.get_param(P) == (0, 0)          # the defaults
        for value in (0, 16, 32, 48, 16):
            assert c.set_param(P64, value) == 0 and c.get_param(P64) == (0, value)
            assert c.get_param(P) == (0, 0) and c.get_param(P5) == (0, 0)       # the old mask is a parameter of its own
        for value in (1, 2, 4, 7, 8, 15, 17, 24, 40, 49, 63, 64, 255, -1, 1 << 16):
            assert c.set_param(P64, value) == api.MSPACK_ERR_ARGS and c.get_param(P64) == (0, 16), value
        # the old param keeps taking 0 to 7 only
        assert c.set_param(P, 5) == 0
        for value in (8, 15, 16, 32, 48, 255, 1 << 16):
            assert c.set_param(P, value) == api.MSPACK_ERR_ARGS and c.get_param(P) == (0, 5), value
        assert c.get_param(P64) == (0, 16)
        # 8 stays no algorithm; room below the algorithm's length: refused, nothing written
        for alg, cap in ((8, 64), (24, 64), (48, 64), (64, 64), (api.MSPACK_DIGEST_SHA384, 47), (api.MSPACK_DIGEST_SHA384, 32),
                         (api.MSPACK_DIGEST_SHA384, 0), (api.MSPACK_DIGEST_SHA512, 63), (api.MSPACK_DIGEST_SHA512, 48)):
            d = (api.C.c_ubyte * 64)(*([0x55] * 64))
            assert c.L.mspack_cabd_digest(c.d, c._files[0], alg, d, cap) == api.MSPACK_ERR_ARGS, (alg, cap)
            assert bytes(d) == b"\x55" * 64 and c.d.contents.last_error(c.d) == api.MSPACK_ERR_ARGS
        d = (api.C.c_ubyte * 80)(*([0x55] * 80))
        assert c.L.mspack_cabd_digest(c.d, None, api.MSPACK_DIGEST_SHA512, d, 80) == api.MSPACK_ERR_ARGS and bytes(d) == bytes(64) + b"\x55" * 16
        # more room than needed: the algorithm's bytes, the rest untouched
        b = api.Cab(GD.cab_bytes(v), mem=True, L=hostlogic)
        err_x, data = b.extract(0)
        b.close()
        d = (api.C.c_ubyte * 80)(*([0x55] * 80))
        assert c.L.mspack_cabd_digest(c.d, c._files[0], api.MSPACK_DIGEST_SHA384, d, 80) == err_x == 0
        assert bytes(d) == hashlib.sha384(data).digest() + b"\x55" * 32
        assert c.digest(0, api.MSPACK_DIGEST_SHA512) == (0, hashlib.sha512(data).digest())
        assert api.cabd_digest_counts(8, L=hostlogic) == (0, 0) and api.cabd_digest_counts(48, L=hostlogic) == (0, 0)


# ---- on the device ----------------------------------------------------------------------------------------------------------------------

def small_files_cabinet():
    import libmspack_amd as M
    from libmspack_amd import apibench as A
    image, plain = A.build_config2_cab(M, N_FILES, FILE_BYTES)
    return bytes(image), [plain[i * FILE_BYTES:(i + 1) * FILE_BYTES].tobytes() for i in range(N_FILES)]


def digest_all(expect):
    """256 files, both bits on: every digest is hashlib's over extract()'s bytes; the counts are `expect` per algorithm"""
    image, _plain = small_files_cabinet()
    for alg in ALGS:
        api.cabd_digest_counts(alg, reset=True)
    with api.Cab(image, mem=True) as a, api.Cab(image, mem=True) as b:
        assert len(a._files) == N_FILES and a.set_param(P64, 48) == 0
        for i in range(N_FILES):
            b.mem.outputs.clear()
            err_x, data = b.extract(i)
            assert err_x == 0 and len(data) == FILE_BYTES
            for alg, h in ALGS.items():
                assert a.digest(i, alg) == (0, h(data).digest()), (i, alg)
        assert not a.mem.outputs
    assert [api.cabd_digest_counts(alg) for alg in ALGS] == [expect] * 2


@pytest.mark.gpu
def test_256_files_are_hashed_on_the_device_gpu(built):
    assert not os.environ.get("MSPACK_HIP_SHA512_RATIO")
    import libmspack_amd as M
    assert M.features() & M.FEAT_SHA384 and M.features() & M.FEAT_SHA512
    digest_all((N_FILES, 0))
    # with the param off (the default) the same calls are the host's
    image, plain = small_files_cabinet()
    api.cabd_digest_counts(api.MSPACK_DIGEST_SHA512, reset=True)
    with api.Cab(image, mem=True) as c:
        assert c.set_param(P, 7) == 0                                          # (the old mask does not turn the new algorithms on)
        for i in (0, 100, 255):
            assert c.digest(i, api.MSPACK_DIGEST_SHA512) == (0, hashlib.sha512(plain[i]).digest())
    assert api.cabd_digest_counts(api.MSPACK_DIGEST_SHA512) == (0, 3)


@pytest.mark.gpu
def test_ratio_0_leaves_every_file_to_the_host_gpu(built):
    """MSPACK_HIP_SHA512_RATIO=0 (read once per process: a fresh one): no file gets a unit, every digest is the host's, and equal"""
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_cab_digest512 as T; T.digest_all((0, T.N_FILES)); print('RATIO0_OK')" % (
        ROOT, os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MSPACK_HIP_SHA512_RATIO="0"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and b"RATIO0_OK" in p.stdout, p.stdout.decode()[-3000:]


@pytest.mark.gpu
def test_prefetch_of_several_cabinets_takes_the_digests_gpu(built):
    """mspack_cabd_prefetch() reads the param: three cabinets in one batch, every file's digests from the device afterwards"""
    import libmspack_amd as M
    from libmspack_amd import apibench as A
    made = []
    for k in range(3):
        plain = M.gen_plaintext(0x512 + k, 0, 64 * FILE_BYTES)
        image, _p = A.build_config2_cab(M, 64, FILE_BYTES, plain=plain)
        made.append((bytes(image), [plain[i * FILE_BYTES:(i + 1) * FILE_BYTES].tobytes() for i in range(64)]))
    for alg in ALGS:
        api.cabd_digest_counts(alg, reset=True)
    with api.CabSet([m[0] for m in made], mem=True) as s:
        assert s.d.contents.set_param(s.d, P64, 48) == 0
        assert s.prefetch() == 0
        for k, (_img, files) in enumerate(made):
            ptrs = s.file_ptrs(k)
            assert len(ptrs) == 64
            for i, f in enumerate(ptrs):
                for alg, h in ALGS.items():
                    assert s.digest(f, alg) == (0, h(files[i]).digest()), (k, i, alg)
    assert [api.cabd_digest_counts(alg) for alg in ALGS] == [(192, 0)] * 2


@pytest.mark.gpu
def test_failing_calls_give_extracts_code_and_zeros_gpu(built):
    """the damaged golden cabinets with the bits on: the code is extract()'s, the digest bytes are zeros; good files beside them are right"""
    n_ok, n_failed = goldens(None, 48, [v for v in GD.VECS if "mutation" in v][:12])
    assert n_failed >= 6 and n_ok >= 6, (n_ok, n_failed)
