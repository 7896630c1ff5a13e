"""The ABI of the CRC-32 range units (include/mspack_hip.h, libmspack_amd/__init__.py): the new constants with the values the
existing tests leave free, the two conventions stated in the header, no new argument on any entry point, and the unit / result
structs unchanged."""
import os
import re

import numpy as np

import libmspack_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "mspack_hip.h")).read()


def define(name):
    m = re.search(r"^#define\s+%s\s+(\S+)" % name, HDR, re.M)
    assert m, name
    return int(m.group(1).rstrip("u"), 0)


def test_constants():
    assert define("MSPACK_HIP_KIND_CRC32") == 20 == M.KIND_CRC32R
    assert define("MSPACK_HIP_FEAT_CRC32_RANGES") == 64 == M.FEAT_CRC32_RANGES
    assert M.MASK_CRC32R == 1 << 20
    # the values the other tests pin stay what they are: no kind 19, no ninth feature bit in between, the flag's own mask
    assert not re.search(r"^#define\s+MSPACK_HIP_KIND_\w+\s+19\b", HDR, re.M)
    assert define("MSPACK_HIP_KIND_DIGEST_MORE") == 18 and define("MSPACK_HIP_FEAT_LZSS_RING") == 32
    assert define("MSPACK_HIP_MASK_CRC32") == 0x40000000 and define("MSPACK_HIP_UF_CRC32") == 128
    # the feature bits are distinct single bits
    feats = [define(n) for n in re.findall(r"^#define\s+(MSPACK_HIP_FEAT_\w+)", HDR, re.M)]
    assert len(set(feats)) == len(feats) and all(f & (f - 1) == 0 for f in feats)


def test_both_conventions_are_stated():
    text = " ".join(HDR.split())
    assert "INVERTED at the end" in text and "NOT inverted at the end" in text and "zlib.crc32(bytes) ^ 0xFFFFFFFF" in text


def test_no_entry_point_gained_an_argument():
    def n_args(name):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, HDR, re.S)
        assert m, name
        return len([a for a in m.group(1).split(",") if a.strip()])
    assert n_args("mspack_hip_decode_batch_device") == 12 and n_args("mspack_hip_time_batch_device") == 13
    for name in ("mspack_hip_decode_batch", "mspack_hip_decode_batch_begin", "mspack_hip_decode_batch_to_device"):
        assert n_args(name) == 7, name
    assert n_args("mspack_hip_decode_batch_multi") == 8


def test_driver_exports_constants_and_signatures(built):
    """the drivers' new calls are exported with struct-free signatures (pointers and ints only), the params are 105 in both drivers and
    104 stays unused, and the host CRC-32 is exported"""
    import ctypes as C
    import zlib
    from libmspack_amd import api
    M2 = open(os.path.join(ROOT, "include", "mspack.h")).read()
    for name, val in (("MSCABD_PARAM_HIP_CRC32", 105), ("MSCHMD_PARAM_HIP_CRC32", 105)):
        assert re.search(r"^#define\s+%s\s+\(%d\)" % (name, val), M2, re.M), name
    assert api.MSCABD_PARAM_HIP_CRC32 == api.MSCHMD_PARAM_HIP_CRC32 == 105
    assert not re.search(r"^#define\s+MSC\w+_PARAM_\w+\s+\(104\)", M2, re.M)
    assert not re.search(r"^#define\s+MSPACK_DIGEST_\w+\s+\(8\)", M2, re.M)        # no fourth MSPACK_DIGEST_* value
    flat = " ".join(M2.split())
    for proto in ("extern int mspack_cabd_crc32(struct mscab_decompressor *self, struct mscabd_file *file, unsigned int *crc);",
                  "extern int mspack_chmd_crc32(struct mschm_decompressor *self, struct mschmd_file *file, unsigned int *crc);",
                  "extern void mspack_cabd_crc32_counts(unsigned long long counts[2], int reset);",
                  "extern void mspack_chmd_crc32_counts(unsigned long long counts[2], int reset);"):
        assert proto in flat, proto
    L = M.lib()
    for name in ("mspack_cabd_crc32", "mspack_chmd_crc32", "mspack_cabd_crc32_counts", "mspack_chmd_crc32_counts", "mspack_crc32_update"):
        assert hasattr(L, name), name
    L.mspack_crc32_update.restype = C.c_uint32
    L.mspack_crc32_update.argtypes = [C.c_uint32, C.c_char_p, C.c_size_t]
    assert L.mspack_crc32_update(0, b"123456789", 9) == 0xCBF43926 == zlib.crc32(b"123456789")
    assert L.mspack_crc32_update(L.mspack_crc32_update(0, b"1234", 4), b"56789", 5) == 0xCBF43926
    c = (C.c_ulonglong * 2)(7, 7)
    L.mspack_cabd_crc32_counts(c, 0); L.mspack_chmd_crc32_counts(None, 0)
    assert api.crc32_counts().keys() == {"cab", "chm"}


def test_structs_and_helpers():
    assert M.UNIT_DTYPE.itemsize == 48 and M.RESULT_DTYPE.itemsize == 24
    u = M.crc32r_units([(5, 7), (0, 0), (1 << 33, 0xFFFFFFFF)])
    assert (u["kind"] == 20).all() and (u["in_len"] == 0).all() and (u["flags"] == 0).all()
    assert [int(x) for x in u["out_off"]] == [5, 0, 1 << 33] and [int(x) for x in u["out_len"]] == [7, 0, 0xFFFFFFFF]
    assert np.array_equal(u.view(np.uint8)[:48][32:33], np.array([20], dtype=np.uint8))      # `kind` is byte 32 of a unit
