"""ctypes mirror of include/mspack.h (the libmspack-compatible object API served by libmspack_hip.so).

Names and argument meaning follow the reference API (mspack_create_cab_decompressor -> open /
extract / close, mspack_create_chm_decompressor -> open / fast_open / fast_find / extract / close),
so tests read like libmspack/test/cabd_test.c.  File I/O goes through the library's default
stdio mspack_system (sys = NULL), or -- mem=True -- through an in-memory mspack_system handed to
mspack_create_*_decompressor(sys) (MemSystem below: the same semantics as the memory system the goldens
were recorded with, oracle/ref_harness.c: reads are clipped at the end, a seek beyond the end fails)."""
import ctypes as C
import os
import shutil
import tempfile

from . import lib

off_t = C.c_int64


class MscabdFolder(C.Structure):
    pass


class MscabdFile(C.Structure):
    pass


class MscabdCabinet(C.Structure):
    pass


MscabdFolder._fields_ = [("next", C.POINTER(MscabdFolder)), ("comp_type", C.c_int), ("num_blocks", C.c_uint)]
MscabdFile._fields_ = [("next", C.POINTER(MscabdFile)), ("filename", C.c_char_p), ("length", C.c_uint),
                       ("attribs", C.c_int), ("time_h", C.c_char), ("time_m", C.c_char), ("time_s", C.c_char),
                       ("date_d", C.c_char), ("date_m", C.c_char), ("date_y", C.c_int),
                       ("folder", C.POINTER(MscabdFolder)), ("offset", C.c_uint)]
MscabdCabinet._fields_ = [("next", C.POINTER(MscabdCabinet)), ("filename", C.c_char_p), ("base_offset", off_t),
                          ("length", C.c_uint), ("prevcab", C.POINTER(MscabdCabinet)),
                          ("nextcab", C.POINTER(MscabdCabinet)), ("prevname", C.c_char_p), ("nextname", C.c_char_p),
                          ("previnfo", C.c_char_p), ("nextinfo", C.c_char_p), ("files", C.POINTER(MscabdFile)),
                          ("folders", C.POINTER(MscabdFolder)), ("set_id", C.c_ushort), ("set_index", C.c_ushort),
                          ("header_resv", C.c_ushort), ("flags", C.c_int)]


class MscabDecompressor(C.Structure):
    pass


_P = C.POINTER
MscabDecompressor._fields_ = [
    ("open", C.CFUNCTYPE(_P(MscabdCabinet), _P(MscabDecompressor), C.c_char_p)),
    ("close", C.CFUNCTYPE(None, _P(MscabDecompressor), _P(MscabdCabinet))),
    ("search", C.CFUNCTYPE(_P(MscabdCabinet), _P(MscabDecompressor), C.c_char_p)),
    ("append", C.CFUNCTYPE(C.c_int, _P(MscabDecompressor), _P(MscabdCabinet), _P(MscabdCabinet))),
    ("prepend", C.CFUNCTYPE(C.c_int, _P(MscabDecompressor), _P(MscabdCabinet), _P(MscabdCabinet))),
    ("extract", C.CFUNCTYPE(C.c_int, _P(MscabDecompressor), _P(MscabdFile), C.c_char_p)),
    ("set_param", C.CFUNCTYPE(C.c_int, _P(MscabDecompressor), C.c_int, C.c_int)),
    ("last_error", C.CFUNCTYPE(C.c_int, _P(MscabDecompressor))),
]


class MschmdHeader(C.Structure):
    pass


class MschmdFile(C.Structure):
    pass


class MschmdSection(C.Structure):
    _fields_ = [("chm", _P(MschmdHeader)), ("id", C.c_uint)]


class MschmdSecUncompressed(C.Structure):
    _fields_ = [("base", MschmdSection), ("offset", off_t)]


class MschmdSecMscompressed(C.Structure):
    _fields_ = [("base", MschmdSection), ("content", _P(MschmdFile)), ("control", _P(MschmdFile)),
                ("rtable", _P(MschmdFile)), ("spaninfo", _P(MschmdFile))]


MschmdFile._fields_ = [("next", _P(MschmdFile)), ("section", _P(MschmdSection)), ("offset", off_t),
                       ("length", off_t), ("filename", C.c_char_p)]
MschmdHeader._fields_ = [("version", C.c_uint), ("timestamp", C.c_uint), ("language", C.c_uint),
                         ("filename", C.c_char_p), ("length", off_t), ("files", _P(MschmdFile)),
                         ("sysfiles", _P(MschmdFile)), ("sec0", MschmdSecUncompressed),
                         ("sec1", MschmdSecMscompressed), ("dir_offset", off_t), ("num_chunks", C.c_uint),
                         ("chunk_size", C.c_uint), ("density", C.c_uint), ("depth", C.c_uint),
                         ("index_root", C.c_uint), ("first_pmgl", C.c_uint), ("last_pmgl", C.c_uint),
                         ("chunk_cache", C.c_void_p)]


class MschmDecompressor(C.Structure):
    pass


MschmDecompressor._fields_ = [
    ("open", C.CFUNCTYPE(_P(MschmdHeader), _P(MschmDecompressor), C.c_char_p)),
    ("close", C.CFUNCTYPE(None, _P(MschmDecompressor), _P(MschmdHeader))),
    ("extract", C.CFUNCTYPE(C.c_int, _P(MschmDecompressor), _P(MschmdFile), C.c_char_p)),
    ("last_error", C.CFUNCTYPE(C.c_int, _P(MschmDecompressor))),
    ("fast_open", C.CFUNCTYPE(_P(MschmdHeader), _P(MschmDecompressor), C.c_char_p)),
    ("fast_find", C.CFUNCTYPE(C.c_int, _P(MschmDecompressor), _P(MschmdHeader), C.c_char_p, _P(MschmdFile), C.c_int)),
]

MSCABD_PARAM_SEARCHBUF, MSCABD_PARAM_FIXMSZIP, MSCABD_PARAM_DECOMPBUF, MSCABD_PARAM_SALVAGE = 0, 1, 2, 3
MSCABD_PARAM_HIP_DEVICES, MSCABD_PARAM_HIP_CACHE_MB, MSCABD_PARAM_HIP_MD5, MSCABD_PARAM_HIP_DIGESTS = 100, 101, 102, 103
MSCHMD_PARAM_HIP_DIGESTS = 103
MSCABD_PARAM_HIP_DIGESTS64 = MSCHMD_PARAM_HIP_DIGESTS64 = 106      # a mask of MSPACK_DIGEST_SHA384 | MSPACK_DIGEST_SHA512
MSCABD_PARAM_HIP_CRC32, MSCHMD_PARAM_HIP_CRC32 = 105, 105     # 1: the batches carry one CRC-32 range unit per file (104 is no param)
MSCABD_PARAM_HIP_STORED = 107    # 1: stored folders are gathered into the batches and served from them while clean
MSPACK_DIGEST_MD5, MSPACK_DIGEST_SHA1, MSPACK_DIGEST_SHA256 = 1, 2, 4
MSPACK_DIGEST_SHA384, MSPACK_DIGEST_SHA512 = 16, 32                  # (8 is no algorithm)
DIGEST_BYTES = {MSPACK_DIGEST_MD5: 16, MSPACK_DIGEST_SHA1: 20, MSPACK_DIGEST_SHA256: 32, MSPACK_DIGEST_SHA384: 48, MSPACK_DIGEST_SHA512: 64}
MSPACK_ERR_OK, MSPACK_ERR_ARGS = 0, 1


def _setup(L=None):
    """L: an already loaded library exporting the mspack.h API (tests of the host logic pass their CPU
    stand-in build here); default = libmspack_hip.so"""
    if L is None:
        L = lib()
    L.mspack_create_cab_decompressor.restype = _P(MscabDecompressor)
    L.mspack_create_cab_decompressor.argtypes = [C.c_void_p]
    L.mspack_destroy_cab_decompressor.argtypes = [_P(MscabDecompressor)]
    L.mspack_create_chm_decompressor.restype = _P(MschmDecompressor)
    L.mspack_create_chm_decompressor.argtypes = [C.c_void_p]
    L.mspack_destroy_chm_decompressor.argtypes = [_P(MschmDecompressor)]
    L.mspack_cabd_prefetch.restype = C.c_int
    L.mspack_cabd_prefetch.argtypes = [_P(MscabDecompressor), _P(_P(MscabdCabinet)), C.c_int]
    L.mspack_cabd_md5.restype = C.c_int
    L.mspack_cabd_md5.argtypes = [_P(MscabDecompressor), _P(MscabdFile), C.c_void_p]
    L.mspack_cabd_md5_counts.restype = None
    L.mspack_cabd_md5_counts.argtypes = [C.c_void_p, C.c_int]
    L.mspack_cabd_digest.restype = C.c_int
    L.mspack_cabd_digest.argtypes = [_P(MscabDecompressor), _P(MscabdFile), C.c_int, C.c_void_p, C.c_size_t]
    L.mspack_cabd_digest_counts.restype = None
    L.mspack_cabd_digest_counts.argtypes = [C.c_int, C.c_void_p, C.c_int]
    L.mspack_cabd_crc32.restype = C.c_int
    L.mspack_cabd_crc32.argtypes = [_P(MscabDecompressor), _P(MscabdFile), _P(C.c_uint)]
    L.mspack_chmd_crc32.restype = C.c_int
    L.mspack_chmd_crc32.argtypes = [_P(MschmDecompressor), _P(MschmdFile), _P(C.c_uint)]
    for fn in (L.mspack_cabd_crc32_counts, L.mspack_chmd_crc32_counts):
        fn.restype = None
        fn.argtypes = [C.c_void_p, C.c_int]
    L.mspack_cabd_stored_counts.restype = None
    L.mspack_cabd_stored_counts.argtypes = [C.c_void_p, C.c_int]
    L.mspack_cabd_get_param.restype = C.c_int
    L.mspack_cabd_get_param.argtypes = [_P(MscabDecompressor), C.c_int, _P(C.c_int)]
    L.mspack_chmd_digest.restype = C.c_int
    L.mspack_chmd_digest.argtypes = [_P(MschmDecompressor), _P(MschmdFile), C.c_int, C.c_void_p, C.c_size_t]
    L.mspack_chmd_digest_counts.restype = None
    L.mspack_chmd_digest_counts.argtypes = [C.c_int, C.c_void_p, C.c_int]
    L.mspack_chmd_prefetch.restype = C.c_int
    L.mspack_chmd_prefetch.argtypes = [_P(MschmDecompressor), _P(_P(MschmdHeader)), C.c_int]
    L.mspack_chmd_batch_counts.restype = None
    L.mspack_chmd_batch_counts.argtypes = [C.c_void_p, C.c_int]
    L.mspack_chmd_set_param.restype = C.c_int
    L.mspack_chmd_set_param.argtypes = [_P(MschmDecompressor), C.c_int, C.c_int]
    L.mspack_chmd_get_param.restype = C.c_int
    L.mspack_chmd_get_param.argtypes = [_P(MschmDecompressor), C.c_int, _P(C.c_int)]
    L.mspack_version.argtypes = [C.c_int]
    L.mspack_sys_selftest_internal.argtypes = [C.c_int]
    return L


def cabd_md5_counts(reset=False, L=None):
    """mspack_cabd_md5_counts (mspack.h): successful md5() calls of this process answered (from a device digest, by the host's MD5)"""
    c = (C.c_ulonglong * 2)()
    _setup(L).mspack_cabd_md5_counts(c, int(reset))
    return int(c[0]), int(c[1])


def cabd_digest_counts(alg, reset=False, L=None):
    """mspack_cabd_digest_counts (mspack.h): successful digest() calls of algorithm alg answered (from a device digest, by the host)"""
    c = (C.c_ulonglong * 2)()
    _setup(L).mspack_cabd_digest_counts(int(alg), c, int(reset))
    return int(c[0]), int(c[1])


def chmd_digest_counts(alg, reset=False, L=None):
    """mspack_chmd_digest_counts (mspack.h): successful Chm.digest() calls of algorithm alg answered (from a device digest, by the host)"""
    c = (C.c_ulonglong * 2)()
    _setup(L).mspack_chmd_digest_counts(int(alg), c, int(reset))
    return int(c[0]), int(c[1])


def cabd_crc32_counts(reset=False, L=None):
    """mspack_cabd_crc32_counts (mspack.h): successful Cab.crc32() calls answered (from the device, by the host's CRC-32)"""
    c = (C.c_ulonglong * 2)()
    _setup(L).mspack_cabd_crc32_counts(c, int(reset))
    return int(c[0]), int(c[1])


def cabd_stored_counts(reset=False, L=None):
    """mspack_cabd_stored_counts (mspack.h): stored folders (served from a batch, streamed while MSCABD_PARAM_HIP_STORED was 1)"""
    c = (C.c_ulonglong * 2)()
    _setup(L).mspack_cabd_stored_counts(c, int(reset))
    return int(c[0]), int(c[1])


def chmd_crc32_counts(reset=False, L=None):
    """mspack_chmd_crc32_counts (mspack.h): successful Chm.crc32() calls answered (from the device, by the host's CRC-32)"""
    c = (C.c_ulonglong * 2)()
    _setup(L).mspack_chmd_crc32_counts(c, int(reset))
    return int(c[0]), int(c[1])


def crc32_counts(reset=False, L=None):
    """both drivers' crc32 counts -> {"cab": (device, host), "chm": (device, host)}"""
    return {"cab": cabd_crc32_counts(reset, L), "chm": chmd_crc32_counts(reset, L)}


def _crc32(fn, d, fptr):
    v = C.c_uint(0xDEADBEEF)
    err = fn(d, fptr, C.byref(v))
    return err, int(v.value)


def chmd_batch_counts(reset=False, L=None):
    """mspack_chmd_batch_counts (mspack.h): (batch calls the CHM driver has issued in this process, interval units in them)"""
    c = (C.c_ulonglong * 2)()
    _setup(L).mspack_chmd_batch_counts(c, int(reset))
    return int(c[0]), int(c[1])


def _digest(L, d, fptr, alg, cap=None, fn=None):
    n = DIGEST_BYTES.get(alg, 32) if cap is None else cap
    buf = (C.c_ubyte * max(n, 1))()
    err = (fn or L.mspack_cabd_digest)(d, fptr, alg, buf, n)
    return err, bytes(buf)[:n]


def _get_param(L, d, param):
    v = C.c_int(-1)
    err = L.mspack_cabd_get_param(d, param, C.byref(v))
    return err, v.value


class MspackSystem(C.Structure):
    """struct mspack_system (mspack.h:285-455): 10 function pointers + a NULL"""
    _fields_ = [("open", C.c_void_p), ("close", C.c_void_p), ("read", C.c_void_p), ("write", C.c_void_p),
                ("seek", C.c_void_p), ("tell", C.c_void_p), ("message", C.c_void_p), ("alloc", C.c_void_p),
                ("free", C.c_void_p), ("copy", C.c_void_p), ("null_ptr", C.c_void_p)]


class MemSystem:
    """An in-memory mspack_system implemented with ctypes callbacks.  "File names" are keys of
    self.files (bytes -> bytes for inputs); files opened for writing collect into self.outputs.
    alloc / free / copy are the library's own defaults; messages are collected in self.messages."""

    def __init__(self, L):
        self.files = {}
        self.outputs = {}
        self._open = {}
        self._next = 1
        dflt = C.POINTER(MspackSystem).in_dll(L, "mspack_default_system").contents
        OPEN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p, C.c_int)
        CLOSE = C.CFUNCTYPE(None, C.c_void_p)
        RW = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)
        SEEK = C.CFUNCTYPE(C.c_int, C.c_void_p, off_t, C.c_int)
        TELL = C.CFUNCTYPE(off_t, C.c_void_p)

        def m_open(_self, name, mode):
            if mode == 0:
                if name not in self.files:
                    return None
                f = dict(data=self.files[name], pos=0, w=None)
            else:
                self.outputs[name] = bytearray()
                f = dict(data=None, pos=0, w=self.outputs[name])
            h = self._next; self._next += 1
            self._open[h] = f
            return h

        def m_close(h):
            self._open.pop(h, None)

        def m_read(h, buf, n):
            f = self._open.get(h)
            if f is None or f["w"] is not None or n < 0:
                return -1
            d = f["data"]
            n = min(n, len(d) - f["pos"])
            if n > 0:
                C.memmove(buf, d[f["pos"]:f["pos"] + n], n)
                f["pos"] += n
            return max(n, 0)

        def m_write(h, buf, n):
            f = self._open.get(h)
            if f is None or f["w"] is None or n < 0:
                return -1
            f["w"] += C.string_at(buf, n)
            return n

        def m_seek(h, off, mode):
            f = self._open.get(h)
            if f is None or f["data"] is None:
                return -1
            base = (0, f["pos"], len(f["data"]))[mode] if 0 <= mode <= 2 else None
            if base is None or base + off < 0 or base + off > len(f["data"]):
                return -1
            f["pos"] = base + off
            return 0

        def m_tell(h):
            f = self._open.get(h)
            return f["pos"] if f else 0

        def m_message(_h, fmt):           # variadic in C; the extra arguments are simply not looked at
            self.messages.append(fmt)
            self.message_handles.append(bool(_h))      # (the reference passes the cabinet's handle with some lines, NULL with others)

        self.messages = []
        self.message_handles = []
        MSG = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
        self._cbs = [OPEN(m_open), CLOSE(m_close), RW(m_read), RW(m_write), SEEK(m_seek), TELL(m_tell), MSG(m_message)]
        vp = [C.cast(cb, C.c_void_p).value for cb in self._cbs]
        self.sys = MspackSystem(vp[0], vp[1], vp[2], vp[3], vp[4], vp[5], vp[6], dflt.alloc, dflt.free,
                                dflt.copy, None)

    def ptr(self):
        return C.addressof(self.sys)


def _walk(ptr):
    while ptr:
        yield ptr
        ptr = ptr.contents.next


class Cab:
    """with Cab(path_or_bytes) as cab: cab.files -> [(name, length, offset, comp_type)];
    cab.extract(i) -> (err, bytes)"""

    def __init__(self, src, fix_mszip=0, salvage=0, mem=False, L=None):
        self.L = _setup(L)
        self._tmp = None
        self.mem = None
        if mem:
            self.mem = MemSystem(self.L)
            self.mem.files[b"mem:in"] = bytes(src)
            self.path = b"mem:in"
        else:
            if isinstance(src, (bytes, bytearray)):
                fd, self._tmp = tempfile.mkstemp(suffix=".cab")
                os.write(fd, src); os.close(fd)
                src = self._tmp
            self.path = os.fsencode(src)
        self.d = self.L.mspack_create_cab_decompressor(self.mem.ptr() if self.mem else None)
        if not self.d:
            raise RuntimeError("mspack_create_cab_decompressor failed")
        self.d.contents.set_param(self.d, MSCABD_PARAM_FIXMSZIP, fix_mszip)
        self.d.contents.set_param(self.d, MSCABD_PARAM_SALVAGE, salvage)
        self.cab = self.d.contents.open(self.d, self.path)
        self.open_error = self.d.contents.last_error(self.d)
        self._files = list(_walk(self.cab.contents.files)) if self.cab else []

    @property
    def files(self):
        return [(f.contents.filename, f.contents.length, f.contents.offset,
                 f.contents.folder.contents.comp_type if f.contents.folder else -1) for f in self._files]

    def extract(self, i):
        if self.mem:
            err = self.d.contents.extract(self.d, self._files[i], b"mem:out")
            return err, bytes(self.mem.outputs.get(b"mem:out", b""))
        fd, out = tempfile.mkstemp(suffix=".out")
        os.close(fd)
        try:
            err = self.d.contents.extract(self.d, self._files[i], os.fsencode(out))
            with open(out, "rb") as fh:
                return err, fh.read()
        finally:
            os.unlink(out)

    def set_param(self, param, value):
        return self.d.contents.set_param(self.d, param, value)

    def md5(self, i):
        """mspack_cabd_md5 (mspack.h): extract(i) with the writes replaced by a hash -> (err, the sixteen digest bytes; zeros unless
        err == 0).  set_param(MSCABD_PARAM_HIP_MD5, 1) before the first call lets the batch take the digests on the device"""
        d = (C.c_ubyte * 16)()
        err = self.L.mspack_cabd_md5(self.d, self._files[i], d)
        return err, bytes(d)

    def get_param(self, param):
        """mspack_cabd_get_param (mspack.h) -> (err, value)"""
        return _get_param(self.L, self.d, param)

    def crc32(self, i):
        """mspack_cabd_crc32 (mspack.h): extract(i) with the writes replaced by zlib's CRC-32 -> (err, value; 0 unless err == 0).
        set_param(MSCABD_PARAM_HIP_CRC32, 1) before the first call lets the batch take the checksums on the device, at any length"""
        return _crc32(self.L.mspack_cabd_crc32, self.d, self._files[i])

    def digest(self, i, alg, cap=None):
        """mspack_cabd_digest (mspack.h): extract(i) with the writes replaced by a hash of algorithm alg (MSPACK_DIGEST_*) -> (err, the
        16 / 20 / 32 / 48 / 64 digest bytes; zeros unless err == 0).  set_param(MSCABD_PARAM_HIP_DIGESTS, mask) before the first call lets the
        batch take the digests on the device.  cap: the digest_cap handed over instead of the algorithm's length"""
        return _digest(self.L, self.d, self._files[i], alg, cap)

    def close(self):
        if self.cab:
            self.d.contents.close(self.d, self.cab); self.cab = None
        if self.d:
            self.L.mspack_destroy_cab_decompressor(self.d); self.d = None
        if self._tmp:
            os.unlink(self._tmp); self._tmp = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()



MSCABD_PARAM_SEARCHBUF = 0


class CabSet:
    """Several cabinets on ONE decompressor, joined with append()/prepend() like cabextract does
    (reference cabd.c:870-1064):  with CabSet([p1, p2, ...]) as s: s.append(0, 1); s.files(0); s.extract(f)"""

    def __init__(self, srcs, fix_mszip=0, salvage=0, mem=False, L=None):
        self.L = _setup(L)
        self._tmps = []
        self.paths = []
        self.mem = MemSystem(self.L) if mem else None          # (mem=True: srcs are bytes, kept in an in-memory mspack_system)
        for k, src in enumerate(srcs):
            if self.mem:
                self.mem.files[b"mem:in%d" % k] = bytes(src)
                self.paths.append(b"mem:in%d" % k)
                continue
            if isinstance(src, (bytes, bytearray)):
                fd, tmp = tempfile.mkstemp(suffix=".cab")
                os.write(fd, src); os.close(fd)
                self._tmps.append(tmp)
                src = tmp
            self.paths.append(os.fsencode(src))           # must outlive the cabinets (mspack.h:968-969)
        self.d = self.L.mspack_create_cab_decompressor(self.mem.ptr() if self.mem else None)
        if not self.d:
            raise RuntimeError("mspack_create_cab_decompressor failed")
        self.d.contents.set_param(self.d, MSCABD_PARAM_FIXMSZIP, fix_mszip)
        self.d.contents.set_param(self.d, MSCABD_PARAM_SALVAGE, salvage)
        self.cabs, self.open_errors = [], []
        for p in self.paths:
            c = self.d.contents.open(self.d, p)
            self.cabs.append(c)
            self.open_errors.append(0 if c else self.d.contents.last_error(self.d))      # (last_error() is the LAST call's)

    def _cab(self, i):
        return self.cabs[i] if i is not None and i >= 0 else None

    def append(self, a, b):
        return self.d.contents.append(self.d, self._cab(a), self._cab(b))

    def prepend(self, a, b):
        return self.d.contents.prepend(self.d, self._cab(a), self._cab(b))

    def prefetch(self, indices=None):
        """mspack_cabd_prefetch (mspack.h): the not-yet-decoded folders of these cabinets (indices into the list given to the
        constructor; None = all that opened) in ONE batch; the extract() calls that follow are slices of it -> MSPACK_ERR_*"""
        if indices is None:
            indices = [i for i, c in enumerate(self.cabs) if c]
        arr = (_P(MscabdCabinet) * max(len(indices), 1))(*[self.cabs[i] for i in indices])
        return self.L.mspack_cabd_prefetch(self.d, arr, len(indices))

    def file_ptrs(self, i):
        return list(_walk(self.cabs[i].contents.files))

    def files(self, i):
        """[(name, length, offset, comp_type, folder ordinal, folder num_blocks)] of cabinet i's list"""
        folders = [C.addressof(f.contents) for f in _walk(self.cabs[i].contents.folders)]
        out = []
        for f in self.file_ptrs(i):
            fo = f.contents.folder
            out.append((f.contents.filename, f.contents.length, f.contents.offset,
                        fo.contents.comp_type if fo else -1,
                        folders.index(C.addressof(fo.contents)) if fo else -1,
                        fo.contents.num_blocks if fo else 0))
        return out

    def set_param(self, param, value):
        return self.d.contents.set_param(self.d, param, value)

    def md5(self, fptr):
        """mspack_cabd_md5 (mspack.h) of a file of file_ptrs() -> (err, the sixteen digest bytes)"""
        d = (C.c_ubyte * 16)()
        err = self.L.mspack_cabd_md5(self.d, fptr, d)
        return err, bytes(d)

    def digest(self, fptr, alg, cap=None):
        """mspack_cabd_digest (mspack.h) of a file of file_ptrs() -> (err, the digest bytes)"""
        return _digest(self.L, self.d, fptr, alg, cap)

    def crc32(self, fptr):
        """mspack_cabd_crc32 (mspack.h) of a file of file_ptrs() -> (err, value)"""
        return _crc32(self.L.mspack_cabd_crc32, self.d, fptr)

    def extract(self, fptr):
        if self.mem:
            self.mem.outputs.clear()
            err = self.d.contents.extract(self.d, fptr, b"mem:out")
            return err, bytes(self.mem.outputs.get(b"mem:out", b""))
        fd, out = tempfile.mkstemp(suffix=".out")
        os.close(fd)
        try:
            err = self.d.contents.extract(self.d, fptr, os.fsencode(out))
            with open(out, "rb") as fh:
                return err, fh.read()
        finally:
            os.unlink(out)

    def close(self):
        if self.d:
            # joined cabinets are freed with the one they are joined to: close one per chain
            seen = set()
            for c in self.cabs:
                if not c:
                    continue
                chain = set()
                w = c
                while w:
                    chain.add(C.addressof(w.contents)); w = w.contents.prevcab
                w = c
                while w:
                    chain.add(C.addressof(w.contents)); w = w.contents.nextcab
                if chain & seen:
                    continue
                seen |= chain
                self.d.contents.close(self.d, c)
            self.cabs = []
            self.L.mspack_destroy_cab_decompressor(self.d); self.d = None
        for t in self._tmps:
            os.unlink(t)
        self._tmps = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def cab_search(src, searchbuf=0):
    """search(): [(base_offset, n_files, first file name)] of the cabinets found inside a file"""
    L = _setup()
    tmp = None
    if isinstance(src, (bytes, bytearray)):
        fd, tmp = tempfile.mkstemp(suffix=".bin")
        os.write(fd, src); os.close(fd)
        src = tmp
    path = os.fsencode(src)
    d = L.mspack_create_cab_decompressor(None)
    try:
        if searchbuf:
            d.contents.set_param(d, MSCABD_PARAM_SEARCHBUF, searchbuf)
        head = d.contents.search(d, path)
        err = d.contents.last_error(d)
        found = []
        for c in _walk(head):
            fl = list(_walk(c.contents.files))
            found.append((c.contents.base_offset, len(fl), fl[0].contents.filename if fl else b""))
        if head:
            d.contents.close(d, head)
        return err, found
    finally:
        L.mspack_destroy_cab_decompressor(d)
        if tmp:
            os.unlink(tmp)


class Chm:
    def __init__(self, src, fast=False, mem=False, L=None):
        self.L = _setup(L)
        self._tmp = None
        self.mem = None
        if mem:
            self.mem = MemSystem(self.L)
            self.mem.files[b"mem:in"] = bytes(src)
            self.path = b"mem:in"
        else:
            if isinstance(src, (bytes, bytearray)):
                fd, self._tmp = tempfile.mkstemp(suffix=".chm")
                os.write(fd, src); os.close(fd)
                src = self._tmp
            self.path = os.fsencode(src)
        self.d = self.L.mspack_create_chm_decompressor(self.mem.ptr() if self.mem else None)
        m = self.d.contents
        self.chm = (m.fast_open if fast else m.open)(self.d, self.path)
        self.open_error = m.last_error(self.d)
        self._files = list(_walk(self.chm.contents.files)) if self.chm else []

    @property
    def files(self):
        return [(f.contents.filename, f.contents.length, f.contents.offset, f.contents.section.contents.id)
                for f in self._files]

    def _extract_ptr(self, fptr):
        if self.mem:
            err = self.d.contents.extract(self.d, fptr, b"mem:out")
            return err, bytes(self.mem.outputs.get(b"mem:out", b""))
        fd, out = tempfile.mkstemp(suffix=".out")
        os.close(fd)
        try:
            err = self.d.contents.extract(self.d, fptr, os.fsencode(out))
            with open(out, "rb") as fh:
                return err, fh.read()
        finally:
            os.unlink(out)

    def extract(self, i):
        return self._extract_ptr(self._files[i])

    def set_param(self, param, value):
        """mspack_chmd_set_param (mspack.h)"""
        return self.L.mspack_chmd_set_param(self.d, param, value)

    def get_param(self, param):
        """mspack_chmd_get_param (mspack.h) -> (err, value)"""
        v = C.c_int(-1)
        err = self.L.mspack_chmd_get_param(self.d, param, C.byref(v))
        return err, v.value

    def digest(self, i, alg, cap=None):
        """mspack_chmd_digest (mspack.h): extract(i) with the writes replaced by a hash of algorithm alg (MSPACK_DIGEST_*) -> (err, the
        16 / 20 / 32 / 48 / 64 digest bytes; zeros unless err == 0).  set_param(MSCHMD_PARAM_HIP_DIGESTS, mask) before the first call lets the
        chunks' batches take the digests on the device.  cap: the digest_cap handed over instead of the algorithm's length"""
        return _digest(self.L, self.d, self._files[i], alg, cap, fn=self.L.mspack_chmd_digest)

    def crc32(self, i):
        """mspack_chmd_crc32 (mspack.h): extract(i) with the writes replaced by zlib's CRC-32 -> (err, value; 0 unless err == 0).
        set_param(MSCHMD_PARAM_HIP_CRC32, 1) before the first call lets the chunks' batches take the checksums on the device"""
        return _crc32(self.L.mspack_chmd_crc32, self.d, self._files[i])

    def find(self, name):
        f = MschmdFile()
        err = self.d.contents.fast_find(self.d, self.chm, name, C.byref(f), C.sizeof(MschmdFile))
        return err, (f if f.section else None)

    def extract_found(self, f):
        return self._extract_ptr(C.pointer(f))

    def close(self):
        if self.chm:
            self.d.contents.close(self.d, self.chm); self.chm = None
        if self.d:
            self.L.mspack_destroy_chm_decompressor(self.d); self.d = None
        if self._tmp:
            os.unlink(self._tmp); self._tmp = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class ChmSet:
    """Many CHM images opened on ONE decompressor and one in-memory mspack_system:
    with ChmSet([blob1, blob2, ...]) as s: s.prefetch(); s.files(k); s.extract(k, i); s.digest(k, i, alg)"""

    def __init__(self, blobs, L=None, fast=False):
        self.L = _setup(L)
        self.mem = MemSystem(self.L)
        self.paths = []
        for k, blob in enumerate(blobs):
            self.mem.files[b"mem:in%d" % k] = bytes(blob)
            self.paths.append(b"mem:in%d" % k)                # must outlive the CHMs: the driver keeps the pointer
        self.d = self.L.mspack_create_chm_decompressor(self.mem.ptr())
        if not self.d:
            raise RuntimeError("mspack_create_chm_decompressor failed")
        m = self.d.contents
        self.chms, self.open_errors, self._files = [], [], []
        for p in self.paths:
            c = (m.fast_open if fast else m.open)(self.d, p)
            self.chms.append(c)
            self.open_errors.append(0 if c else m.last_error(self.d))
            self._files.append(list(_walk(c.contents.files)) if c else [])

    @property
    def messages(self):
        return self.mem.messages

    def last_error(self):
        return self.d.contents.last_error(self.d)

    def set_param(self, param, value):
        return self.L.mspack_chmd_set_param(self.d, param, value)

    def prefetch(self, indices=None):
        """mspack_chmd_prefetch (mspack.h): the not-yet-decoded reset intervals of these CHMs (indices into the list given to the
        constructor; None = all that are open) in ONE batch -> MSPACK_ERR_*"""
        if indices is None:
            indices = [k for k, c in enumerate(self.chms) if c]
        arr = (_P(MschmdHeader) * max(len(indices), 1))(*[self.chms[k] for k in indices])
        return self.L.mspack_chmd_prefetch(self.d, arr, len(indices))

    def files(self, k):
        """[(name, length, offset, section)] of CHM k's list"""
        return [(f.contents.filename, f.contents.length, f.contents.offset, f.contents.section.contents.id) for f in self._files[k]]

    def extract(self, k, i):
        self.mem.outputs.clear()
        err = self.d.contents.extract(self.d, self._files[k][i], b"mem:out")
        return err, bytes(self.mem.outputs.get(b"mem:out", b""))

    def find(self, k, name):
        f = MschmdFile()
        err = self.d.contents.fast_find(self.d, self.chms[k], name, C.byref(f), C.sizeof(MschmdFile))
        return err, (f if f.section else None)

    def extract_found(self, f):
        self.mem.outputs.clear()
        err = self.d.contents.extract(self.d, C.pointer(f), b"mem:out")
        return err, bytes(self.mem.outputs.get(b"mem:out", b""))

    def digest(self, k, i, alg, cap=None):
        """mspack_chmd_digest (mspack.h) of file i of CHM k -> (err, the digest bytes)"""
        return _digest(self.L, self.d, self._files[k][i], alg, cap, fn=self.L.mspack_chmd_digest)

    def crc32(self, k, i):
        """mspack_chmd_crc32 (mspack.h) of file i of CHM k -> (err, value)"""
        return _crc32(self.L.mspack_chmd_crc32, self.d, self._files[k][i])

    def close(self, k=None):
        """close(k): CHM k alone; close(): every CHM that is still open, then the decompressor"""
        if k is not None:
            if self.d and self.chms[k]:
                self.d.contents.close(self.d, self.chms[k])
                self.chms[k] = None; self._files[k] = []
            return
        if self.d:
            for j, c in enumerate(self.chms):
                if c:
                    self.d.contents.close(self.d, c)
                    self.chms[j] = None; self._files[j] = []
            self.L.mspack_destroy_chm_decompressor(self.d); self.d = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class MsoabDecompressor(C.Structure):
    pass


MsoabDecompressor._fields_ = [
    ("decompress", C.CFUNCTYPE(C.c_int, _P(MsoabDecompressor), C.c_char_p, C.c_char_p)),
    ("decompress_incremental", C.CFUNCTYPE(C.c_int, _P(MsoabDecompressor), C.c_char_p, C.c_char_p, C.c_char_p)),
    ("set_param", C.CFUNCTYPE(C.c_int, _P(MsoabDecompressor), C.c_int, C.c_int)),
]


def oab_decompress(blob, base=None, decompbuf=0, L=None):
    """mspack_create_oab_decompressor -> decompress / decompress_incremental over temporary files
    -> (err, output bytes).  L: as in _setup (the CPU stand-in build of the host logic: tests)"""
    L = L or lib()
    L.mspack_create_oab_decompressor.restype = _P(MsoabDecompressor)
    L.mspack_create_oab_decompressor.argtypes = [C.c_void_p]
    L.mspack_destroy_oab_decompressor.argtypes = [_P(MsoabDecompressor)]
    tmps = []

    def tmp(data):
        fd, path = tempfile.mkstemp(suffix=".oab")
        os.write(fd, data); os.close(fd)
        tmps.append(path)
        return os.fsencode(path)
    d = L.mspack_create_oab_decompressor(None)
    try:
        if decompbuf:
            d.contents.set_param(d, 0, decompbuf)
        pin, pout = tmp(bytes(blob)), tmp(b"")
        if base is None:
            err = d.contents.decompress(d, pin, pout)
        else:
            err = d.contents.decompress_incremental(d, pin, tmp(bytes(base)), pout)
        with open(os.fsdecode(pout), "rb") as fh:
            return err, fh.read()
    finally:
        L.mspack_destroy_oab_decompressor(d)
        for t in tmps:
            os.unlink(t)


class MsoabdJob(C.Structure):
    _fields_ = [("input", C.c_char_p), ("base", C.c_char_p), ("output", C.c_char_p), ("error", C.c_int)]


def _setup_oab(L=None):
    """argument types of the OAB driver and its extensions (mspack.h); L as in _setup"""
    L = L or lib()
    L.mspack_create_oab_decompressor.restype = _P(MsoabDecompressor)
    L.mspack_create_oab_decompressor.argtypes = [C.c_void_p]
    L.mspack_destroy_oab_decompressor.argtypes = [_P(MsoabDecompressor)]
    L.mspack_oabd_decompress_many.restype = C.c_int
    L.mspack_oabd_decompress_many.argtypes = [_P(MsoabDecompressor), _P(MsoabdJob), C.c_int]
    L.mspack_oabd_batch_counts.restype = None
    L.mspack_oabd_batch_counts.argtypes = [C.c_void_p, C.c_int]
    return L


def oab_batch_counts(reset=False, L=None):
    """mspack_oabd_batch_counts (mspack.h): (batch calls the OAB driver has issued in this process, jobs that went out in a batch of
    mspack_oabd_decompress_many, jobs decoded again alone because their shared batch failed)"""
    c = (C.c_ulonglong * 3)()
    _setup_oab(L).mspack_oabd_batch_counts(c, int(reset))
    return int(c[0]), int(c[1]), int(c[2])


def oab_decompress_paths(jobs, decompbuf=0, L=None, sys=None):
    """mspack_oabd_decompress_many over files that exist: jobs = [(input, base or None, output)] (bytes names; a None input or output
    goes through as NULL) -> (the call's return value, [jobs[k].error]).  sys: a MemSystem, else the library's stdio system"""
    L = _setup_oab(L)
    d = L.mspack_create_oab_decompressor(sys.ptr() if sys is not None else None)
    try:
        if decompbuf:
            d.contents.set_param(d, 0, decompbuf)
        arr = (MsoabdJob * max(len(jobs), 1))()
        for k, (pin, pbase, pout) in enumerate(jobs):
            arr[k].input, arr[k].base, arr[k].output, arr[k].error = pin, pbase, pout, -1
        rc = L.mspack_oabd_decompress_many(d, arr, len(jobs))
        return rc, [int(arr[k].error) for k in range(len(jobs))]
    finally:
        L.mspack_destroy_oab_decompressor(d)


def oab_decompress_many(items, decompbuf=0, L=None):
    """mspack_oabd_decompress_many over temporary files: items = [(blob, base or None)] -> [(err, output bytes)], one call for all of
    them.  L: as in _setup (the CPU stand-in build of the host logic: tests)"""
    tmpdir = tempfile.mkdtemp(prefix="oab_many_")

    def tmp(name, data):
        path = os.path.join(tmpdir, name)
        with open(path, "wb") as fh:
            fh.write(bytes(data))
        return os.fsencode(path)
    try:
        jobs = [(tmp("%d.oab" % k, blob), None if base is None else tmp("%d.base" % k, base),
                 os.fsencode(os.path.join(tmpdir, "%d.out" % k))) for k, (blob, base) in enumerate(items)]
        rc, errs = oab_decompress_paths(jobs, decompbuf, L)
        if rc:
            raise RuntimeError("mspack_oabd_decompress_many: error %d" % rc)
        out = []
        for (_i, _b, pout), err in zip(jobs, errs):
            # (a job that fails before its output is opened creates none: the lone call's temporary file is then as empty)
            data = b""
            if os.path.exists(pout):
                with open(pout, "rb") as fh:
                    data = fh.read()
            out.append((err, data))
        return out
    finally:
        shutil.rmtree(tmpdir, ignore_errors=True)


class MsszdddHeader(C.Structure):
    _fields_ = [("format", C.c_int), ("length", off_t), ("missing_char", C.c_char)]


class MsszddDecompressor(C.Structure):
    pass


MsszddDecompressor._fields_ = [
    ("open", C.CFUNCTYPE(_P(MsszdddHeader), _P(MsszddDecompressor), C.c_char_p)),
    ("close", C.CFUNCTYPE(None, _P(MsszddDecompressor), _P(MsszdddHeader))),
    ("extract", C.CFUNCTYPE(C.c_int, _P(MsszddDecompressor), _P(MsszdddHeader), C.c_char_p)),
    ("decompress", C.CFUNCTYPE(C.c_int, _P(MsszddDecompressor), C.c_char_p, C.c_char_p)),
    ("last_error", C.CFUNCTYPE(C.c_int, _P(MsszddDecompressor))),
]


class MskwajdHeader(C.Structure):
    _fields_ = [("comp_type", C.c_ushort), ("data_offset", off_t), ("headers", C.c_int), ("length", off_t),
                ("filename", C.c_char_p), ("extra", C.c_char_p), ("extra_length", C.c_ushort)]


class MskwajDecompressor(C.Structure):
    pass


MskwajDecompressor._fields_ = [
    ("open", C.CFUNCTYPE(_P(MskwajdHeader), _P(MskwajDecompressor), C.c_char_p)),
    ("close", C.CFUNCTYPE(None, _P(MskwajDecompressor), _P(MskwajdHeader))),
    ("extract", C.CFUNCTYPE(C.c_int, _P(MskwajDecompressor), _P(MskwajdHeader), C.c_char_p)),
    ("decompress", C.CFUNCTYPE(C.c_int, _P(MskwajDecompressor), C.c_char_p, C.c_char_p)),
    ("last_error", C.CFUNCTYPE(C.c_int, _P(MskwajDecompressor))),
]


def szdd_kwaj_extract(kind, blob, L=None):
    """kind 0 = SZDD, 1 = KWAJ: open() + extract() over temporary files
    -> dict(open_err, err, data, comp_type (SZDD: format), length, filename (SZDD: the missing character)).
    L: as in _setup (the CPU stand-in build of the host logic: tests)"""
    L = L or lib()
    T = MsszddDecompressor if kind == 0 else MskwajDecompressor
    create = L.mspack_create_szdd_decompressor if kind == 0 else L.mspack_create_kwaj_decompressor
    destroy = L.mspack_destroy_szdd_decompressor if kind == 0 else L.mspack_destroy_kwaj_decompressor
    create.restype = _P(T); create.argtypes = [C.c_void_p]; destroy.argtypes = [_P(T)]
    fd, pin = tempfile.mkstemp(suffix=".in"); os.write(fd, bytes(blob)); os.close(fd)
    fd, pout = tempfile.mkstemp(suffix=".out"); os.close(fd)
    d = create(None)
    try:
        h = d.contents.open(d, os.fsencode(pin))
        if not h:
            e = d.contents.last_error(d)
            return dict(open_err=e, err=e, data=b"", comp_type=-1, length=-1, filename=b"")
        hc = h.contents
        info = dict(open_err=0, comp_type=hc.format if kind == 0 else hc.comp_type, length=hc.length,
                    filename=(hc.missing_char.rstrip(b"\0") if kind == 0 else (hc.filename or b"")))
        info["err"] = d.contents.extract(d, h, os.fsencode(pout))
        d.contents.close(d, h)
        with open(pout, "rb") as fh:
            info["data"] = fh.read()
        return info
    finally:
        destroy(d)
        os.unlink(pin); os.unlink(pout)


def _setup_sk(L=None):
    """argument types of the SZDD / KWAJ extensions (mspack.h); L as in _setup"""
    L = L or lib()
    for T, name in ((MsszddDecompressor, "szdd"), (MskwajDecompressor, "kwaj")):
        create, destroy = getattr(L, "mspack_create_%s_decompressor" % name), getattr(L, "mspack_destroy_%s_decompressor" % name)
        create.restype = _P(T); create.argtypes = [C.c_void_p]; destroy.argtypes = [_P(T)]
    L.mspack_szddd_prefetch.restype = C.c_int
    L.mspack_szddd_prefetch.argtypes = [_P(MsszddDecompressor), _P(_P(MsszdddHeader)), C.c_int]
    L.mspack_kwajd_prefetch.restype = C.c_int
    L.mspack_kwajd_prefetch.argtypes = [_P(MskwajDecompressor), _P(_P(MskwajdHeader)), C.c_int]
    for f in (L.mspack_szddd_batch_counts, L.mspack_kwajd_batch_counts):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_int]
    L.mspack_szdd_kwaj_ring_units.restype = C.c_ulonglong
    L.mspack_szdd_kwaj_ring_units.argtypes = [C.c_int]
    return L


def szdd_batch_counts(reset=False, L=None):
    """mspack_szddd_batch_counts (mspack.h): (batches the SZDD driver issued, extract() calls answered from a prefetch batch, members
    decoded again alone because they did not fit their room)"""
    c = (C.c_ulonglong * 3)()
    _setup_sk(L).mspack_szddd_batch_counts(c, int(reset))
    return int(c[0]), int(c[1]), int(c[2])


def kwaj_batch_counts(reset=False, L=None):
    """mspack_kwajd_batch_counts (mspack.h): as szdd_batch_counts, of the KWAJ driver"""
    c = (C.c_ulonglong * 3)()
    _setup_sk(L).mspack_kwajd_batch_counts(c, int(reset))
    return int(c[0]), int(c[1]), int(c[2])


def lzss_ring_units(reset=False, L=None):
    """mspack_szdd_kwaj_ring_units (mspack.h): LZSS members of the two drivers' prefetch batches that went out with UF_LZSS_RING"""
    return int(_setup_sk(L).mspack_szdd_kwaj_ring_units(int(reset)))


class _SkSet:
    """Many SZDD (or KWAJ) images opened on ONE decompressor and one in-memory mspack_system:
    with SzddSet([blob1, blob2, ...]) as s: s.prefetch(); s.extract(k)"""
    KIND = 0

    def __init__(self, blobs, L=None):
        self.L = _setup_sk(L)
        self.mem = MemSystem(self.L)
        self.paths = []
        for k, blob in enumerate(blobs):
            self.mem.files[b"mem:in%d" % k] = bytes(blob)
            self.paths.append(b"mem:in%d" % k)
        create = self.L.mspack_create_szdd_decompressor if self.KIND == 0 else self.L.mspack_create_kwaj_decompressor
        self.d = create(self.mem.ptr())
        if not self.d:
            raise RuntimeError("the decompressor could not be created")
        m = self.d.contents
        self.hdrs, self.open_errors = [], []
        for p in self.paths:
            h = m.open(self.d, p)
            self.hdrs.append(h if h else None)
            self.open_errors.append(0 if h else m.last_error(self.d))

    @property
    def messages(self):
        return self.mem.messages

    def last_error(self):
        return self.d.contents.last_error(self.d)

    def prefetch(self, indices=None):
        """mspack_szddd_prefetch / mspack_kwajd_prefetch (mspack.h): the coded streams of these files (indices into the list given
        to the constructor, None entries allowed; None = all that are open) in ONE batch -> MSPACK_ERR_*"""
        if indices is None:
            indices = [k for k, h in enumerate(self.hdrs) if h]
        H = MsszdddHeader if self.KIND == 0 else MskwajdHeader
        arr = (_P(H) * max(len(indices), 1))()
        for j, k in enumerate(indices):
            if k is not None and self.hdrs[k]:
                arr[j] = self.hdrs[k]
        fn = self.L.mspack_szddd_prefetch if self.KIND == 0 else self.L.mspack_kwajd_prefetch
        return fn(self.d, arr, len(indices))

    def extract(self, k):
        """-> the dict of szdd_kwaj_extract for file k"""
        h = self.hdrs[k]
        if not h:
            e = self.open_errors[k]
            return dict(open_err=e, err=e, data=b"", comp_type=-1, length=-1, filename=b"")
        hc = h.contents
        info = dict(open_err=0, comp_type=hc.format if self.KIND == 0 else hc.comp_type, length=hc.length,
                    filename=(hc.missing_char.rstrip(b"\0") if self.KIND == 0 else (hc.filename or b"")))
        self.mem.outputs.clear()
        info["err"] = self.d.contents.extract(self.d, h, b"mem:out")
        info["data"] = bytes(self.mem.outputs.get(b"mem:out", b""))
        return info

    def close(self, k=None):
        """close(k): file k alone; close(): every file that is still open, then the decompressor"""
        if k is not None:
            if self.d and self.hdrs[k]:
                self.d.contents.close(self.d, self.hdrs[k])
                self.hdrs[k] = None
            return
        if self.d:
            for j, h in enumerate(self.hdrs):
                if h:
                    self.d.contents.close(self.d, h)
                    self.hdrs[j] = None
            (self.L.mspack_destroy_szdd_decompressor if self.KIND == 0 else self.L.mspack_destroy_kwaj_decompressor)(self.d)
            self.d = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class SzddSet(_SkSet):
    KIND = 0


class KwajSet(_SkSet):
    KIND = 1
