"""Measurements for MSPACK_HIP_KIND_STORED and MSCABD_PARAM_HIP_STORED -> profiles/stored_folders.txt.
  1. the copy alone, device-resident: mspack_hip_time_batch_device against hipMemcpyAsync device-to-device of the same bytes
  2. through the cabinet driver (Python object API, open to last call), MSCABD_PARAM_HIP_STORED 0 against 1
Three runs each, min - max.  usage: python tools/stored_bench.py [--out profiles/stored_folders.txt] [--quick]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import libmspack_amd as M
from libmspack_amd import api

RUNS = 3
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def span(v, fmt="%.2f"):
    return (fmt + " - " + fmt) % (min(v), max(v))


class Hip:
    def __init__(self):
        h = self.h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        h.hipFree.argtypes = [C.c_void_p]

    def alloc(self, n):
        p = C.c_void_p()
        assert self.h.hipMalloc(C.byref(p), max(n, 16)) == 0
        return p.value

    def put(self, p, arr):
        assert self.h.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0

    def get(self, p, n):
        out = np.empty(n, dtype=np.uint8)
        assert self.h.hipMemcpy(out.ctypes.data, p, n, 2) == 0
        return out


def copy_alone(hip, name, lens, iters):
    """units packed back to back, sources at an odd offset (in_off - out_off = 5 mod 16: the realigned path)"""
    rows, ipos, opos = [], 5, 0
    for n in lens:
        rows.append((ipos, n, opos, n)); ipos += n; opos += n
    u = np.zeros(len(rows), dtype=M.UNIT_DTYPE)
    u["kind"] = M.KIND_STORED
    u["in_off"] = [r[0] for r in rows]; u["in_len"] = [r[1] for r in rows]; u["out_off"] = [r[2] for r in rows]; u["out_len"] = [r[3] for r in rows]
    total = opos
    src = np.random.default_rng(1).integers(0, 256, min(ipos, 1 << 24), dtype=np.uint8)
    d_in, d_out, d_u, d_r = hip.alloc(ipos + 64), hip.alloc(total + 64), hip.alloc(u.nbytes), hip.alloc(len(u) * 24)
    for o in range(0, ipos, src.size):
        hip.put(d_in + o, src[:min(src.size, ipos - o)])
    hip.put(d_u, u.view(np.uint8))
    L = M.lib()
    ms = []
    for _ in range(RUNS + 1):                                              # (the first run warms up)
        t = L.mspack_hip_time_batch_device(d_u, None, len(u), d_in, ipos, d_out, total, d_r, None, 0, M.MASK_STORED, None, iters)
        assert t > 0, L.mspack_hip_last_error()
        ms.append(t)
    ms = ms[1:]
    # one look at the bytes: the first and the last MiB
    chk = min(total, 1 << 20)
    assert np.array_equal(hip.get(d_out, chk), np.resize(src, ipos)[5:5 + chk]) if ipos <= src.size else True
    # the yardstick: hipMemcpyAsync device to device of the same bytes -- one copy per unit, at most 4096 of them (scaled to all)
    cap = min(len(rows), 4096)
    ref = []
    for _ in range(RUNS + 1):
        hip.h.hipDeviceSynchronize()
        t0 = time.perf_counter()
        for _i in range(iters):
            for (io, n, oo, _n) in rows[:cap]:
                if n:
                    hip.h.hipMemcpyAsync(d_out + oo, d_in + io, n, 3, None)
        hip.h.hipDeviceSynchronize()
        ref.append((time.perf_counter() - t0) * 1e3 / iters * (len(rows) / cap))
    ref = ref[1:]
    gbs = [total / (t * 1e-3) / 1e9 for t in ms]
    rgbs = [total / (t * 1e-3) / 1e9 for t in ref]
    say("%-44s %9.1f MB  kernel %s ms (%s GB/s)   hipMemcpyAsync D2D%s %s ms (%s GB/s)   ratio of rates %.2f" % (
        name, total / 1e6, span(ms, "%.3f"), span(gbs, "%.1f"), " (first %d copies, scaled)" % cap if cap < len(rows) else "", span(ref, "%.3f"),
        span(rgbs, "%.1f"), np.median(gbs) / np.median(rgbs)))
    for p in (d_in, d_out, d_u, d_r):
        hip.h.hipFree(p)


def driver(quick):
    import test_cab_stored as T
    nf = 4096 if not quick else 256
    data = T.rnd(5, nf * 32768)
    cab, _ = T.build_cab([dict(data=data, files=[(b"f%04d.bin" % k, k * 32768, 32768) for k in range(nf)])])
    say("cabinet of one stored folder, %d files of 32 KiB (%.0f MB), open to last call, ms:" % (nf, len(cab) / 1e6))
    for what, params in (("crc32()", ((api.MSCABD_PARAM_HIP_CRC32, 1),)), ("md5()", ((api.MSCABD_PARAM_HIP_MD5, 1),)),
                         ("digest(SHA-256)", ((api.MSCABD_PARAM_HIP_DIGESTS, 4),)), ("extract()", ())):
        res = {}
        for stored in (0, 1):
            ts = []
            for _ in range(RUNS):
                t0 = time.perf_counter()
                with api.Cab(cab, mem=False) as c:
                    c.set_param(api.MSCABD_PARAM_HIP_STORED, stored)
                    for p, v in params:
                        c.set_param(p, v)
                    for i in range(nf):
                        if what == "crc32()":
                            e, _v = c.crc32(i)
                        elif what == "md5()":
                            e, _v = c.md5(i)
                        elif what == "extract()":
                            e = c.d.contents.extract(c.d, c._files[i], b"/dev/null")
                        else:
                            e, _v = c.digest(i, 4)
                        assert e == 0
                ts.append((time.perf_counter() - t0) * 1e3)
            res[stored] = ts
        say("  %-16s HIP_STORED 0: %s   HIP_STORED 1: %s" % (what, span(res[0], "%.1f"), span(res[1], "%.1f")))
    nc = 1024 if not quick else 64
    cabs = [T.build_cab([dict(data=T.rnd(1000 + k, 16384), files=[(b"a.bin", 0, 16384)])])[0] for k in range(nc)]
    res = {}
    for stored in (0, 1):
        ts = []
        for _ in range(RUNS):
            M.slot_stats(reset=True)
            t0 = time.perf_counter()
            with api.CabSet(cabs, mem=False) as s:
                s.set_param(api.MSCABD_PARAM_HIP_STORED, stored)
                assert s.prefetch() == 0
                for k in range(nc):
                    for f in s.file_ptrs(k):
                        assert s.d.contents.extract(s.d, f, b"/dev/null") == 0
            ts.append((time.perf_counter() - t0) * 1e3)
            res[stored] = (ts, M.slot_stats()[0])
    say("%d cabinets of one stored folder of 16 KiB, prefetch() + extract(), ms:  HIP_STORED 0: %s (%d batches)   HIP_STORED 1: %s (%d batch)" % (
        nc, span(res[0][0], "%.1f"), res[0][1], span(res[1][0], "%.1f"), res[1][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stored_folders.txt"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    say("# tools/stored_bench.py: %s; three runs each, min - max" % M.lib().mspack_hip_version().decode())
    say("## 1. the copy alone (device-resident, mspack_hip_time_batch_device; sources 5 bytes off the destinations' rows)")
    hip = Hip()
    rng = np.random.default_rng(3)
    small = [int(x) for x in rng.integers(64, 301, 100000 if not a.quick else 5000)]
    big = (256 << 20) if not a.quick else (16 << 20)
    copy_alone(hip, "one unit of %d MiB" % (big >> 20), [big], 5)
    copy_alone(hip, "four units of %d MiB" % (big >> 22), [big // 4] * 4, 5)
    copy_alone(hip, "4096 units of 32 KiB", [32768] * 4096, 10)
    copy_alone(hip, "%d units of 64 to 300 bytes" % len(small), small, 5)
    copy_alone(hip, "... with the %d MiB unit among them" % (big >> 20), small[:len(small) // 2] + [big] + small[len(small) // 2:], 3)
    say("## 2. through the cabinet driver")
    driver(a.quick)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
