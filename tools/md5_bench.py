"""Per-file MD5 through the object API against what a caller had to do before mspack_cabd_md5() existed:
python tools/md5_bench.py [N=4096] [REPS=5]            the two shapes, three variants each
python tools/md5_bench.py rates [MIB=8] [REPS=5]       the two rates behind the cabinet driver's long-range bound
Shapes (config 2's plaintext, C in-memory mspack_system, libmspack_amd/csrc/bench/api_bench.c -- no Python inside a call):
  one_cabinet    ONE cabinet of N MSZIP folders of 32 KiB, one file each: the first call forms the batch;
  many_cabinets  N one-folder cabinets on one decompressor behind one mspack_cabd_prefetch().
Variants, run in turn, REPS times each after one warm-up of each, wall time around the whole session (create .. destroy):
  md5_on    md5() of every file, MSCABD_PARAM_HIP_MD5 = 1 (digests from the device where the policy gives a file a unit);
  md5_off   md5() of every file, the param off (the plain-C MD5 on the host);
  extract   extract() of every file into memory, then hashlib.md5 per file -- inside the timed region: the baseline, what a user
            of the library without md5() does.
Every variant's digests are compared with hashlib's.  One JSON line: min / median / max per variant and shape, in ms.

rates: `lane` one digest unit (MSPACK_HIP_KIND_MD5) over one range of MIB MiB alone in its batch, device-resident, timed with
events (mspack_hip_time_batch_device): the rate of ONE lane; `wave` / `waves64` 64 and 4096 ranges, for scale; `host` the drivers'
plain-C MD5 (csrc/host/md5.c) over the same bytes on one core, beside hashlib.  ratio = lane rate / host rate."""
import ctypes as C, hashlib, json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import libmspack_amd as M
from libmspack_amd import apibench as A


def stats(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def shapes(n, reps):
    ub = 32768
    images, plain = A.build_small_cabs(M, n, ub)
    one, _p = A.build_config2_cab(M, n, ub, plain=plain)
    want = [hashlib.md5(plain[i * ub:(i + 1) * ub].tobytes()).digest() for i in range(n)]
    L = A.lib()
    L.mspack_cabd_md5_counts.argtypes = [C.c_void_p, C.c_int]
    res = {"n_files": n, "file_bytes": ub, "reps": reps}
    for shape, imgs, pf in (("one_cabinet", [one], 0), ("many_cabinets", images, 1)):
        legs = {"md5_on": [], "md5_off": [], "extract": []}
        counts = {}
        for k in range(reps + 1):
            for leg in legs:
                L.mspack_cabd_md5_counts(None, 1)
                t0 = time.perf_counter()
                if leg == "extract":
                    rc, out, d = A.run_cabs(imgs, plain.size, pf)
                    got = [hashlib.md5(out[i * ub:(i + 1) * ub]).digest() for i in range(n)]
                else:
                    rc, got, d = A.run_cabs_md5(imgs, pf, leg == "md5_on", max_files=n)
                ms = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and d["n_errors"] == 0 and d["n_files"] == n and got == want, (shape, leg, rc, d)
                c = (C.c_ulonglong * 2)(); L.mspack_cabd_md5_counts(c, 0)
                counts[leg] = [int(c[0]), int(c[1])]
                if k:
                    legs[leg].append(ms)
        res[shape] = {leg: stats(v) for leg, v in legs.items()}
        res[shape]["digests_from_device_and_host"] = counts
    print(json.dumps(res))


def rates(mib, reps):
    L = M.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def dev(arr):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(arr.nbytes, 16)) == 0
        assert hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
        return p.value
    n = mib << 20
    data = np.random.default_rng(1).integers(0, 256, n + 64, dtype=np.uint8)
    d_out = dev(data)
    res = {"range_mib": mib, "reps": reps}
    for name, count, each in (("lane", 1, n), ("wave", 64, n // 64), ("waves64", 4096, n // 4096)):
        units = M.md5_units([(i * each + (i % 16), each - 16) for i in range(count)])
        d_units, d_res = dev(units.view(np.uint8)), dev(np.zeros(count * 24, dtype=np.uint8))
        ms = [L.mspack_hip_time_batch_device(d_units, None, count, None, 0, d_out, n + 64, d_res, None, 0, M.MASK_MD5, None, 1) for _ in range(reps + 1)][1:]
        assert min(ms) > 0
        back = np.zeros(count, dtype=M.RESULT_DTYPE)
        assert hip.hipMemcpy(back.ctypes.data, d_res, back.nbytes, 2) == 0
        o, ln = int(units["out_off"][count - 1]), int(units["out_len"][count - 1])
        assert M.result_digests(back)[count - 1] == hashlib.md5(data[o:o + ln].tobytes()).digest()
        res[name + "_ms"] = stats(ms)
        res[name + "_MBps"] = round(count * (each - 16) / 1e6 / (statistics.median(ms) * 1e-3), 1)

    class Ctx(C.Structure):
        _fields_ = [("st", C.c_uint32 * 4), ("bytes", C.c_uint64), ("buf", C.c_ubyte * 64)]

    def host_once():
        c, d = Ctx(), (C.c_ubyte * 16)()
        t0 = time.perf_counter()
        L.mspack_md5_init(C.byref(c)); L.mspack_md5_update(C.byref(c), C.c_void_p(data.ctypes.data), C.c_size_t(n)); L.mspack_md5_final(C.byref(c), d)
        t = time.perf_counter() - t0
        assert bytes(d) == hashlib.md5(data[:n].tobytes()).digest()
        return t * 1e3
    ms = [host_once() for _ in range(reps + 1)][1:]
    res["host_ms"] = stats(ms)
    res["host_MBps"] = round(n / 1e6 / (statistics.median(ms) * 1e-3), 1)
    buf = data[:n].tobytes()
    t = []
    for _ in range(reps + 1):
        t0 = time.perf_counter(); hashlib.md5(buf).digest(); t.append((time.perf_counter() - t0) * 1e3)
    res["hashlib_MBps"] = round(n / 1e6 / (statistics.median(t[1:]) * 1e-3), 1)
    res["ratio"] = round(res["lane_MBps"] / res["host_MBps"], 4)
    print(json.dumps(res))


if len(sys.argv) > 1 and sys.argv[1] == "rates":
    rates(int(sys.argv[2]) if len(sys.argv) > 2 else 8, int(sys.argv[3]) if len(sys.argv) > 3 else 5)
else:
    shapes(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
