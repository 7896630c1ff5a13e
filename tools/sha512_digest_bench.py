"""Per-file SHA-384 / SHA-512 through mspack_cabd_digest() against what a caller had to do before it existed:
python tools/sha512_digest_bench.py [N=4096] [REPS=5]            one cabinet of N files of 32 KiB, three variants per algorithm
python tools/sha512_digest_bench.py rates [MIB=8] [REPS=3]       the two rates behind the cabinet driver's long-range bound
Workload (tools/digest_bench.py's: config 2's plaintext, C in-memory mspack_system, libmspack_amd/csrc/bench/api_bench.c -- no Python
inside a call): ONE cabinet of N MSZIP folders of 32 KiB, one file each; the first call forms the batch.
Variants per algorithm, run in turn, REPS times each after one warm-up of each, wall time around the whole session (create .. destroy):
  on        digest() of every file, the algorithm's bit of MSCABD_PARAM_HIP_DIGESTS64 set (digests from the device where the policy
            gives a file a unit);
  off       digest() of every file, the param 0 (the plain-C hash on the host);
  extract   extract() of every file into memory, then hashlib per file -- inside the timed region: the baseline, which does not depend
            on this library's digest code.
Every variant's digests are compared with hashlib's.  One JSON line: min / median / max per variant, in ms.

rates: `lane` one digest unit over one range of MIB MiB alone in its batch, device-resident, timed with events
(mspack_hip_time_batch_device): the rate of ONE lane; `wave` 64 ranges, for scale; `host` the drivers' plain-C hash
(csrc/host/sha512.c) over the same bytes on one core, beside hashlib.  ratio = lane rate / host rate, per run; the compiled
SHA512_RATIO_DEFAULT (csrc/host/host_digest.h) is the quotient rounded down, one for both algorithms."""
import ctypes as C, hashlib, json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import libmspack_amd as M
from libmspack_amd import apibench as A

ALGS = (("sha384", 16, hashlib.sha384, M.KIND_SHA384, M.MASK_SHA384), ("sha512", 32, hashlib.sha512, M.KIND_SHA512, M.MASK_SHA512))


def stats(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def shapes(n, reps):
    ub = 32768
    one, plain = A.build_config2_cab(M, n, ub)
    L = A.lib()
    L.mspack_cabd_digest_counts.argtypes = [C.c_int, C.c_void_p, C.c_int]
    res = {"n_files": n, "file_bytes": ub, "reps": reps}
    for name, alg, h, _k, _m in ALGS:
        want = [h(plain[i * ub:(i + 1) * ub].tobytes()).digest() for i in range(n)]
        legs = {"on": [], "off": [], "extract": []}
        counts = {}
        for k in range(reps + 1):
            for leg in legs:
                L.mspack_cabd_digest_counts(alg, None, 1)
                t0 = time.perf_counter()
                if leg == "extract":
                    rc, out, d = A.run_cabs([one], plain.size, 0)
                    got = [h(out[i * ub:(i + 1) * ub]).digest() for i in range(n)]
                else:
                    rc, got, d = A.run_cabs_digest64([one], 0, alg if leg == "on" else 0, alg, max_files=n)
                ms = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and d["n_errors"] == 0 and d["n_files"] == n and got == want, (name, leg, rc, d)
                c = (C.c_ulonglong * 2)(); L.mspack_cabd_digest_counts(alg, c, 0)
                counts[leg] = [int(c[0]), int(c[1])]
                if k:
                    legs[leg].append(ms)
        res[name] = {leg: stats(v) for leg, v in legs.items()}
        res[name]["digests_from_device_and_host"] = counts
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

    class Ctx(C.Structure):
        _fields_ = [("st", C.c_uint64 * 8), ("bytes", C.c_uint64), ("buf", C.c_ubyte * 128), ("out", C.c_int)]

    for name, alg, h, kind, mask in ALGS:
        r = {}
        for leg, count, each in (("lane", 1, n), ("wave", 64, n // 64)):
            ranges = [(i * each + (i % 16), each - 16) for i in range(count)]
            units, _heads = M.digest_units(ranges, kind)
            d_units, d_res = dev(units.view(np.uint8)), dev(np.zeros(len(units) * 24, dtype=np.uint8))
            ms = [L.mspack_hip_time_batch_device(d_units, None, len(units), None, 0, d_out, n + 64, d_res, None, 0, mask, None, 1) for _ in range(reps + 1)][1:]
            assert min(ms) > 0
            back = np.zeros(len(units), dtype=M.RESULT_DTYPE)
            assert hip.hipMemcpy(back.ctypes.data, d_res, back.nbytes, 2) == 0
            o, ln = ranges[-1]
            assert M.result_wide_digests(back, units)[-1] == h(data[o:o + ln].tobytes()).digest()
            r[leg + "_ms"] = [round(x, 3) for x in ms]
            r[leg + "_MBps"] = [round(count * (each - 16) / 1e6 / (x * 1e-3), 1) for x in ms]

        def host_once():
            c, d = Ctx(), (C.c_ubyte * 64)()
            t0 = time.perf_counter()
            (L.mspack_sha384_init if alg == 16 else L.mspack_sha512_init)(C.byref(c))
            L.mspack_sha512_update(C.byref(c), C.c_void_p(data.ctypes.data), C.c_size_t(n)); L.mspack_sha512_final(C.byref(c), d)
            t = time.perf_counter() - t0
            assert bytes(d)[:h().digest_size] == h(data[:n].tobytes()).digest()
            return t * 1e3
        ms = [host_once() for _ in range(reps + 1)][1:]
        r["host_ms"] = [round(x, 3) for x in ms]
        r["host_MBps"] = [round(n / 1e6 / (x * 1e-3), 1) for x in ms]
        buf = data[:n].tobytes()
        t = []
        for _ in range(reps + 1):
            t0 = time.perf_counter(); h(buf).digest(); t.append((time.perf_counter() - t0) * 1e3)
        r["hashlib_MBps"] = round(n / 1e6 / (statistics.median(t[1:]) * 1e-3), 1)
        r["ratio"] = [round(a / b, 4) for a, b in zip(r["lane_MBps"], r["host_MBps"])]
        res[name] = r
    print(json.dumps(res))


if len(sys.argv) > 1 and sys.argv[1] == "rates":
    rates(int(sys.argv[2]) if len(sys.argv) > 2 else 8, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
else:
    shapes(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 5)
