"""The CRC-32 range pass (MSPACK_HIP_KIND_CRC32) alone, device-resident, timed with events (mspack_hip_time_batch_device):
python tools/crc32_files_bench.py [REPS=3] > profiles/crc32_files.txt
  balance     100 000 ranges of 64 - 300 bytes plus ONE range of 256 MiB in one list, against the 256 MiB range alone: where the
              ticket space has to show (with one wave per range the long range would be one wave's work);
  files_32k   4096 ranges of 32 KiB back to back (the digest benches' shape, as ranges);
  large_4     four ranges of 64 MiB (one LZX folder of 256 MiB holding four large files, as ranges);
  zlib        zlib.crc32 over the same 256 MiB on one core: the yardstick, what a caller does today after extract().
Every list's checksums are compared with zlib's.  One JSON line per shape: min / median / max in ms, and MB/s at the median.

python tools/crc32_files_bench.py files [N=4096] [REPS=3]
  shape (a): ONE cabinet of N MSZIP folders of 32 KiB, one file each (the digest benches' shape), through the Python object API on an
  in-memory mspack_system, a fresh decompressor per run, wall time from open to the last call:
    crc32_on   Cab.crc32(i) of every file, MSCABD_PARAM_HIP_CRC32 = 1;
    crc32_off  the same with the param 0 (the host fallback);
    extract    Cab.extract(i) of every file + zlib.crc32: what users do today -- the yardstick.

python tools/crc32_files_bench.py large [MIB=256] [REPS=3]
  shape (b): ONE cabinet with ONE LZX folder (window 2^21) of MIB MiB holding four large files of unequal length that tile it -- the
  shape the lane digests cannot serve: every file is far above the digest ratio.  The same three legs, the same way."""
import ctypes as C, json, os, statistics, sys, time, zlib
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import libmspack_amd as M


def stats(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main(reps):
    L = M.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def dev(arr):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(arr.nbytes, 16)) == 0
        assert hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
        return p.value
    big = 256 << 20
    rng = np.random.default_rng(32)
    data = rng.integers(0, 256, big + 64, dtype=np.uint8)
    d_out = dev(data)
    short = [(int(o), int(n)) for o, n in zip(rng.integers(0, big - 300, 100000), rng.integers(64, 301, 100000))]
    shapes = (("long_alone", [(5, big)]),
              ("short_and_long", short[:50000] + [(5, big)] + short[50000:]),
              ("short_alone", short),
              ("files_32k", [(i * 32768, 32768) for i in range(4096)]),
              ("large_4", [(i * (64 << 20) + i, (64 << 20) - 16) for i in range(4)]))
    for name, ranges in shapes:
        units = M.crc32r_units(ranges)
        d_units, d_res = dev(units.view(np.uint8)), dev(np.zeros(len(units) * 24, dtype=np.uint8))
        ms = [L.mspack_hip_time_batch_device(d_units, None, len(units), None, 0, d_out, big + 64, d_res, None, 0, M.MASK_CRC32R, None, 1)
              for _ in range(reps + 1)][1:]
        assert min(ms) > 0
        back = np.zeros(len(units), dtype=M.RESULT_DTYPE)
        assert hip.hipMemcpy(back.ctypes.data, d_res, back.nbytes, 2) == 0
        assert (back["err"] == 0).all() and (back["in_used"] == 0).all() and (back["good_len"] == 0).all() and (back["in_next"] == 0).all()
        for i in sorted(set([0, len(units) // 2, len(units) - 1] + [int(np.argmax(units["out_len"]))])):
            o, n = ranges[i]
            assert int(back["out_len"][i]) == zlib.crc32(data[o:o + n]) & 0xFFFFFFFF, (name, i)
        nbytes = int(units["out_len"].astype(np.int64).sum())
        print(json.dumps({"shape": name, "ranges": len(units), "bytes": nbytes, "reps": reps, "ms": stats(ms),
                          "MBps": round(nbytes / 1e6 / (statistics.median(ms) * 1e-3), 1)}), flush=True)
        hip.hipFree(d_units); hip.hipFree(d_res)
    buf = data[:big].tobytes()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); zlib.crc32(buf); t.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"shape": "zlib", "bytes": big, "reps": reps, "ms": stats(t), "MBps": round(big / 1e6 / (statistics.median(t) * 1e-3), 1)}))


def large_cab(mib):
    """one LZX-21 folder of mib MiB (the corpus encoder at chain depth 1: the cabinet is built once, outside every timed region),
    four files cut at unaligned places -> (cabinet, [the files' bytes])"""
    n = mib << 20
    data = M.gen_plaintext(0xB16, 0, n)
    lz, fo = M.lzx_encode(data, 21, 0, M.lzx_opts(depth=1, lazy=0))
    blocks = [lz[int(fo[i]):int(fo[i + 1])].tobytes() for i in range(len(fo) - 1)]
    edges = [0, n * 5 // 32 + 3, n * 13 // 32 + 1001, n * 3 // 4 - 77, n]
    files = [(b"large%d.bin" % k, edges[k + 1] - edges[k], edges[k], 0) for k in range(4)]
    cab = M.cab_write([(3 | (21 << 8), blocks, [32768] * (n // 32768))], files)
    return cab, [data[edges[k]:edges[k + 1]] for k in range(4)]


def files(n, reps, mib=0):
    from libmspack_amd import api, apibench as A
    ub = 32768
    if mib:
        cab, parts = large_cab(mib)
        n = len(parts)
        want = [zlib.crc32(p) & 0xFFFFFFFF for p in parts]
    else:
        cab, plain = A.build_config2_cab(M, n, ub)
        want = [zlib.crc32(plain[i * ub:(i + 1) * ub].tobytes()) & 0xFFFFFFFF for i in range(n)]
    legs = {"crc32_on": [], "crc32_off": [], "extract": []}
    counts = {}
    for k in range(reps + 1):
        for leg in legs:
            api.cabd_crc32_counts(reset=True)
            t0 = time.perf_counter()
            with api.Cab(cab, mem=True) as c:
                if leg == "extract":
                    got = []
                    for i in range(n):
                        c.mem.outputs.clear()
                        err, data = c.extract(i)
                        assert err == 0
                        got.append(zlib.crc32(data) & 0xFFFFFFFF)
                else:
                    assert c.set_param(api.MSCABD_PARAM_HIP_CRC32, int(leg == "crc32_on")) == 0
                    got = []
                    for i in range(n):
                        err, v = c.crc32(i)
                        assert err == 0
                        got.append(v)
            ms = (time.perf_counter() - t0) * 1e3
            assert got == want, leg
            counts[leg] = api.cabd_crc32_counts()
            if k:
                legs[leg].append(ms)
    shape = {"shape": "b: one LZX folder", "folder_mib": mib, "file_bytes": [len(p) for p in parts], "cabinet_bytes": len(cab)} if mib else \
            {"shape": "a: one MSZIP cabinet", "file_bytes": ub}
    print(json.dumps({**shape, "n_files": n, "reps": reps,
                      **{leg: stats(v) for leg, v in legs.items()}, "crc32_from_device_and_host": counts}))


if len(sys.argv) > 1 and sys.argv[1] == "large":
    files(0, int(sys.argv[3]) if len(sys.argv) > 3 else 3, mib=int(sys.argv[2]) if len(sys.argv) > 2 else 256)
elif len(sys.argv) > 1 and sys.argv[1] == "files":
    files(int(sys.argv[2]) if len(sys.argv) > 2 else 4096, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
else:
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
