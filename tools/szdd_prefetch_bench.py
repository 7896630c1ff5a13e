"""A directory of small SZDD files through the object API, with and without mspack_szddd_prefetch():
python tools/szdd_prefetch_bench.py [N=256,1024,4096] [REPS=5] [SESSIONS=3] -- N recipe SZDD files (tests/szdd_kwaj_recipe.py) of
about 16 KiB of text each, as files in a temporary directory, on ONE decompressor over the library's default (stdio) mspack_system:
  (a) open all, extract() every file -- every extract() is a batch of one unit (the behaviour without the call: the baseline);
  (b) open all, prefetch(all), the same extracts -- one batch.
(a) and (b) run alternately, REPS times each after one warm-up of each; every output file is compared with its plaintext.
Then the kernel alone: the same 1024 streams as one device-resident batch through mspack_hip_time_batch_device(), with
MSPACK_HIP_UF_LZSS_RING (no room below the units) and without it (4096 bytes below each), alternately, SESSIONS sessions of 20
iterations after a warm-up; ms per batch, lowest to highest session.  No ratio is asserted: the lines say what was measured."""
import ctypes as C, json, os, shutil, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import libmspack_amd as M
from libmspack_amd import api
import szdd_kwaj_recipe as Z

ns = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [256, 1024, 4096]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sessions = int(sys.argv[3]) if len(sys.argv) > 3 else 3
DISTINCT = 32                                    # distinct texts; the files cycle through them
plains = [M.gen_plaintext(500 + k, (0, 2)[k & 1], 16384 - 37 * k).tobytes() for k in range(DISTINCT)]
blobs = [Z.szdd_file(p) for p in plains]
L = api._setup_sk()
res = {"file_bytes": [min(map(len, blobs)), max(map(len, blobs))], "plain_bytes": [min(map(len, plains)), max(map(len, plains))], "runs": {}}


def leg(paths_in, paths_out, prefetch):
    """open all, (prefetch,) extract all, close all -> (seconds, seconds of the prefetch call)"""
    t0 = time.perf_counter()
    d = L.mspack_create_szdd_decompressor(None)
    m = d.contents
    hdrs = [m.open(d, p) for p in paths_in]
    assert all(hdrs)
    tp = 0.0
    if prefetch:
        arr = (C.POINTER(api.MsszdddHeader) * len(hdrs))(*hdrs)
        t1 = time.perf_counter()
        assert L.mspack_szddd_prefetch(d, arr, len(hdrs)) == 0
        tp = time.perf_counter() - t1
    for h, po in zip(hdrs, paths_out):
        assert m.extract(d, h, po) == 0
    for h in hdrs:
        m.close(d, h)
    L.mspack_destroy_szdd_decompressor(d)
    return time.perf_counter() - t0, tp


tmp = tempfile.mkdtemp(prefix="szdd_bench_")
try:
    for n in ns:
        pin = [os.fsencode(os.path.join(tmp, "f%05d.tx_" % i)) for i in range(n)]
        pout = [os.fsencode(os.path.join(tmp, "f%05d.txt" % i)) for i in range(n)]
        for i, p in enumerate(pin):
            with open(p, "wb") as fh:
                fh.write(blobs[i % DISTINCT])
        legs, counts, pf_ms = {"a": [], "b": []}, {}, []
        for k in range(reps + 1):
            for name, pf in (("a", 0), ("b", 1)):
                api.szdd_batch_counts(reset=True)
                api.lzss_ring_units(reset=True)
                t, tp = leg(pin, pout, pf)
                counts[name] = api.szdd_batch_counts() + (api.lzss_ring_units(),)
                for i in range(0, n, max(1, n // 64)):
                    with open(pout[i], "rb") as fh:
                        assert fh.read() == plains[i % DISTINCT], (name, i)
                if k:
                    legs[name].append(round(t * 1e3, 2))
                    if pf:
                        pf_ms.append(round(tp * 1e3, 2))
        res["runs"][n] = {"a_no_prefetch_ms": legs["a"], "b_prefetch_ms": legs["b"], "b_prefetch_call_ms": pf_ms,
                          "a_counts_batches_held_refit_ring": counts["a"], "b_counts_batches_held_refit_ring": counts["b"]}
        for p in pin + pout:
            os.unlink(p)
finally:
    shutil.rmtree(tmp, ignore_errors=True)

# ---- the kernel alone: 1024 streams, device-resident, flagged against unflagged ----
lib = M.lib()
EMU = hasattr(lib, "emu_dev_alloc")              # (the wavefront emulator's build: rehearsals of this script without a device; no timing means anything there)
hip = C.CDLL("libamdhip64.so") if not EMU else None
if EMU:
    lib.emu_dev_alloc.restype = C.c_void_p
    lib.emu_dev_alloc.argtypes = [C.c_size_t, C.c_int]


class EmuHip:
    def hipMalloc(self, pp, n):
        pp._obj.value = lib.emu_dev_alloc(n, 0)
        return 0

    def hipMemcpy(self, dst, src, n, _kind):
        C.memmove(dst, src, n)
        return 0

    def hipMemset(self, p, v, n):
        C.memset(p, v, n)
        return 0


if EMU:
    hip = EmuHip()
else:
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]


def dev(arr=None, nbytes=0):
    p = C.c_void_p()
    n = arr.nbytes if arr is not None else nbytes
    assert hip.hipMalloc(C.byref(p), max(n, 16)) == 0
    if arr is not None:
        assert hip.hipMemcpy(p, arr.ctypes.data, n, 1) == 0
    else:
        assert hip.hipMemset(p, 0, max(n, 16)) == 0
    return p


NK = 1024 if not EMU else 48
streams = [blobs[i % DISTINCT][14:] for i in range(NK)]
offs, pos = [], 0
for s in streams:
    pos = (pos + 15) & ~15
    offs.append(pos); pos += len(s)
arena = np.zeros(pos + 64, dtype=np.uint8)
for s, o in zip(streams, offs):
    arena[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
rooms = [len(plains[i % DISTINCT]) for i in range(NK)]
d_in = dev(arena)
kern = {}
for name, flags in (("ring", M.UF_LZSS_RING), ("plain", 0)):
    units, out_bytes = M.make_units(M.KIND_LZSS, offs, [len(s) for s in streams], rooms, flags=flags)
    units = np.ascontiguousarray(units)
    kern[name] = dict(units=dev(units), out=dev(nbytes=out_bytes + 64), res=dev(nbytes=NK * M.RESULT_DTYPE.itemsize), out_bytes=out_bytes,
                      host_units=units, mask=(1 << M.KIND_LZSS) | (M.MASK_LZSS_RING if flags else 0), ms=[])


def timed(k, iters):
    v = lib.mspack_hip_time_batch_device(k["units"], None, NK, d_in, arena.size, k["out"], k["out_bytes"], k["res"], None, 0, k["mask"], None, iters)
    assert v >= 0, lib.mspack_hip_last_error()
    return v


for name in kern:                                # warm-up, and the bytes
    timed(kern[name], 3)
    k = kern[name]
    out = np.empty(k["out_bytes"], dtype=np.uint8)
    r = np.zeros(NK, dtype=M.RESULT_DTYPE)
    assert hip.hipMemcpy(out.ctypes.data, k["out"], out.nbytes, 2) == 0 and hip.hipMemcpy(r.ctypes.data, k["res"], r.nbytes, 2) == 0
    for i in (0, 1, NK // 2, NK - 1):
        o = int(k["host_units"]["out_off"][i])
        assert r["err"][i] == 0 and r["out_len"][i] == rooms[i] and out[o:o + rooms[i]].tobytes() == plains[i % DISTINCT], (name, i)
for _s in range(sessions):
    for name in ("ring", "plain"):
        kern[name]["ms"].append(round(timed(kern[name], 20), 4))
res["kernel_1024_streams"] = {"ring_ms_per_batch": sorted(kern["ring"]["ms"]), "plain_ms_per_batch": sorted(kern["plain"]["ms"]),
                              "ring_out_arena_bytes": kern["ring"]["out_bytes"], "plain_out_arena_bytes": kern["plain"]["out_bytes"],
                              "in_bytes": int(arena.size)}
print(json.dumps(res))
for n, r in res["runs"].items():
    print("N=%s: without the call %s ms (%d batches), with it %s ms (%d batch; the call itself %s ms)" % (
        n, r["a_no_prefetch_ms"], r["a_counts_batches_held_refit_ring"][0], r["b_prefetch_ms"], r["b_counts_batches_held_refit_ring"][0],
        r["b_prefetch_call_ms"]))
k = res["kernel_1024_streams"]
print("kernel, 1024 streams: flagged %s ms per batch, unflagged %s ms per batch; output arena %d against %d bytes" % (
    k["ring_ms_per_batch"], k["plain_ms_per_batch"], k["ring_out_arena_bytes"], k["plain_out_arena_bytes"]))
