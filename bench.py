#!/usr/bin/env python3
"""bench.py -- headline metric of BASELINE.json: decompressed MB/s, LZX 21-bit window,
4096-interval batch (per GPU; weak scaling over --gpus), inputs resident in HBM.

A "step" = one pass of the hot path (mspack_hip_decode_batch_device) over the whole batch of
independent CHM-style reset intervals (64 KiB each = reset interval of 2 frames).
Prints ONE JSON line on rank 0.

Multi-GPU: one process per GPU, no data-path collective (units are independent); torch.distributed
(backend nccl = RCCL) is used only for the barrier and the max-over-ranks time.  `--gpus N` without a
launcher (no WORLD_SIZE in the environment) spawns the N ranks itself; under torchrun the launcher's world
size must equal --gpus.  A box with fewer GPUs than ranks is an error, never a silent 1-GPU run.
  --scaling weak   (default) every rank decodes its own --units intervals (BASELINE metric, 4096 per GPU)
  --scaling strong --total-units T: BASELINE config 5 (T = 65536): one global list of T intervals, rank r
                   decodes the contiguous shard libmspack_amd.dist.shard_range(T, r, world) of it.

A plain run sets up, warms up, times --steps steps, checks the last step's per-unit results (no error, full length) and
prints the line.  `--dump-outputs DIR` also writes what that last step handed back (rank 0) as DIR/<name>.npy.
`--full` adds, after the timed region, every byte compared with the plaintext (config.bit_exact), the spread of single
launches and
  roofline        the LZX kernel's duration from HIP events on the launch stream vs algorithmic bytes
and at N=1 (host_inclusive's clean-process worker runs first):
  host_inclusive  SURVEY 8(d)'s metric as written: from compressed units in HOST memory to decoded bytes in
                  device memory (mspack_hip_decode_batch_to_device) and, separately, back in host memory
                  (mspack_hip_decode_batch) -- what a cabd/chmd extract() caller gets; measured in a process of its
                  own that holds only the library (started before this one touches the GPU), and from this process
  secondary       BASELINE configs 2 (4096 MSZIP blocks) and 4 (512 Quantum folders, window 21, 32 frames)
  cpu_baseline    the real reference lzxd on the host cores (oracle/_ref), or -- loudly -- our CPU port
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0     # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md
LZX_KERNELS = "mspack_lzx_pipe_map + mspack_lzx_pipe + mspack_decode_lzx (resume)"
METRIC = "decompressed MB/s (whole node), LZX 21-bit window, 4096-interval batch"


def usable_cpus():
    """CPUs this process can actually run on: the affinity mask capped by the cgroup CPU quota (the GPU
    boxes expose every host thread but grant a fixed quota, and threads beyond it only add contention)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except Exception:
            pass
    return n


def lscpu_summary():
    """what the host is (lscpu): model, sockets, cores per socket, threads per core -- printed beside the CPU baseline"""
    keep = ("model name", "socket(s)", "core(s) per socket", "thread(s) per core", "cpu(s)", "numa node(s)", "cpu max mhz")
    out = {}
    try:
        txt = subprocess.run(["lscpu"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=10).stdout.decode()
        for l in txt.splitlines():
            k, _, v = l.partition(":")
            if k.strip().lower() in keep:
                out[k.strip()] = v.strip()
    except Exception:
        pass
    return out


def cores_per_socket():
    """physical cores of one socket of this host (lscpu), or None"""
    try:
        txt = subprocess.run(["lscpu"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=10).stdout.decode()
        for l in txt.splitlines():
            if l.strip().lower().startswith("core(s) per socket"):
                return int(l.split(":")[1])
    except Exception:
        pass
    return None


def cpu_baseline(comp, off, ln, n_units, unit_bytes):
    """Reference CPU path (oracle/_ref = the real libmspack lzxd, built from /root/reference in the
    dev container) over the same units on the host cores.  If oracle/_ref did not travel, the line says so
    in so many words and times our CPU restatement instead (kind "port")."""
    import ctypes as C
    import helpers
    cores = usable_cpus()
    why = "oracle/_ref/librefharness.so is missing"
    if helpers.have_ref():
        try:
            R = helpers.ref()
            off64 = np.ascontiguousarray(off, dtype=np.uint64)
            ilen = np.ascontiguousarray(ln + 4, dtype=np.uint32)
            olen = np.full(n_units, unit_bytes, dtype=np.uint32)

            def run(threads, reps):
                b = C.c_ulonglong(0); e = C.c_int(0)
                t = R.refh_bench(0, comp.ctypes.data, off64.ctypes.data, ilen.ctypes.data, olen.ctypes.data,
                                 n_units, 21, unit_bytes // 32768, threads, reps, C.byref(b), C.byref(e))
                if e.value:
                    raise RuntimeError("reference failed on %d units" % e.value)
                return b.value / t / 1e6, t
            one, _t = run(1, 1)                                   # one core, one pass: MB/s per core
            est_pass_s = n_units * unit_bytes / (one * 1e6) / cores
            reps = max(2, min(256, int(15.0 / max(est_pass_s, 1e-3))))
            allv, tall = run(cores, reps)
            return {"value": round(allv, 1), "unit": "MB/s", "cores": cores, "kind": "reference",
                    "one_core_MBps": round(one, 1), "host_threads": os.cpu_count(),
                    "sample": "%d passes over the same %d-unit batch (%.0f MiB decoded per pass) on %d threads (= usable "
                              "CPUs: affinity and cgroup quota) in %.2f s, threads released together; libmspack "
                              "lzxd_decompress memory-to-memory, one decompressor per thread" %
                              (reps, n_units, n_units * unit_bytes / 2**20, cores, tall)}
        except Exception as ex:          # pragma: no cover
            why = "the reference harness failed: %s" % ex
    sys.stderr.write("bench.py: WARNING: cpu_baseline is NOT the reference (%s); timing the CPU port instead\n" % why)
    sample = min(n_units, 256)
    t0 = time.perf_counter()
    for i in range(sample):
        e, o, _ = helpers.oracle_lzx(comp[int(off[i]):int(off[i]) + int(ln[i]) + 4].tobytes(), unit_bytes, 21,
                                     unit_bytes // 32768)
        assert e == 0
    dt = time.perf_counter() - t0
    return {"value": round(sample * unit_bytes / dt / 1e6, 1), "unit": "MB/s", "cores": 1, "kind": "port",
            "fallback": True, "fallback_reason": why,
            "sample": "first %d units, single thread, oracle/liboracle.so (NOT the reference)" % sample}


def ref_cpu_secondary(kind, comp, off, ln, out_lens, window_bits, reset_frames, budget_s=8.0):
    """the real reference codec (oracle/_ref: kind 0 lzxd, 1 mszipd, 2 qtmd) over the same units on the usable host cores,
    a bounded number of passes; None when the reference library did not travel"""
    import ctypes as C
    import helpers
    if not helpers.have_ref():
        return None
    try:
        R = helpers.ref()
        cores = usable_cpus()
        n = len(off)
        off64 = np.ascontiguousarray(off, dtype=np.uint64)
        ilen = np.ascontiguousarray(ln, dtype=np.uint32)
        olen = np.ascontiguousarray(out_lens, dtype=np.uint32)

        def run(units, threads, reps):
            b = C.c_ulonglong(0); e = C.c_int(0)
            t = R.refh_bench(kind, comp.ctypes.data, off64.ctypes.data, ilen.ctypes.data, olen.ctypes.data, units,
                             window_bits, reset_frames, threads, reps, C.byref(b), C.byref(e))
            if e.value:
                raise RuntimeError("reference failed on %d units" % e.value)
            return b.value / t / 1e6, t
        probe = max(1, min(n, cores))                                # one unit per core: the per-core rate
        rate1, t1 = run(probe, probe, 1)
        est_pass = float(olen.sum()) / (rate1 * 1e6)
        reps = max(1, min(64, int(budget_s / max(est_pass, 1e-3))))
        units = n if est_pass <= budget_s else max(cores, int(n * budget_s / est_pass))
        v, t = run(units, cores, reps)
        used = min(cores, units)                                     # (a thread per unit at most: ONE folder is one core's work)
        return {"value": round(v, 1), "unit": "MB/s", "cores": used, "kind": "reference",
                "sample": "%d pass(es) over %d of the %d units on %d threads in %.2f s (libmspack's own codec, memory to memory)" %
                          (reps, units, n, used, t)}
    except Exception as ex:          # pragma: no cover
        return {"value": None, "kind": "reference", "error": str(ex)}


# ---- device-resident batch: upload once, time launches with HIP events on the launch stream ----------------
class DeviceBatch:
    def __init__(self, M, torch, dev, units, comp, out_bytes, kind):
        self.M, self.torch, self.kind = M, torch, kind
        self.frame_tables = bool((units["flags"] & M.UF_FRAME_TABLE).any())
        self.n = len(units)
        self.units, self.comp_size, self.out_bytes = units, int(comp.size), int(out_bytes)
        self.n_frames = int(M.frames_of(units).sum())
        order = np.argsort(-(units["in_len"].astype(np.int64)), kind="stable").astype(np.uint32)   # longest first
        self.d_in = torch.zeros(comp.size + 64, dtype=torch.uint8, device=dev)
        self.d_in[:comp.size] = torch.from_numpy(comp).to(dev)
        self.d_units = torch.from_numpy(units.view(np.uint8)).to(dev)
        self.d_order = torch.from_numpy(order.view(np.uint8)).to(dev)
        self.d_out = torch.zeros(out_bytes + 64, dtype=torch.uint8, device=dev)
        self.d_res = torch.zeros(self.n * M.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.d_fm = torch.zeros(max(64, M.lib().mspack_hip_frame_scratch_bytes(self.n_frames)), dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.L = M.lib()

    def _args(self):
        return (self.d_units.data_ptr(), self.d_order.data_ptr(), self.n, self.d_in.data_ptr(), self.comp_size,
                self.d_out.data_ptr(), self.out_bytes, self.d_res.data_ptr(), self.d_fm.data_ptr(), self.n_frames,
                (1 << self.kind) | (0x80000000 if self.frame_tables else 0), self.stream)

    def step(self):
        rc = self.L.mspack_hip_decode_batch_device(*self._args())
        if rc:
            raise RuntimeError(self.L.mspack_hip_last_error().decode())

    def kernel_ms(self, iters):
        ms = self.L.mspack_hip_time_batch_device(*(self._args() + (iters,)))
        self.torch.cuda.synchronize()
        if ms < 0:
            raise RuntimeError("mspack_hip_time_batch_device failed")
        return ms

    def results(self):
        return self.d_res.cpu().numpy().view(self.M.RESULT_DTYPE)

    def output(self):
        return self.d_out.cpu().numpy()


def roofline(algo_bytes, ms, kernel, **extra):
    gbs = algo_bytes / (ms * 1e-3) / 1e9
    d = {"bound": "hbm", "achieved": round(gbs, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": round(gbs / HBM_PEAK_GBS, 5), "kernel": kernel, "kernel_ms": round(ms, 4),
         "algorithmic_bytes_per_launch": int(algo_bytes)}
    d.update(extra)
    return d


DUMP_MAX_UNITS = 1 << 16        # per-unit arrays: 64 B a unit (float64) -> at most 4 MiB
DUMP_SAMPLE_BYTES = 1 << 22     # decoded bytes kept as float32 -> 16 MiB


def dump_outputs(d, batch, units):
    """--dump-outputs DIR: what the timed path (mspack_hip_decode_batch_device) handed its caller in the last step, as .npy files --
    result_<field>.npy: every field of the results array (float64; a seeded sample of DUMP_MAX_UNITS units beyond that many);
    unit_checksums.npy: per unit of the same units, [sum of its decoded bytes, sum of byte x (1-based position)] (float64, exact);
    output_sample.npy: a seeded sample of DUMP_SAMPLE_BYTES of all decoded bytes (float32), sorted by position.
    The whole output (256 MiB at the defaults) is too large to keep; the checksums still see every byte."""
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(0x5EED)
    n = len(units)
    keep = np.arange(n) if n <= DUMP_MAX_UNITS else np.sort(rng.choice(n, DUMP_MAX_UNITS, replace=False))
    res = batch.results()[keep]
    for f in res.dtype.names:
        np.save(os.path.join(d, "result_%s.npy" % f), res[f].astype(np.float64))
    out = batch.output()
    oo, ol = units["out_off"].astype(np.int64), units["out_len"].astype(np.int64)
    pos = np.arange(1, int(ol.max()) + 1, dtype=np.float64)
    sums = np.zeros((len(keep), 2))
    for k, i in enumerate(keep):
        seg = out[oo[i]:oo[i] + ol[i]]
        sums[k] = seg.sum(dtype=np.float64), np.dot(seg, pos[:ol[i]])
    np.save(os.path.join(d, "unit_checksums.npy"), sums)
    total = int(ol.sum())
    flat = np.sort(rng.integers(0, total, min(total, DUMP_SAMPLE_BYTES)))
    starts = np.cumsum(ol) - ol
    u = np.searchsorted(starts, flat, side="right") - 1
    np.save(os.path.join(d, "output_sample.npy"), out[oo[u] + flat - starts[u]].astype(np.float32))


def secondary_mszip(M, torch, dev, n=4096, ub=32768, iters=10, cpu=True):
    """BASELINE config 2: n independent MSZIP CFDATA blocks ('CK' + raw deflate, zlib level 6), one per unit"""
    import zlib
    plain = M.gen_plaintext(0xC0FFEE, 0, n * ub)
    parts, offs, lens, pos = [], [], [], 0
    for i in range(n):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        blob = b"CK" + co.compress(plain[i * ub:(i + 1) * ub].tobytes()) + co.flush()
        pad = (-len(blob)) % 16
        offs.append(pos); lens.append(len(blob)); parts.append(blob + b"\0" * pad); pos += len(blob) + pad
    comp = np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8).copy()
    off = np.array(offs, dtype=np.uint64); ln = np.array(lens, dtype=np.uint32)
    # every unit carries its block table -- where its CFDATA blocks start, which a cabinet states (cabd.c:1362-1479) --
    # here one entry, 0: all units share one zero dword behind the arena's last block
    ztab = np.full(n, (pos + 15) & ~15, dtype=np.uint64)
    units, out_bytes = M.make_units(M.KIND_MSZIP, off, ln, np.full(n, ub), out_slack=32768, frame_tabs=ztab)
    b = DeviceBatch(M, torch, dev, units, comp, out_bytes, M.KIND_MSZIP)
    b.step(); torch.cuda.synchronize()
    ms = b.kernel_ms(iters)
    res, out = b.results(), b.output()
    oo = units["out_off"].astype(np.int64)
    ok = bool((res["err"] == 0).all()) and all(np.array_equal(out[oo[i]:oo[i] + ub], plain[i * ub:(i + 1) * ub]) for i in range(n))
    adopted = float(((res["flags"] & M.F_FRAMES_ADOPTED) != 0).mean())
    # the same units without tables: one wavefront per unit does everything (round 2's launch)
    u0, _ = M.make_units(M.KIND_MSZIP, off, ln, np.full(n, ub), out_slack=32768)
    b0 = DeviceBatch(M, torch, dev, u0, comp, out_bytes, M.KIND_MSZIP)
    b0.step(); torch.cuda.synchronize()
    ms0 = b0.kernel_ms(iters)
    return {"config": "BASELINE config 2: %d independent MSZIP CFDATA blocks of %d KiB (zlib level 6), ratio %.3f" %
                      (n, ub // 1024, float(ln.sum()) / (n * ub)),
            "value": round(n * ub / ms / 1e3, 1), "unit": "MB/s", "kernel_ms": round(ms, 4), "bit_exact": ok,
            "units_on_block_parallel_path": adopted, "kernel_ms_without_block_tables": round(ms0, 4),
            "roofline": roofline(float(ln.sum()) + n * ub, ms, "mspack_lzx_frame_map + mspack_mszip_parse + mspack_decode_mszip"),
            "cpu_baseline": ref_cpu_secondary(1, comp, off, ln, np.full(n, ub), 0, 0) if cpu else None}


def secondary_qtm(M, torch, dev, n=512, frames=32, window_bits=21, iters=2, cpu=True, marks=0):
    """BASELINE config 4 as SURVEY 8(d) specifies it: comp_type 0x1572 -- Quantum, window 2^21 -- n folders of
    `frames` 32 KiB blocks each (the folder stream as cabd feeds it: every block followed by the 0xFF trailer)"""
    from concurrent.futures import ThreadPoolExecutor
    ub = frames * 32768
    plain = M.gen_plaintext(0xC0FFEE, 0, n * ub)

    def enc(i):
        st, _fs = M.qtm_encode(plain[i * ub:(i + 1) * ub], window_bits)
        return bytes(st)
    with ThreadPoolExecutor(max_workers=usable_cpus()) as ex:
        blobs = list(ex.map(enc, range(n)))
    parts, offs, lens, pos = [], [], [], 0
    for blob in blobs:
        pad = (-len(blob)) % 16
        offs.append(pos); lens.append(len(blob)); parts.append(blob + b"\0" * pad); pos += len(blob) + pad
    if marks:       # (tools/bench_qtm_config4.py: every folder with a table of marks, as the cabinet driver's folders carry -- MSPACK_HIP_UF_QTM_MARKS)
        tab = np.sort(np.random.default_rng(1).integers(1, ub, marks)).astype(np.uint32).tobytes()
        tab_off = pos; parts.append(tab)
    comp = np.frombuffer(b"".join(parts) + b"\0" * 64, dtype=np.uint8).copy()
    off = np.array(offs, dtype=np.uint64); ln = np.array(lens, dtype=np.uint32)
    units, out_bytes = M.make_units(M.KIND_QUANTUM, off, ln, np.full(n, ub), window_bits=window_bits, out_slack=(16 + 4 * marks) if marks else 0)
    if marks:
        units["flags"] |= M.UF_QTM_MARKS; units["in_chunk"] = tab_off // 4; units["ref_len"] = marks
    b = DeviceBatch(M, torch, dev, units, comp, out_bytes, M.KIND_QUANTUM)
    b.step(); torch.cuda.synchronize()
    ms = b.kernel_ms(iters)
    res, out = b.results(), b.output()
    oo = units["out_off"].astype(np.int64)
    ok = bool((res["err"] == 0).all()) and all(np.array_equal(out[oo[i]:oo[i] + ub], plain[i * ub:(i + 1) * ub]) for i in range(n))
    return {"config": "BASELINE config 4: %d Quantum folders (comp_type 0x1572: window 2^%d), %d blocks = %d KiB each, ratio %.3f" %
                      (n, window_bits, frames, ub // 1024, float(ln.sum()) / (n * ub)),
            "value": round(n * ub / ms / 1e3, 1), "unit": "MB/s", "kernel_ms": round(ms, 4), "bit_exact": ok,
            "roofline": roofline(float(ln.sum()) + n * ub, ms, "mspack_decode_qtm"),
            "cpu_baseline": ref_cpu_secondary(2, comp, off, ln, np.full(n, ub), window_bits, 0) if cpu else None}


def secondary_lzx(M, torch, dev, what, n, ub, seed, first_unit=0, iters=10, threads=1, block_size=0):
    """another LZX launch shape (BASELINE configs 3 and 5): n CHM-style reset intervals of ub bytes, window 2^21, frame tables.
    block_size: uncompressed bytes per LZX block (0: this build's encoder's default, one block per 32 KiB frame; real encoders
    write blocks that span frames -- the parse tasks then carry the open block from frame to frame)"""
    plain, comp, off, ln, tab = M.corpus_lzx_units(seed, 0, n, ub, 21, opts=M.lzx_opts(block_size=block_size) if block_size else None,
                                                   n_threads=threads, first_unit=first_unit, frame_tables=True)
    units, out_bytes = M.make_units(M.KIND_LZX, off, ln + 4, np.full(n, ub), window_bits=21, reset_frames=ub // 32768, frame_tabs=tab)
    b = DeviceBatch(M, torch, dev, units, comp, out_bytes, M.KIND_LZX)
    b.step(); torch.cuda.synchronize()
    ms = b.kernel_ms(iters)
    res, out = b.results(), b.output()[:n * ub]
    ok = bool((res["err"] == 0).all() and (res["out_len"] == ub).all() and np.array_equal(out, plain))
    return {"config": what + ", ratio %.3f" % (float(ln.sum()) / (n * ub)),
            "value": round(n * ub / ms / 1e3, 1), "unit": "MB/s", "kernel_ms": round(ms, 4), "bit_exact": ok,
            "units_on_frame_parallel_path": round(float(((res["flags"] & M.F_FRAMES_ADOPTED) != 0).mean()), 4),
            "roofline": roofline(float(ln.sum()) + n * ub, ms, LZX_KERNELS)}


def secondary_one_folder(M, torch, dev, kind, frames=512, seed=77, iters=3, cpu=True):
    """ONE folder of ordinary data: the text corpus as a single cabinet folder -- LZX-21 with blocks of
    4 MiB (what Microsoft's encoder writes), or MSZIP with history -- `frames` CFDATA blocks, block table passed.  Nothing here is
    independent but the parse: the folder's copies are a chain from frame to frame (mspack_lzx_fold / mspack_mszip_fold:
    lzx_fold.hpp).  The reference codec on ONE host core beside it: what a user of one folder would otherwise have."""
    import zlib
    n = frames * 32768
    plain = M.gen_plaintext(seed, 0, n)
    if kind == M.KIND_LZX:
        lz, fo = M.lzx_encode(plain, 21, 0, M.lzx_opts(block_size=4 << 20))
        stream, tab, wb, what = lz.tobytes(), np.asarray(fo[:-1]), 21, "LZX-21, blocks of 4 MiB"
    else:
        blocks, prev = [], None
        for k in range(0, n, 32768):
            b = plain[k:k + 32768].tobytes()
            c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, 0, prev) if prev else zlib.compressobj(6, zlib.DEFLATED, -15)
            blocks.append(b"CK" + c.compress(b) + c.flush()); prev = b
        stream, tab, wb, what = b"".join(blocks), np.cumsum([0] + [len(b) for b in blocks[:-1]]), 0, "MSZIP (zlib level 6, history)"
    base = (len(stream) + 64 + 15) & ~15
    arena = np.zeros(base + 4 * len(tab) + 64, dtype=np.uint8)
    arena[:len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    arena[base:base + 4 * len(tab)] = np.asarray(tab, dtype=np.uint32).view(np.uint8)
    units, out_bytes = M.make_units(kind, [0], [len(stream)], [n], window_bits=wb, reset_frames=0, frame_tabs=[base],
                                    out_slack=32768 if kind == M.KIND_MSZIP else 0)
    b = DeviceBatch(M, torch, dev, units, arena, out_bytes, kind)
    b.step(); torch.cuda.synchronize()
    ms = b.kernel_ms(iters)
    res, out = b.results(), b.output()[:n]
    ok = bool(res["err"][0] == 0 and res["out_len"][0] == n and np.array_equal(out, plain))
    off, ln = np.zeros(1, dtype=np.uint64), np.asarray([len(stream)], dtype=np.uint32)
    return {"config": "ONE cabinet folder of %d blocks (%d MiB of the text corpus), %s, ratio %.3f" % (frames, n >> 20, what, len(stream) / n),
            "value": round(n / ms / 1e3, 1), "unit": "MB/s", "kernel_ms": round(ms, 3), "bit_exact": ok,
            "units_on_frame_parallel_path": round(float(((res["flags"] & M.F_FRAMES_ADOPTED) != 0).mean()), 4),
            "roofline": roofline(float(len(stream)) + n, ms, "the launches of one mspack_hip_decode_batch_device call (parse, fold, unit kernel)"),
            "cpu_baseline": ref_cpu_secondary(0 if kind == M.KIND_LZX else 1, arena, off, ln, np.asarray([n]), wb, 0, budget_s=4.0) if cpu else None}


class _HipBuf:
    """device memory through the HIP runtime the library is linked with (no torch)"""

    def __init__(self, M, nbytes):
        import ctypes as C
        M.lib()
        self.C = C
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        p = C.c_void_p()
        if self.hip.hipMalloc(C.byref(p), nbytes):
            raise RuntimeError("hipMalloc failed")
        self.ptr, self.n = p.value, nbytes

    def to_host(self, out):
        if self.hip.hipMemcpy(out.ctypes.data, self.ptr, out.size, 2):
            raise RuntimeError("hipMemcpy D2H failed")

    def from_host(self, src):
        if self.hip.hipMemcpy(self.ptr, src.ctypes.data, src.size, 1):
            raise RuntimeError("hipMemcpy H2D failed")


def host_inclusive(M, units, comp, out_bytes, plain, n, ub, reps=5, torch=None, dev=None):
    """SURVEY 8(d)'s metric as written: compressed units in (pageable) HOST memory -> decoded bytes in device
    memory, and -> decoded bytes back in host memory; the host-buffer entry points the C drivers call.
    torch=None: device memory through the library's own HIP runtime (the clean-process worker)."""
    L = M.lib()
    u = np.ascontiguousarray(units.copy())
    res = np.zeros(n, dtype=M.RESULT_DTYPE)
    if torch is None:
        d_buf = _HipBuf(M, out_bytes + 64); d_ptr = d_buf.ptr
    else:
        d_out = torch.zeros(out_bytes + 64, dtype=torch.uint8, device=dev); d_ptr = d_out.data_ptr()
    h_out = np.zeros(out_bytes + 64, dtype=np.uint8)            # written once here: pages exist (a reused buffer)

    def to_dev():
        rc = L.mspack_hip_decode_batch_to_device(u.ctypes.data, n, comp.ctypes.data, comp.size, d_ptr,
                                                 out_bytes + 64, res.ctypes.data)
        if rc:
            raise RuntimeError(L.mspack_hip_last_error().decode())

    def to_host():
        rc = L.mspack_hip_decode_batch(u.ctypes.data, n, comp.ctypes.data, comp.size, h_out.ctypes.data,
                                       out_bytes + 64, res.ctypes.data)
        if rc:
            raise RuntimeError(L.mspack_hip_last_error().decode())

    def best(fn):
        fn()                                                    # grows the persistent context
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        return min(ts), sum(ts) / len(ts)
    bd, md = best(to_dev)
    if torch is None:
        back = np.empty(n * ub, dtype=np.uint8); d_buf.to_host(back)
    else:
        back = d_out[:n * ub].cpu().numpy()
    ok_d = bool((res["err"] == 0).all()) and np.array_equal(back, plain)
    bh, mh = best(to_host)
    ok_h = bool((res["err"] == 0).all()) and np.array_equal(h_out[:n * ub], plain)
    tot = n * ub
    r = {"MBps": round(tot / md / 1e6, 1), "MBps_best": round(tot / bd / 1e6, 1), "ms": round(md * 1e3, 3),
         "what": "mspack_hip_decode_batch_to_device: pageable host input -> decoded bytes in HBM (mean of %d calls)" % reps,
         "to_host_MBps": round(tot / mh / 1e6, 1), "to_host_MBps_best": round(tot / bh / 1e6, 1),
         "to_host_ms": round(mh * 1e3, 3),
         "to_host_what": "mspack_hip_decode_batch: ... -> decoded bytes in (pageable, already touched) host memory",
         "bit_exact": bool(ok_d and ok_h)}
    if torch is None:
        # the bare copies of the same arenas, for scale (pageable host memory, synchronous hipMemcpy)
        d_in = _HipBuf(M, comp.size)
        d_in.from_host(comp)
        t0 = time.perf_counter(); d_in.from_host(comp); h2d = time.perf_counter() - t0
        tmp = np.zeros(out_bytes, dtype=np.uint8)
        d_buf.to_host(tmp)
        t0 = time.perf_counter(); d_buf.to_host(tmp); d2h = time.perf_counter() - t0
        r.update({"h2d_ms": round(h2d * 1e3, 3), "d2h_ms": round(d2h * 1e3, 3), "h2d_MB": round(comp.size / 1e6, 1),
                  "d2h_MB": round(out_bytes / 1e6, 1)})
    return r


def host_path_worker(args):
    """bench.py --host-path-worker: the host-buffer entry points in a process that holds nothing but the library (as a C
    program linked with it does): no torch, so ONE HIP runtime and only the library's own streams.  Prints one JSON object."""
    import libmspack_amd as M
    from libmspack_amd import dist as D
    n, ub = args.units, args.unit_kib * 1024
    plain, comp, off, ln, tab = M.corpus_lzx_units(D.unit_seed_base(0xBA5E11, 0), args.text, n, ub, 21,
                                                   n_threads=max(1, usable_cpus()), frame_tables=True)
    units, out_bytes = M.make_units(M.KIND_LZX, off, ln + 4, np.full(n, ub), window_bits=21, reset_frames=ub // 32768,
                                    frame_tabs=tab)
    r = host_inclusive(M, units, comp, out_bytes, plain, n, ub)
    r["process"] = "a separate process holding only the library (one HIP runtime, the library's own streams)"
    del plain, comp, units
    if not args.no_api:
        r["through_api"] = through_api(M)
    print(json.dumps(r), flush=True)


def through_api(M, reps=3):
    """BASELINE configs 2, 3 and 4 as CONTAINERS through the API the north star names -- mspack_create_cab/chm_decompressor() ->
    open() -> extract() of every file -- driven from C with an in-memory mspack_system (libmspack_amd/csrc/bench/api_bench.c):
    MB/s of extracted bytes over the whole run, and where the time goes.  Every byte is compared with the plaintext."""
    from libmspack_amd import apibench as A
    out = {}

    def measure(key, kind, image, plain, check):
        runs = []
        ok = True
        for k in range(reps + 1):                     # (the first run grows the library's persistent buffers)
            rc, o, offs, d = A.run(kind, image, plain.size)
            ok = ok and rc == 0 and d["n_errors"] == 0 and check(o, offs)
            if k:
                runs.append(d)
        best = min(runs, key=lambda d: d["total_s"])
        s = A.summary(best, "; best of %d runs, mean %.1f MB/s" % (reps, float(np.mean([d["bytes_out"] / d["total_s"] / 1e6 for d in runs]))))
        s["bit_exact"] = bool(ok)
        s["container_bytes"] = len(image)
        out[key] = s
    try:
        cab, plain = A.build_config2_cab(M)
        measure("config 2", "cab", cab, plain, lambda o, offs: np.array_equal(o, plain))
        out["config 2"]["container"] = "ONE cabinet: 4096 MSZIP folders of one 32 KiB CFDATA block, 4096 files"
        chm, plain, slices = A.build_config3_chm(M, threads=max(1, usable_cpus()))
        measure("config 3", "chm", chm, plain,
                lambda o, offs: all(np.array_equal(o[int(offs[k]):int(offs[k + 1])], plain[a:a + l]) for k, (a, l) in enumerate(slices)))
        out["config 3"]["container"] = "ONE CHM: 1024 LZX reset intervals of 64 KiB (window 2^21, reset every 2 frames), %d files" % len(slices)
        cab, plain = A.build_config4_cab(M)
        measure("config 4", "cab", cab, plain, lambda o, offs: np.array_equal(o, plain))
        out["config 4"]["container"] = "ONE cabinet: 512 Quantum folders (window 2^21) of 32 CFDATA blocks, 512 files"
    except Exception as ex:          # pragma: no cover
        out["error"] = str(ex)
    return out


def run_host_path_worker(args):
    """-> the worker's JSON object, or an object that says why there is none"""
    cmd = [sys.executable, os.path.abspath(__file__), "--host-path-worker", "--units", str(args.units),
           "--unit-kib", str(args.unit_kib), "--text", str(args.text)] + (["--no-api"] if args.no_api else [])
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        if p.returncode:
            return {"error": "worker exit code %d: %s" % (p.returncode, p.stderr.decode()[-400:])}
        return json.loads(p.stdout.decode().strip().splitlines()[-1])
    except Exception as ex:          # pragma: no cover
        return {"error": str(ex)}


def spawn_ranks(args):
    """--gpus N without a launcher: start the N ranks ourselves (one process per GPU)."""
    import socket
    import torch
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < args.gpus:
        raise SystemExit("bench.py --gpus %d: this box has %d GPU(s); refusing to report a %d-GPU line from fewer devices"
                         % (args.gpus, have, args.gpus))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rcs = [p.wait() for p in procs]
    if any(rcs):
        raise SystemExit("bench.py: rank exit codes %s" % rcs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--units", type=int, default=4096, help="reset intervals per GPU (weak scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--total-units", type=int, default=65536, help="strong scaling: intervals in the global list (BASELINE config 5)")
    ap.add_argument("--unit-kib", type=int, default=64)
    ap.add_argument("--text", type=int, default=0, help="plaintext family (0 = mix)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-frame-tables", action="store_true",
                    help="units without frame tables: the serial kernel only.  Default: every unit carries its frame table (as a "
                         "CHM's reset table states it per frame) and the launch is mspack_lzx_pipe: parse tasks and commit tasks "
                         "from one ticket counter, then the unit kernel for the last bytes of every unit")
    ap.add_argument("--no-extras", action="store_true", help="skip host_inclusive and the secondary configs")
    ap.add_argument("--host-path-worker", action="store_true", help="internal: the host_inclusive measurement in a process of its own")
    ap.add_argument("--no-api", action="store_true", help="skip through_api (containers through the object API) in the worker")
    ap.add_argument("--exp", action="store_true", help="kernel experiments: skip the parity gate and the CPU leg (the line is then NOT a valid result)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: every byte against the plaintext, the roofline and the spread of single launches, "
                         "host_inclusive, the secondary configs and the CPU baseline (--no-extras / --no-cpu drop parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last step computed (rank 0) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.host_path_worker:
        return host_path_worker(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(args)
    # SURVEY 8(d)'s host-inclusive figures come from a process that holds only the library -- what a C program linked with
    # it is -- and it runs FIRST, before this process initialises torch's own copy of the HIP runtime: with two runtimes'
    # queues on the device the chunks' launches of the host path time-share hardware queues (measured: 8.2 ms instead of
    # 4.0 for the same call, profiles/round3_hostpath.txt).  The same calls made from this process are reported beside it.
    host_clean = None
    if args.full and args.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and not args.exp and not args.no_extras \
            and args.scaling == "weak" and not args.no_frame_tables:
        host_clean = run_host_path_worker(args)

    import torch
    import libmspack_amd as M
    from libmspack_amd import dist as D
    rank, world, local = D.env_rank_world()
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s); refusing to print a line whose n_gpus "
                         "differs from the request" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback exists)")
    if local >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d wants GPU %d but this box has %d" % (rank, local, torch.cuda.device_count()))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = D.init("nccl", dev)

    ub = args.unit_kib * 1024
    threads = max(1, usable_cpus() // max(world, 1))
    t0 = time.perf_counter()
    if args.scaling == "strong":
        lo, hi = D.shard_range(args.total_units, rank, world)      # contiguous shard of ONE global list
        n = hi - lo
        plain, comp, off, ln, tab = M.corpus_lzx_units(0xC0F165, args.text, n, ub, 21, n_threads=threads, first_unit=lo,
                                                       frame_tables=True)
    else:
        n = args.units                                             # every rank its own corpus: fixed work per GPU
        plain, comp, off, ln, tab = M.corpus_lzx_units(D.unit_seed_base(0xBA5E11, rank), args.text, n, ub, 21,
                                                       n_threads=threads, frame_tables=True)
    gen_s = time.perf_counter() - t0
    # every unit carries its frame table (where each 32 KiB frame starts in the compressed stream), as a CHM's
    # reset table states it per frame (chmd.c:1146-1149): the frames' tokens are parsed by one wavefront each
    units, out_bytes = M.make_units(M.KIND_LZX, off, ln + 4, np.full(n, ub), window_bits=21, reset_frames=ub // 32768,
                                    frame_tabs=None if args.no_frame_tables else tab)
    batch = DeviceBatch(M, torch, dev, units, comp, out_bytes, M.KIND_LZX)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        batch.step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        batch.step()
    barrier()
    my_elapsed = time.perf_counter() - t0
    elapsed, total_out = D.reduce_scalars(dist, dev, my_elapsed, float(n * ub))
    per_rank_ms = D.gather_scalar(dist, dev, my_elapsed / args.steps * 1e3)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, batch, units)

    if args.full:
        ms_kernel = batch.kernel_ms(max(3, min(args.steps, 10)))       # roofline numerator: HIP events on the launch stream
        singles = sorted(batch.kernel_ms(1) for _ in range(7))          # spread of single launches (outside the timed region)
        step_spread = [round(singles[0], 4), round(singles[len(singles) // 2], 4), round(singles[-1], 4)]

    # ---- parity, outside the timed region: every unit's result; with --full every byte too ----
    res = batch.results()
    ok = bool((res["err"] == 0).all() and (res["out_len"] == ub).all())
    if args.full:
        ok = ok and np.array_equal(batch.output()[:n * ub], plain)
    adopted = float(((res["flags"] & M.F_FRAMES_ADOPTED) != 0).mean())
    all_ok = D.all_true(dist, dev, ok)
    if not all_ok and not args.exp:
        raise SystemExit("rank %d: GPU output is NOT %s on some rank; refusing to report a number" %
                         (rank, "bit-exact" if args.full else "free of unit errors"))

    comp_bytes = float(ln.sum())
    algo_bytes = comp_bytes + n * ub                      # in + out, per launch
    # HBM traffic per launch: PMC counters cannot be collected from inside this process; the latest rocprofv3
    # --pmc FETCH_SIZE / WRITE_SIZE passes of the same workload are kept in profiles/traffic.json
    traffic, traffic_source = None, None
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        w = tj["workload"]
        if (w["units_per_gpu"], w["unit_bytes"], w["text"]) == (n, ub, args.text) and args.scaling == "weak":
            traffic = int((tj["fetch_kib_per_launch"] * tj.get("fetch_correction", 1.0) + tj["write_kib_per_launch"]) * 1024)
            traffic_source = "profiles/traffic.json (rocprofv3 --pmc passes of this workload, %s; replayed, not measured in this run)" % tj.get("round", "earlier round")
    except Exception:
        traffic = None
    if rank == 0:
        if args.scaling == "strong":
            wl = ("BASELINE config 5: CHM-style LZX, window_bits=21, reset interval %d frames (%d KiB), %d intervals in one "
                  "global list sharded contiguously over %d GPU(s) (%d on rank 0), plaintext family %d" %
                  (ub // 32768, args.unit_kib, args.total_units, world, n, args.text))
        else:
            wl = ("CHM-style LZX, window_bits=21, reset interval %d frames (%d KiB), %d intervals per GPU, plaintext family "
                  "%d, ratio %.3f" % (ub // 32768, args.unit_kib, n, args.text, comp_bytes / (n * ub)))
        line = {
            "metric": METRIC,
            "value": round(total_out * args.steps / elapsed / 1e6, 1),
            "unit": "MB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "u8", "data": "synthetic",
            "config": {"workload": wl, "units_per_gpu": n, "unit_bytes": ub,
                       "frame_tables": "off (serial kernel)" if args.no_frame_tables else "on (mspack_lzx_pipe)",
                       "residency": "value: compressed units and decoded bytes resident in HBM; host_inclusive: the same batch from host memory",
                       "units_on_frame_parallel_path": round(adopted, 4),
                       "corpus_gen_s": round(gen_s, 2), "per_rank_ms_per_step": [round(x, 4) for x in per_rank_ms],
                       "launcher": "torchrun" if "TORCHELASTIC_RUN_ID" in os.environ else ("self-spawned" if world > 1 else "single")},
        }
        if args.full:
            line["config"]["bit_exact"] = all_ok
            line["config"]["step_ms_min_median_max"] = step_spread
            line["roofline"] = roofline(algo_bytes, ms_kernel, LZX_KERNELS if adopted > 0.5 else "mspack_decode_lzx",
                                        traffic=traffic, traffic_source=traffic_source)
        extras = args.full and world == 1 and not args.exp and not args.no_extras
        if extras:
            inproc = host_inclusive(M, units, comp, out_bytes, plain, n, ub, torch=torch, dev=dev)
            if host_clean and "MBps" in host_clean:
                line["host_inclusive"] = host_clean
                line["host_inclusive"]["same_calls_from_this_process"] = {
                    k: inproc[k] for k in ("MBps", "ms", "to_host_MBps", "to_host_ms", "bit_exact")}
                line["host_inclusive"]["same_calls_from_this_process"]["note"] = \
                    "this process also holds torch's copy of the HIP runtime and its queues"
            else:
                line["host_inclusive"] = inproc
                line["host_inclusive"]["process"] = "the bench process (torch's HIP runtime beside the library's)"
                if host_clean:
                    line["host_inclusive"]["clean_process_error"] = host_clean.get("error")
        del batch
        torch.cuda.empty_cache()
        cpu = args.full and world == 1 and not args.no_cpu and not args.exp
        if extras:
            lo5, hi5 = D.shard_range(65536, 0, 8)
            line["secondary"] = [
                secondary_lzx(M, torch, dev, "BASELINE config 3's launch shape: 1024 LZX reset intervals of 64 KiB (window 2^21)", 1024, ub,
                              0xBA5E11, threads=threads),
                secondary_lzx(M, torch, dev, "BASELINE config 5, rank 0's shard of 8: %d of 65536 LZX reset intervals of 64 KiB in one "
                              "launch (strong-scaling seeding)" % (hi5 - lo5), hi5 - lo5, ub, 0xC0F165, first_unit=lo5, threads=threads),
                secondary_mszip(M, torch, dev, cpu=cpu), secondary_qtm(M, torch, dev, cpu=cpu),
                # what real containers look like: LZX blocks that span frames; one long folder per codec
                secondary_lzx(M, torch, dev, "config 3's launch shape with LZX blocks that SPAN frames (one block of 64 KiB per reset interval, "
                              "as real encoders write them): 1024 LZX reset intervals of 64 KiB (window 2^21)", 1024, ub, 0xBA5E12,
                              threads=threads, block_size=65536),
                secondary_one_folder(M, torch, dev, M.KIND_LZX, cpu=cpu), secondary_one_folder(M, torch, dev, M.KIND_MSZIP, cpu=cpu)]
            ta = (host_clean or {}).pop("through_api", None) if isinstance(host_clean, dict) else None
            if "host_inclusive" in line:
                line["host_inclusive"].pop("through_api", None)
            if ta:
                for sec in line["secondary"]:
                    for key in ("config 2", "config 3", "config 4"):
                        if ("BASELINE " + key) in sec["config"] and key in ta:
                            sec["through_api"] = ta[key]
                            hi = line.get("host_inclusive", {}).get("to_host_MBps")
                            if hi:
                                sec["through_api"]["vs_host_inclusive_to_host"] = round(ta[key]["MBps"] / hi, 3)
                if "error" in ta:
                    line["through_api_error"] = ta["error"]
        if extras and "MBps" in line.get("host_inclusive", {}):
            # SURVEY 8(d) defines the metric from compressed units in HOST memory: the same batch by that definition, at the top level
            # beside `value` (which the bench contract wants HBM-resident)
            line["value_host_inclusive"] = line["host_inclusive"]["MBps"]
            line["value_host_to_host"] = line["host_inclusive"].get("to_host_MBps")
        if cpu:
            line["cpu_baseline"] = cpu_baseline(comp, off, ln, n, ub)
            cb = line["cpu_baseline"]
            if cb:
                cb["lscpu"] = lscpu_summary()
            if cb and cb.get("value"):
                line["vs_cpu_baseline"] = {"device_resident": round(line["value"] / cb["value"], 2),
                                           "host_to_device": round(line["host_inclusive"]["MBps"] / cb["value"], 2) if extras else None,
                                           "host_to_host": round(line["host_inclusive"]["to_host_MBps"] / cb["value"], 2) if extras else None,
                                           "note": "against %d host threads (the container's CPU quota), not a whole socket" % cb["cores"]}
                cps = cores_per_socket()
                if cps and cb.get("one_core_MBps"):
                    est = cb["one_core_MBps"] * cps
                    line["vs_cpu_baseline"]["single_socket_estimate"] = {
                        "physical_cores_per_socket": cps, "MBps": round(est, 1), "device_resident": round(line["value"] / est, 2),
                        "host_to_device": round(line["host_inclusive"]["MBps"] / est, 2) if extras else None,
                        "what": "ESTIMATE, not measured: one_core_MBps x the physical cores of one socket (lscpu); the quota of %d CPUs "
                                "does not allow the measurement.  The north star's target is 10x THIS" % cb["cores"]}
        else:
            line["cpu_baseline"] = None
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
