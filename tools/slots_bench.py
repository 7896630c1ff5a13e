#!/usr/bin/env python3
"""Context slots (include/mspack_hip.h: mspack_hip_set_slots): the aggregate decoded GB/s of T application threads, T = 1, 2, 4, with
1, 2 and 4 slots.  Every thread has containers of its own -- a CHM of 256 LZX-21 reset intervals of 64 KiB and a cabinet of 1024
MSZIP folders of one 32 KiB block, both small beside the chip on purpose -- and opens and extracts every file of both through the
object API, driven from C with an in-memory mspack_system (libmspack_amd/csrc/bench/api_bench.c; ctypes gives the GIL up for the
call, so the threads really run side by side).  A measurement: all threads leave a barrier, each runs --reps rounds of (CHM, cabinet),
the clock stops when the last one is through; GB/s = extracted bytes of all threads / that time.  Every byte of the first (unmeasured)
round is compared with the plaintext.

    python tools/slots_bench.py                  one session: a JSON line with GB/s per (threads, slots)
    python tools/slots_bench.py --sessions 3     three sessions, each a process of its own: min / median / max per cell as a table,
                                                 and the ratio "T threads with min(T, 4) slots / T threads with one slot"
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                   # noqa: E402
import libmspack_amd as M                                            # noqa: E402
from libmspack_amd import apibench as A                              # noqa: E402

THREADS = (1, 2, 4)
SLOTS = (1, 2, 4)


def containers(t):
    """thread t's own CHM and cabinet -> [(kind, image, plain, check)]"""
    chm, cplain, slices = A.build_config3_chm(M, n=256, n_files=31, seed=0xBA5E11 + 977 * t, threads=4)
    zplain = M.gen_plaintext(0xC0FFEE + t, 0, 1024 * 32768)
    cab, zplain = A.build_config2_cab(M, n=1024, plain=zplain)

    def chm_ok(o, offs):
        return all(np.array_equal(o[int(offs[k]):int(offs[k + 1])], cplain[a:a + ln]) for k, (a, ln) in enumerate(slices))
    return [("chm", chm, cplain, chm_ok), ("cab", cab, zplain, lambda o, offs: np.array_equal(o, zplain))]


def measure(sets, n_threads, reps):
    """-> (GB/s over all threads, slot statistics)"""
    bar = threading.Barrier(n_threads + 1)
    bad = []

    def body(t):
        try:
            for kind, image, plain, ok in sets[t]:            # unmeasured: the slot's buffers grow, the bytes are checked
                rc, o, offs, d = A.run(kind, image, plain.size)
                if rc or d["n_errors"] or not ok(o, offs):
                    bad.append((t, kind, rc, d["n_errors"]))
            bar.wait()
            for _ in range(reps):
                for kind, image, plain, _ok in sets[t]:
                    rc, _o, _offs, d = A.run(kind, image, plain.size)
                    if rc or d["n_errors"]:
                        bad.append((t, kind, rc, d["n_errors"]))
            bar.wait()
        except BaseException as e:
            bad.append((t, repr(e)))
            bar.abort()
    th = [threading.Thread(target=body, args=(t,)) for t in range(n_threads)]
    for x in th:
        x.start()
    bar.wait()
    M.slot_stats(reset=True)
    t0 = time.perf_counter()
    bar.wait()
    dt = time.perf_counter() - t0
    for x in th:
        x.join()
    if bad:
        raise SystemExit("slots_bench: %r" % (bad,))
    nbytes = reps * sum(p.size for t in range(n_threads) for _k, _i, p, _c in sets[t])
    return nbytes / dt / 1e9, M.slot_stats()


def session(reps):
    sets = [containers(t) for t in range(max(THREADS))]
    out = {}
    for nt in THREADS:
        for ns in SLOTS:
            M.set_slots(ns)
            gbps, s = measure(sets, nt, reps)
            out["T%d/S%d" % (nt, ns)] = {"GBps": round(gbps, 3), "batches": s[0], "at_once": s[1], "waited": s[2]}
    M.set_slots(1)
    M.lib().mspack_hip_release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="rounds of (CHM, cabinet) per thread and measurement")
    ap.add_argument("--sessions", type=int, default=0, help="run this many sessions, each in a process of its own, and print the table")
    args = ap.parse_args()
    if not args.sessions:
        print(json.dumps(session(args.reps)), flush=True)
        return
    runs = []
    for _ in range(args.sessions):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps)], stdout=subprocess.PIPE, timeout=600)
        if p.returncode:
            raise SystemExit("slots_bench: a session ended with exit code %d" % p.returncode)
        runs.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        print(json.dumps(runs[-1]), flush=True)

    def mmm(v):
        return "%6.3f / %6.3f / %6.3f" % (min(v), statistics.median(v), max(v))
    print("aggregate decoded GB/s, min / median / max of %d sessions (%d rounds each)" % (args.sessions, args.reps))
    print("%-9s" % "threads" + "".join("%-28s" % ("slots = %d" % ns) for ns in SLOTS) + "at once (max), waited (median)")
    for nt in THREADS:
        cells = [[r["T%d/S%d" % (nt, ns)] for r in runs] for ns in SLOTS]
        print("%-9d" % nt + "".join("%-28s" % mmm([c["GBps"] for c in cs]) for cs in cells) +
              "  ".join("S%d: %d, %d" % (ns, max(c["at_once"] for c in cs), statistics.median(c["waited"] for c in cs)) for ns, cs in zip(SLOTS, cells)))
    print("gain: T threads with min(T, 4) slots over T threads with one slot, per session and median")
    for nt in THREADS[1:]:
        ratios = [r["T%d/S%d" % (nt, min(nt, 4))]["GBps"] / r["T%d/S1" % nt]["GBps"] for r in runs]
        print("T = %d: %s   median %.3f" % (nt, "  ".join("%.3f" % x for x in ratios), statistics.median(ratios)))


if __name__ == "__main__":
    main()
