"""Per-file MD5 / SHA-1 / SHA-256 of a CHM's members through mspack_chmd_digest() against what a caller had to do before it existed:
python tools/chm_digest_bench.py [N_FILES=4096] [REPS=5] [OUT=profile file to write]
Workload: ONE recipe CHM built with the corpus writers (libmspack_amd/csrc/corpus; apibench.build_config3_chm): 1024 LZX reset
intervals of 64 KiB, window 2^21 -- 64 MiB, one chunk of the driver, one GPU batch -- tiled by N_FILES section-1 files of unequal
length (about 16 KiB each at 4096).  C in-memory mspack_system (libmspack_amd/csrc/bench/api_bench.c: no Python inside a call).
Legs per algorithm, run in turn, REPS times each after one warm-up of each, wall time around the whole session (create .. destroy):
  on        digest() of every file in list order, the algorithm's bit of MSCHMD_PARAM_HIP_DIGESTS set (digests from the device where
            the planner gives a file a unit);
  off       digest() of every file, the param 0 (the plain-C hash on the host);
  extract   extract() of every file into memory, then hashlib per file -- inside the timed region: the baseline, what a CHM caller
            had before.
Every leg's digests are compared with hashlib's over the plaintext.  One JSON line: min / median / max per leg in ms, the
device / host counts of the last session of each leg, whether on's slowest repetition beat extract's fastest, and where an `on`
session's time goes (the first call -- the batch with its digest pass -- against the rest)."""
import ctypes as C, hashlib, json, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import libmspack_amd as M
from libmspack_amd import apibench as A

ALGS = (("md5", 1, hashlib.md5), ("sha1", 2, hashlib.sha1), ("sha256", 4, hashlib.sha256))


def stats(v):
    return {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}


def main(n_files, reps, out_path):
    image, plain, files = A.build_config3_chm(M, n=1024, ub=65536, n_files=n_files)
    total = int(plain.size)
    buf = plain.tobytes()
    L = A.lib()
    L.mspack_chmd_digest_counts.argtypes = [C.c_int, C.c_void_p, C.c_int]
    res = {"n_files": n_files, "section1_bytes": total, "mean_file_bytes": total // n_files,
           "max_file_bytes": max(ln for _o, ln in files), "reps": reps, "sessions_per_leg": reps + 1}
    for name, alg, h in ALGS:
        want = [h(buf[o:o + ln]).digest() for o, ln in files]
        legs = {"on": [], "off": [], "extract": []}
        counts, first_ms = {}, []
        for k in range(reps + 1):
            for leg in legs:
                L.mspack_chmd_digest_counts(alg, None, 1)
                t0 = time.perf_counter()
                if leg == "extract":
                    rc, out, offs, d = A.run("chm", image, total, max_files=n_files)
                    got = [h(out[int(offs[i]):int(offs[i + 1])]).digest() for i in range(n_files)]
                else:
                    rc, got, d = A.run_chm_digest(image, alg if leg == "on" else 0, alg, max_files=n_files)
                ms = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and d["n_errors"] == 0 and d["n_files"] == n_files and got == want, (name, leg, rc, d)
                c = (C.c_ulonglong * 2)(); L.mspack_chmd_digest_counts(alg, c, 0)
                counts[leg] = [int(c[0]), int(c[1])]
                if k:
                    legs[leg].append(ms)
                    if leg == "on":
                        first_ms.append(d["first_extract_s"] * 1e3)
        res[name] = {leg: stats(v) for leg, v in legs.items()}
        res[name]["digests_from_device_and_host"] = counts
        res[name]["on_first_call_ms"] = stats(first_ms)
        res[name]["on_slowest_beats_extract_fastest"] = max(legs["on"]) < min(legs["extract"])
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 5,
         sys.argv[3] if len(sys.argv) > 3 else None)
