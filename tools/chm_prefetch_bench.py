"""A collection of small CHMs through the object API, with and without mspack_chmd_prefetch():
python tools/chm_prefetch_bench.py [N=1024] [REPS=3] -- N CHMs of two 64 KiB LZX reset intervals each (window 2^16) on ONE decompressor
over the C in-memory mspack_system (libmspack_amd/csrc/bench/api_bench.c: mspk_api_bench_chms):
  extract  (a) open all, extract() every file -- every CHM's first extract() is a batch of its own;
           (b) open all, prefetch(all), the same extracts -- one batch;
  digest   the same two with MSCHMD_PARAM_HIP_DIGESTS = 7 and mspack_chmd_digest() (MD5, SHA-1, SHA-256 in turn over the runs) of
           every file instead of extract().
(a) and (b) run alternately, REPS times each after one warm-up of each.  No ratio is asserted: the line says what was measured, with
mspack_chmd_batch_counts() and the split of mspack_hip_host_path_stats() beside the times."""
import hashlib, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import libmspack_amd as M
from libmspack_amd import api, apibench as A
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
images, plains, lists = A.build_small_chms(M, n)
plain = np.frombuffer(b"".join(plains), dtype=np.uint8)
HASH = {1: hashlib.md5, 2: hashlib.sha1, 4: hashlib.sha256}
ms = lambda runs: [round(d["total_s"] * 1e3, 2) for d in runs]
res = {"n_chms": n, "bytes": int(plain.size), "intervals_per_chm": 2}
for mode in ("extract", "digest"):
    legs = {"a": [], "b": []}
    counts = {}
    for k in range(reps + 1):
        alg = 0 if mode == "extract" else (1, 2, 4)[k % 3]
        for leg, pf in (("a", 0), ("b", 1)):
            api.chmd_batch_counts(reset=True)
            for g in HASH:
                api.chmd_digest_counts(g, reset=True)
            rc, out, d = A.run_chms(images, plain.size, pf, hip_digests=7 if alg else 0, alg=alg)
            assert rc == 0 and d["n_errors"] == 0 and d["n_files"] == sum(len(l) for l in lists), (mode, leg, rc, d)
            if alg:
                want = [HASH[alg](plains[c][off:off + ln]).digest() for c, l in enumerate(lists) for off, ln in l]
                assert out == want, (mode, leg)
            else:
                want = b"".join(plains[c][off:off + ln] for c, l in enumerate(lists) for off, ln in l)
                assert out.tobytes() == want, (mode, leg)
            d["chmd_batch_counts"] = api.chmd_batch_counts()
            d["digests_from_device_and_host"] = [sum(api.chmd_digest_counts(g)[i] for g in HASH) for i in (0, 1)]
            if k:
                legs[leg].append(d)
    res[mode] = {"a_no_prefetch_ms": ms(legs["a"]), "b_prefetch_ms": ms(legs["b"]),
                 "a_batch_calls_units": legs["a"][0]["chmd_batch_counts"], "b_batch_calls_units": legs["b"][0]["chmd_batch_counts"],
                 "a_host_path_calls": legs["a"][0]["lib_calls"], "b_host_path_calls": legs["b"][0]["lib_calls"],
                 "a_digests_from_device_and_host": legs["a"][-1]["digests_from_device_and_host"],
                 "b_digests_from_device_and_host": legs["b"][-1]["digests_from_device_and_host"],
                 "b_prefetch_call_ms": [round(d["first_extract_s"] * 1e3, 2) for d in legs["b"]],
                 "a_best_split": A.summary(min(legs["a"], key=lambda d: d["total_s"])),
                 "b_best_split": A.summary(min(legs["b"], key=lambda d: d["total_s"]))}
print(json.dumps(res))
for mode in ("extract", "digest"):
    r = res[mode]
    print("%s: without the call %s ms (%d batches), with it %s ms (%d batch)" %
          (mode, r["a_no_prefetch_ms"], r["a_batch_calls_units"][0], r["b_prefetch_ms"], r["b_batch_calls_units"][0]))
