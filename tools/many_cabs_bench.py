"""A directory of small cabinets through the object API, with and without mspack_cabd_prefetch():
python tools/many_cabs_bench.py [N=4096] [REPS=3] -- N cabinets of one 32 KiB MSZIP folder each (config 2's plaintext) on ONE
decompressor over the C in-memory mspack_system (libmspack_amd/csrc/bench/api_bench.c: mspk_api_bench_cabs):
  (a) open all, extract() every file -- every cabinet is a batch of its own;
  (b) open all, prefetch(all), the same extracts -- one batch;
  (c) config 2 itself, ONE cabinet of N folders, for scale.
(a) and (b) run alternately, REPS times each after one warm-up of each; the bar: the slowest (b) beats the fastest (a)."""
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import libmspack_amd as M
from libmspack_amd import apibench as A
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
images, plain = A.build_small_cabs(M, n)
legs = {"a": [], "b": []}
for k in range(reps + 1):
    for leg, pf in (("a", 0), ("b", 1)):
        rc, out, d = A.run_cabs(images, plain.size, pf)
        assert rc == 0 and d["n_errors"] == 0 and d["n_files"] == n and np.array_equal(out, plain), (leg, rc, d)
        if k:
            legs[leg].append(d)
one, _p = A.build_config2_cab(M, n, plain=plain)
c_runs = []
for k in range(reps + 1):
    rc, out, _offs, d = A.run("cab", one, plain.size)
    assert rc == 0 and d["n_errors"] == 0 and np.array_equal(out, plain)
    if k:
        c_runs.append(d)
ms = lambda runs: [round(d["total_s"] * 1e3, 2) for d in runs]
res = {"n_cabinets": n, "bytes": int(plain.size),
       "a_no_prefetch_ms": ms(legs["a"]), "b_prefetch_ms": ms(legs["b"]), "c_one_cabinet_ms": ms(c_runs),
       "a_batch_calls": legs["a"][0]["lib_calls"], "b_batch_calls": legs["b"][0]["lib_calls"], "c_batch_calls": c_runs[0]["lib_calls"],
       "b_best_split": A.summary(min(legs["b"], key=lambda d: d["total_s"])),
       "c_best_split": A.summary(min(c_runs, key=lambda d: d["total_s"])),
       "a_best_split": A.summary(min(legs["a"], key=lambda d: d["total_s"]))}
print(json.dumps(res))
assert max(res["b_prefetch_ms"]) < min(res["a_no_prefetch_ms"]), "prefetch is not faster: b %s, a %s" % (res["b_prefetch_ms"], res["a_no_prefetch_ms"])
print("OK: slowest (b) %.2f ms < fastest (a) %.2f ms; best (c) %.2f ms" % (max(res["b_prefetch_ms"]), min(res["a_no_prefetch_ms"]), min(res["c_one_cabinet_ms"])))
