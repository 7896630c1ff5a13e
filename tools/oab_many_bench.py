"""A directory of small OAB files through the object API, one call per file against one mspack_oabd_decompress_many():
python tools/oab_many_bench.py [N=256,1024] [REPS=5] -- N recipe OAB files (tests/oab_recipe.py) of ONE 16 KiB block of text each (the
per-language templates of an address list), as files in a temporary directory, on ONE decompressor over the library's default (stdio)
mspack_system (as tools/szdd_prefetch_bench.py: an in-memory system made of Python callbacks would time the callbacks); and a second
set of N in which every fourth file is a patch against another file's plaintext:
  (a) decompress() / decompress_incremental() for every file -- every call is a batch of its own (the behaviour without the call);
  (b) one mspack_oabd_decompress_many() over the same jobs -- one batch.
(a) and (b) run alternately, REPS times each after one warm-up of each; every 64th output file is compared with its plaintext.
No ratio is asserted: the lines say what was measured."""
import json, os, shutil, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import libmspack_amd as M
from libmspack_amd import api
import oab_recipe as O

ns = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [256, 1024]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
DISTINCT = 32                                    # distinct texts; the files cycle through them
plains = [M.gen_plaintext(700 + k, (0, 2)[k & 1], 16384 - 37 * k).tobytes() for k in range(DISTINCT)]
fulls = [O.oab_full(p, 16384) for p in plains]
patches = [O.oab_patch(plains[(k + 1) % DISTINCT], plains[k], 16384) for k in range(DISTINCT)]     # plains[k + 1] -> plains[k]
L = api._setup_oab()
res = {"full_file_bytes": [min(map(len, fulls)), max(map(len, fulls))], "patch_file_bytes": [min(map(len, patches)), max(map(len, patches))],
       "plain_bytes": [min(map(len, plains)), max(map(len, plains))], "runs": {}}


def leg(jobs, many):
    """-> seconds for all jobs = [(input, base or None, output)], the decompressor's creation and destruction included"""
    t0 = time.perf_counter()
    if many:
        rc, errs = api.oab_decompress_paths(jobs, L=L)
        assert rc == 0
    else:
        d = L.mspack_create_oab_decompressor(None)
        m = d.contents
        errs = [m.decompress(d, pi, po) if pb is None else m.decompress_incremental(d, pi, pb, po) for pi, pb, po in jobs]
        L.mspack_destroy_oab_decompressor(d)
    t = time.perf_counter() - t0
    assert not any(errs)
    return t


tmp = tempfile.mkdtemp(prefix="oab_bench_")
try:
    bases = []
    for k, p in enumerate(plains):
        bases.append(os.fsencode(os.path.join(tmp, "base%02d" % k)))
        with open(bases[-1], "wb") as fh:
            fh.write(p)
    for n in ns:
        for share in (0, 4):                     # every share-th file a patch (0: none)
            jobs = []
            for i in range(n):
                k = i % DISTINCT
                patch = share and i % share == share - 1
                pi = os.fsencode(os.path.join(tmp, "f%05d.lzx" % i))
                with open(pi, "wb") as fh:
                    fh.write(patches[k] if patch else fulls[k])
                jobs.append((pi, bases[(k + 1) % DISTINCT] if patch else None, os.fsencode(os.path.join(tmp, "f%05d.oab" % i))))
            legs, counts = {"a": [], "b": []}, {}
            for r in range(reps + 1):
                for name, many in (("a", 0), ("b", 1)):
                    api.oab_batch_counts(reset=True)
                    t = leg(jobs, many)
                    counts[name] = api.oab_batch_counts()
                    for i in range(0, n, max(1, n // 64)):
                        with open(jobs[i][2], "rb") as fh:
                            assert fh.read() == plains[i % DISTINCT], (name, i)
                    if r:
                        legs[name].append(round(t * 1e3, 2))
            res["runs"]["%d files, %s" % (n, "every 4th a patch" if share else "all full")] = {
                "a_loop_ms": legs["a"], "b_one_call_ms": legs["b"], "a_counts_batches_jobs_again": counts["a"],
                "b_counts_batches_jobs_again": counts["b"]}
            for pi, _pb, po in jobs:
                os.unlink(pi); os.unlink(po)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
print(json.dumps(res))
for name, r in res["runs"].items():
    print("%s: the loop %s ms (%d batches), one call %s ms (%d batch)" % (
        name, r["a_loop_ms"], r["a_counts_batches_jobs_again"][0], r["b_one_call_ms"], r["b_counts_batches_jobs_again"][0]))
