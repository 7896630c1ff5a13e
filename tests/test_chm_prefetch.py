"""mspack_chmd_prefetch (include/mspack.h): the reset intervals of MANY CHMs in one batch, said by the caller before the extract() calls.

The yardstick everywhere is the same calls on a fresh decompressor WITHOUT the call: bytes, return codes, last_error() and the lines
said through sys->message, call by call; for the variants of tests/golden/chm_extract.json also what the real chmd answered when
they were recorded.  mspack_chmd_batch_counts() says how many batches the driver issued: one for the call, none for the extract()
calls of clean CHMs behind it.

  * `-m "not gpu"`: the driver (csrc/host/chmd.c) on the CPU stand-in for the batch ABI (tests/csrc/batch_standin.c), whose jobs are
    lazy and fill the results with 0xEE: a driver that reads what it has not waited for fails here; the same sequences as a program
    of its own under ASan + UBSan (tests/csrc/chm_prefetch_check.c);
  * `-m gpu`: libmspack_hip.so."""
import glob
import hashlib
import json
import os
import subprocess

import pytest

from libmspack_amd import api
import chm_extract_recipe as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VECS = {v["tag"]: v for v in json.load(open(os.path.join(HERE, "golden", "chm_extract.json")))}
ALGS = {api.MSPACK_DIGEST_MD5: hashlib.md5, api.MSPACK_DIGEST_SHA1: hashlib.sha1, api.MSPACK_DIGEST_SHA256: hashlib.sha256}
ALG_LIST = list(ALGS)
P = api.MSCHMD_PARAM_HIP_DIGESTS
ERR_READ, ERR_DECRUNCH = 3, 11

_blobs = {}
_cases = {}


def golden(tag):
    if tag not in _blobs:
        v = VECS[tag]
        chm, _d, _files = R.build(v["case"])
        assert hashlib.md5(chm).hexdigest() == v["chm_md5"], "recipe no longer reproduces the golden CHM"
        _blobs[tag] = chm
    return _blobs[tag]


def custom(name, **case):
    """a CHM of the goldens' recipe that has no golden: files given, or n_files spread over the stream (an empty one among them)"""
    if name not in _blobs:
        if "files" not in case:
            files = R.spread_files(case["n_bytes"], case.pop("n_files", 6), case["seed"], case["reset_frames"] * R.FRAME)
            files.insert(2, ["/empty.bin", files[2][1], 0])
            case["files"] = files
        _cases[name] = case
        _blobs[name] = R.build(case)[0]
    return _blobs[name]


def sec0_only():
    """the files of w16-r2-small, every directory entry's section number set to 0: a CHM whose listed files (one of length 0) are
    all read straight from section 0 -- the bytes of the CHM file itself that lie at those offsets"""
    if "sec0" not in _blobs:
        b = bytearray(blob_of("w16-r2-small"))
        for nm, _off, _ln in _cases["w16-r2-small"]["files"]:
            at = b.find(nm.encode() + b"\x01")
            assert at > 0 and b.find(nm.encode() + b"\x01", at + 1) < 0
            b[at + len(nm)] = 0
        _blobs["sec0"] = bytes(b)
    return _blobs["sec0"]


# ---- the sets ------------------------------------------------------------------------------------------------------------------------
# windows 15, 16, 21; reset intervals of 1, 2 and 64 frames; E8; a short last interval (an interval of 3 frames: lzx17-r1-interval3);
# a reset table shorter than the stream (fewentries: n_fast 3 of 6 intervals); section-0 files only; files of length 0
GOLDEN_IN_MIXED = ["lzx21-r2", "lzx16-r2", "lzx21-r64", "lzx21-r2-e8", "lzx17-r1-interval3", "lzx21-r2-fewentries"]
CLEAN = {"lzx21-r2", "lzx16-r2", "lzx21-r64", "w15-r1", "w16-r2-small", "sec0"}      # no batch behind a prefetch, whatever the order


def mixed_set():
    names = ["lzx21-r2", "w15-r1", "lzx16-r2", "lzx21-r64", "lzx21-r2-e8", "sec0", "lzx17-r1-interval3", "lzx21-r2-fewentries", "w16-r2-small"]
    return names, [blob_of(n) for n in names]


def blob_of(name):
    if name in VECS:
        return golden(name)
    if name == "sec0":
        return sec0_only()
    if name == "w15-r1":                                         # three intervals of one frame, the last file ends the stream
        return custom(name, seed=41, text=0, n_bytes=3 * R.FRAME, window_bits=15, reset_frames=1, n_files=7)
    if name == "w16-r2-small":
        return custom(name, seed=43, text=1, n_bytes=2 * 2 * R.FRAME, window_bits=16, reset_frames=2, n_files=5)
    if name == "flip-interval1":                                 # one flipped payload bit in the second interval (frame 2)
        c = dict(VECS["lzx16-r2-flip@f6"]["case"])
        c["mutations"] = [["flip_content", 2, 40, 4]]
        return custom(name, **c)
    if name == "no-rtable":                                      # the ResetTable's directory entry names something else
        if name not in _blobs:
            b = bytearray(golden("lzx21-r2"))
            at = b.find(b"InstanceData/ResetTable")
            assert at > 0 and b.find(b"InstanceData/ResetTable", at + 1) < 0
            b[at + len(b"InstanceData/ResetTabl")] = ord("f")
            _blobs[name] = bytes(b)
        return _blobs[name]
    raise KeyError(name)


def orders(s, n):
    """every file of every CHM: forward, backward, interleaved across the CHMs"""
    per = [[(k, i) for i in range(len(s.files(k)))] for k in range(n)]
    fwd = [op for p in per for op in p]
    inter = [p[j] for j in range(max(len(p) for p in per)) for p in per if j < len(p)]
    return dict(forward=fwd, backward=fwd[::-1], interleaved=inter)


def run_ops(s, ops, L, digest_alg=None):
    """-> per call (k, i, err, last_error, md5 of the bytes written / the digest, lines said, batches issued)"""
    out = []
    for n, (k, i) in enumerate(ops):
        before, b0 = len(s.messages), api.chmd_batch_counts(L=L)[0]
        if digest_alg is None:
            err, data = s.extract(k, i)
            what = (len(data), hashlib.md5(data).hexdigest())
        else:
            alg = digest_alg if isinstance(digest_alg, int) else ALG_LIST[n % 3]
            err, dg = s.digest(k, i, alg)
            what = (alg, dg.hex())
            assert not s.mem.outputs
        out.append((k, i, err, s.last_error(), what, list(s.messages[before:]), api.chmd_batch_counts(L=L)[0] - b0))
    return out


def strip(records):
    return [r[:6] for r in records]


def check_mixed(L, where):
    names, blobs = mixed_set()
    total = 0
    for kind in ("forward", "backward", "interleaved"):
        with api.ChmSet(blobs, L=L) as a, api.ChmSet(blobs, L=L) as b:
            assert a.open_errors == b.open_errors == [0] * len(blobs)
            ops = orders(a, len(blobs))[kind]
            api.chmd_batch_counts(reset=True, L=L)
            want = run_ops(a, ops, L)
            n_without = api.chmd_batch_counts(L=L)[0]
            api.chmd_batch_counts(reset=True, L=L)
            said = len(b.messages)
            assert b.prefetch() == 0 and b.last_error() == 0 and len(b.messages) == said and not b.mem.outputs
            n_batches, n_units = api.chmd_batch_counts(L=L)
            assert n_batches == 1 and n_units >= 12 + 3 + 12 + 2 + 10 + 2 + 3 + 2, (n_batches, n_units)
            got = run_ops(b, ops, L)
            assert strip(got) == strip(want), (where, kind, [(x, y) for x, y in zip(got, want) if x[:6] != y[:6]][:3])
            assert all(r[6] == 0 for r in got if names[r[0]] in CLEAN), (where, kind, [r for r in got if r[6] and names[r[0]] in CLEAN][:3])
            assert n_without >= sum(1 for n in names if n != "sec0"), n_without      # one or more per CHM without the call
            assert any(r[4][0] == 0 and r[2] == 0 for r in got)                           # a file of length 0
            assert any(a.files(k)[i][3] == 0 and a.files(k)[i][1] > 0 for k, i in ops)    # files of section 0
            assert all(f[3] == 0 for f in a.files(names.index("sec0")))
            total += len(ops)
    return total


def check_goldens(L, where):
    """what the real chmd answered (tests/golden/chm_extract.json), call by call, behind one prefetch of all of them"""
    blobs = [golden(t) for t in GOLDEN_IN_MIXED]
    for ri in range(max(len(VECS[t]["runs"]) for t in GOLDEN_IN_MIXED)):
        with api.ChmSet(blobs, L=L) as s:
            assert s.prefetch() == 0
            for k, t in enumerate(GOLDEN_IN_MIXED):
                runs = VECS[t]["runs"]
                if ri >= len(runs):
                    continue
                for n, (idx, exp) in enumerate(zip(runs[ri]["order"], runs[ri]["results"])):
                    err, data = s.extract(k, idx)
                    assert err == exp["err"] and len(data) == exp["n"] and hashlib.md5(data).hexdigest() == exp["md5"], (where, t, ri, n, idx, err, exp)


def check_isolation(L, where):
    names = ["lzx16-r2", "lzx21-r2-cut", "w16-r2-small", "flip-interval1", "w15-r1"]
    blobs = [blob_of(n) for n in names]
    alone = []
    for blob in blobs:                                           # every CHM alone, on a decompressor of its own
        with api.ChmSet([blob], L=L) as s:
            alone.append(run_ops(s, orders(s, 1)["forward"], L))
    assert any(r[2] == ERR_READ for r in alone[1]) and any(r[2] != 0 for r in alone[3]) and any(r[2] == 0 for r in alone[3])
    assert all(r[2] == 0 for k in (0, 2, 4) for r in alone[k])
    with api.ChmSet(blobs, L=L) as s:
        api.chmd_batch_counts(reset=True, L=L)
        assert s.prefetch() == 0 and api.chmd_batch_counts(L=L)[0] == 1
        for k in (2, 1, 3, 0, 4):
            got = run_ops(s, [(k, i) for i in range(len(s.files(k)))], L)
            assert [r[1:6] for r in got] == [r[1:6] for r in alone[k]], (where, names[k], [(x, y) for x, y in zip(got, alone[k]) if x[1:6] != y[1:6]][:3])
            if k in (0, 2, 4):
                assert all(r[6] == 0 for r in got)


def check_budget(L, where, set_mb, get_mb):
    names = ["lzx16-r2", "w16-r2-small", "lzx21-r2", "w15-r1"]     # 768 KiB, 128 KiB, 768 KiB, 96 KiB of decoded bytes
    blobs = [blob_of(n) for n in names]
    old = get_mb()
    try:
        assert set_mb(1) == 0
        with api.ChmSet(blobs, L=L) as a, api.ChmSet(blobs, L=L) as b:
            ops = orders(a, len(blobs))["interleaved"]
            want = run_ops(a, ops, L)
            api.chmd_batch_counts(reset=True, L=L)
            assert b.prefetch() == 0
            assert api.chmd_batch_counts(L=L) == (1, 12 + 2), api.chmd_batch_counts(L=L)    # the first two fit 1 MiB, the third does not
            got = run_ops(b, ops, L)
            assert strip(got) == strip(want), (where, [(x, y) for x, y in zip(got, want) if x[:6] != y[:6]][:3])
            assert all(r[6] == 0 for r in got if r[0] < 2) and sum(r[6] for r in got if r[0] >= 2) >= 2
    finally:
        assert set_mb(old) == 0


def check_digests(L, where, on_device):
    names = ["lzx16-r2", "w15-r1", "lzx21-r2", "w16-r2-small", "sec0"]
    blobs = [blob_of(n) for n in names]
    for alg in ALGS:
        api.chmd_digest_counts(alg, reset=True, L=L)
    with api.ChmSet(blobs, L=L) as a, api.ChmSet(blobs, L=L) as b:
        assert b.set_param(P, 7) == 0
        ops = orders(a, len(blobs))["forward"]
        want = [a.extract(k, i) for k, i in ops]
        assert all(err == 0 for (k, _i), (err, _d) in zip(ops, want) if names[k] != "sec0")
        api.chmd_batch_counts(reset=True, L=L)
        assert b.prefetch() == 0 and api.chmd_batch_counts(L=L)[0] == 1
        n_ok = 0
        for alg, h in ALGS.items():
            for (k, i), (err_x, data) in zip(ops, want):
                err, dg = b.digest(k, i, alg)
                assert err == err_x and dg == (h(data).digest() if err == 0 else bytes(api.DIGEST_BYTES[alg])), (where, names[k], i, alg)
                n_ok += err == 0
        assert api.chmd_batch_counts(L=L)[0] == 1                    # the call's, and none behind it
    counts = [api.chmd_digest_counts(alg, L=L) for alg in ALGS]
    assert sum(c[0] + c[1] for c in counts) == n_ok
    if on_device:
        assert all(c[0] > 0 for c in counts), counts                 # files inside one chunk, below the ratio: the device's
    else:
        assert all(c[0] == 0 for c in counts), counts                # the stand-in has no digest feature


# ---- CPU -----------------------------------------------------------------------------------------------------------------------------
def test_mixed_set_three_orders_cpu(built, hostlogic):
    assert check_mixed(hostlogic, "cpu") > 100


def test_goldens_behind_one_prefetch_cpu(built, hostlogic):
    check_goldens(hostlogic, "cpu")


def test_neighbours_of_a_cut_and_a_damaged_chm_cpu(built, hostlogic):
    check_isolation(hostlogic, "cpu")


def test_setup_failure_is_not_cached_and_says_nothing_cpu(built, hostlogic):
    L = hostlogic
    names = ["lzx16-r2", "lzx21-r2-badwindow", "w16-r2-small", "no-rtable", "w15-r1"]
    blobs = [blob_of(n) for n in names]
    for fast in (False, True):
        with api.ChmSet(blobs, L=L) as a, api.ChmSet(blobs, L=L, fast=fast) as b:
            ops = orders(a, len(blobs))["interleaved"]
            want = run_ops(a, ops, L)
            assert any(r[2] != 0 for r in want if r[0] == 1) and all(r[2] == 0 for r in want if r[0] in (0, 2, 4))
            api.chmd_batch_counts(reset=True, L=L)
            said = len(b.messages)
            assert b.prefetch() == 0 and b.last_error() == 0 and len(b.messages) == said
            assert api.chmd_batch_counts(L=L) == (1, 12 + 2 + 3)         # the good ones are in the batch
            if fast:                                                      # (fast_open lists no files: the names, through fast_find)
                got = []
                for k, i in ops:
                    before = len(b.messages)
                    err_f, f = b.find(k, a.files(k)[i][0])
                    assert err_f == 0 and f is not None
                    err, data = b.extract_found(f)
                    got.append((k, i, err, b.last_error(), (len(data), hashlib.md5(data).hexdigest()), list(b.messages[before:])))
            else:
                got = strip(run_ops(b, ops, L))
            assert got == strip(want), [(x, y) for x, y in zip(got, strip(want)) if x != y][:3]


def test_advice_and_arguments_cpu(built, hostlogic):
    L = api._setup(hostlogic)
    blobs = [blob_of(n) for n in ("lzx16-r2", "w16-r2-small", "w15-r1")]
    HP = api._P(api.MschmdHeader)
    with api.ChmSet(blobs, L=hostlogic) as s:
        api.chmd_batch_counts(reset=True, L=hostlogic)
        arr = (HP * 2)(s.chms[0], None)
        assert L.mspack_chmd_prefetch(None, arr, 1) == api.MSPACK_ERR_ARGS
        for args in ((arr, -1), (None, 1), (arr, 2)):
            assert L.mspack_chmd_prefetch(s.d, args[0], args[1]) == api.MSPACK_ERR_ARGS and s.last_error() == api.MSPACK_ERR_ARGS
        assert L.mspack_chmd_prefetch(s.d, None, 0) == 0 and s.last_error() == 0 and s.prefetch([]) == 0
        assert api.chmd_batch_counts(L=hostlogic) == (0, 0) and not s.messages
        L.mspack_chmd_batch_counts(None, 0)                                   # (counts may be NULL)
        # some extract() calls first: the call takes only what is left
        err, data0 = s.extract(0, 3)
        assert err == 0 and api.chmd_batch_counts(L=hostlogic) == (1, 12)
        assert s.prefetch([1, 1, 0, 2, 1]) == 0                                # twice, thrice: harmless
        assert api.chmd_batch_counts(L=hostlogic) == (2, 12 + 2 + 3)
        assert s.prefetch() == 0 and s.prefetch([2]) == 0                     # everything is decoded: no batch
        assert api.chmd_batch_counts(L=hostlogic) == (2, 12 + 2 + 3)
        with api.ChmSet(blobs, L=hostlogic) as ref:
            for k, i in orders(s, 3)["backward"]:
                assert s.extract(k, i) == ref.extract(k, i)
        assert s.extract(0, 3) == (0, data0)


def test_budget_leaves_the_rest_to_extract_cpu(built, hostlogic):
    check_budget(hostlogic, "cpu", hostlogic.mspack_hip_set_cache_mb, hostlogic.mspack_hip_cache_mb)


def lifetime_sequences(L):
    names = ["lzx16-r2", "w15-r1", "lzx21-r2", "w16-r2-small"]
    blobs = [blob_of(n) for n in names]
    with api.ChmSet(blobs, L=L) as ref:
        want = {(k, i): ref.extract(k, i) for k, i in orders(ref, len(blobs))["forward"]}
    # close one CHM of the batch (the second: its units lie between the others'), then extract from the others, last CHM first
    with api.ChmSet(blobs, L=L) as s:
        assert s.prefetch() == 0
        ops = orders(s, len(blobs))["backward"]
        s.close(1)
        for k, i in ops:
            if k != 1:
                assert s.extract(k, i) == want[(k, i)], (k, i)
        s.close(3); s.close(0)
        assert s.extract(2, 0) == want[(2, 0)]
    # close all and destroy without extracting anything; destroy at once
    s = api.ChmSet(blobs, L=L)
    assert s.prefetch() == 0
    s.close()
    s = api.ChmSet(blobs, L=L)
    assert s.prefetch([3, 2]) == 0
    s.close(2)
    s.close()


def test_lifetime_of_a_running_batch_cpu(built, hostlogic):
    L = api._setup(hostlogic)
    L.mspack_standin_jobs_begun.restype = api.C.c_ulong
    b0 = L.mspack_standin_jobs_begun()
    lifetime_sequences(hostlogic)
    assert L.mspack_standin_jobs_begun() >= b0 + 3                            # those batches did run as (lazy) jobs
    # synchronous: no jobs, and the sharded call of two devices
    b0 = L.mspack_standin_jobs_begun()
    os.environ["MSPACK_HIP_JOBS"] = "0"
    try:
        lifetime_sequences(hostlogic)
    finally:
        del os.environ["MSPACK_HIP_JOBS"]
    old = hostlogic.mspack_hip_default_devices()
    try:
        assert hostlogic.mspack_hip_set_default_devices(2) == 0
        lifetime_sequences(hostlogic)
    finally:
        assert hostlogic.mspack_hip_set_default_devices(old) == 0
    assert L.mspack_standin_jobs_begun() == b0


def test_digests_of_a_prefetched_set_cpu(built, hostlogic):
    check_digests(hostlogic, "cpu", on_device=False)


ONE_BATCH = ["lzx16-r2", "w15-r1", "w16-r2-small", "one-interval"]     # 12, 3, 2 reset intervals, and 1: never a job


def one_interval():
    return custom("one-interval", seed=47, text=2, n_bytes=R.FRAME, window_bits=15, reset_frames=1, n_files=4)


MIB = 1 << 20


def three_chunks():
    """3 MiB in 48 intervals of 64 KiB -- three chunks of 16 units where chmd.c is built with chunks of 1 MiB (the sanitizer program's
    sequence 6).  Files, in directory order: in chunk 0's first interval, in chunk 1, in chunk 2, further into chunk 0, across
    the border of chunks 0 and 1"""
    return custom("three-chunks", seed=53, text=0, n_bytes=3 * MIB, window_bits=16, reset_frames=2,
                  files=[["/a.bin", 1000, 5000], ["/b.bin", MIB + 70000, 5000], ["/c.bin", 2 * MIB + 200000, 70000],
                         ["/d.bin", 500000, 300000], ["/e.bin", MIB - 3000, 10000]])


def destroy_with_chms_open(s):
    """the decompressor goes while its CHMs are open; what the CHMs themselves hold is given back afterwards through a second
    decompressor on the same mspack_system (close() needs the system alone), so that a leak checker has nothing to report"""
    s.L.mspack_destroy_chm_decompressor(s.d)
    d2 = s.L.mspack_create_chm_decompressor(s.mem.ptr())
    for j, c in enumerate(s.chms):
        if c:
            d2.contents.close(d2, c)
            s.chms[j] = None; s._files[j] = []
    s.L.mspack_destroy_chm_decompressor(d2)
    s.d = None


def one_batch_sequences(L, where, set_mb, get_mb, jobs_begun=None):
    """Where a chunk's own batch (the first extract() that needs the chunk) and the batch of many CHMs meet: both are a struct
    chm_batch (csrc/host/chmd.c), the first with one member.  Every call against the same call on a fresh decompressor that was
    never told anything: code, last_error(), bytes, lines said.  None of these CHMs is damaged, so a call's answer does not depend
    on the calls before it."""
    blobs = [blob_of(n) for n in ONE_BATCH[:3]] + [one_interval()]

    def counts():
        return api.chmd_batch_counts(L=L)

    def calls(s, ops):
        return [r[2:6] for r in run_ops(s, ops, L)]

    with api.ChmSet(blobs, L=L) as ref:
        every = orders(ref, 4)["forward"]
        want = dict(zip(every, calls(ref, every)))
        assert all(w[0] == 0 and not w[3] for w in want.values())

    def same(s, ops, seq):
        got = calls(s, ops)
        assert got == [want[o] for o in ops], (where, seq, [(o, x, want[o]) for o, x in zip(ops, got) if x != want[o]][:3])

    # 1. the first file of lzx16-r2: the chunk's own job runs with most of its units unwaited -- close() at once; and on a
    #    second decompressor: destroy without closing
    s = api.ChmSet(blobs[:1], L=L)
    same(s, [(0, 0)], 1)
    s.close()
    s = api.ChmSet(blobs[:1], L=L)
    same(s, [(0, 0)], 1)
    destroy_with_chms_open(s)

    # 2. two CHMs on demand, then prefetch() of all four: the batch holds the others' units only; everything backward; close in an
    #    order that frees a one-member batch (CHM 0's) between the members of the shared one (CHMs 1 and 3)
    with api.ChmSet(blobs, L=L) as s:
        api.chmd_batch_counts(reset=True, L=L)
        same(s, [(0, 0), (2, 1)], 2)
        assert counts() == (2, 12 + 2)
        assert s.prefetch() == 0 and counts() == (3, 12 + 2 + 3 + 1), counts()
        same(s, every[::-1], 2)
        assert counts() == (3, 12 + 2 + 3 + 1), counts()
        for k in (1, 0, 3, 2):
            s.close(k)

    # 3. prefetch([a, b]), close a, one file of c on demand, prefetch() again: nothing of b or c is issued twice
    with api.ChmSet(blobs, L=L) as s:
        api.chmd_batch_counts(reset=True, L=L)
        assert s.prefetch([0, 1]) == 0 and counts() == (1, 12 + 3), counts()
        s.close(0)
        same(s, [(2, 1)], 3)                                              # (file 0 is the empty one)
        assert counts() == (2, 12 + 3 + 2), counts()
        assert s.prefetch() == 0 and counts() == (3, 12 + 3 + 2 + 1), counts()      # the one interval of the last CHM is what is left
        same(s, [o for o in every[::-1] if o[0] != 0], 3)
        assert s.prefetch() == 0 and counts() == (3, 12 + 3 + 2 + 1), counts()

    # 4. a budget of 1 MiB, lzx16-r2 and lzx21-r2 (768 KiB each) on demand, their files in turn: the answers of the default budget.
    #    (The driver's LRU counts per CHM, so each of the two keeps its one chunk while the other's job may still run: nothing is
    #    evicted here.  A chunk whose own job still runs is evicted in tests/csrc/chm_prefetch_check.c, sequence 6: that needs a
    #    CHM of several chunks, which the library's 64 MiB chunks put out of a quick test's reach.)
    two = [blobs[0], blob_of("lzx21-r2")]
    with api.ChmSet(two, L=L) as ref:
        turns = orders(ref, 2)["interleaved"]
        want4 = calls(ref, turns)
    old = get_mb()
    try:
        assert set_mb(1) == 0
        with api.ChmSet(two, L=L) as s:
            got = calls(s, turns)
            assert got == want4, (where, 4, [(o, x, y) for o, x, y in zip(turns, got, want4) if x != y][:3])
    finally:
        assert set_mb(old) == 0

    # 5. (the stand-in only) the CHM of one interval on demand, and prefetched alone: a batch of one unit each, never a job
    if jobs_begun:
        b0 = jobs_begun()
        last = [i for k, i in every if k == 3][::-1]
        for tell in (False, True):
            with api.ChmSet(blobs[3:], L=L) as s:
                api.chmd_batch_counts(reset=True, L=L)
                assert not tell or (s.prefetch() == 0 and counts() == (1, 1))
                assert calls(s, [(0, i) for i in last]) == [want[(3, i)] for i in last], (where, 5, tell)
                assert counts() == (1, 1), counts()
        assert jobs_begun() == b0


def test_own_batch_and_shared_batch_meet_cpu(built, hostlogic):
    """one_batch_sequences on the stand-in's lazy jobs, without jobs (MSPACK_HIP_JOBS=0) and on two devices (the sharded,
    synchronous call); the batch of one unit (sequence 5) begins no job in any of them"""
    L = api._setup(hostlogic)
    L.mspack_standin_jobs_begun.restype = api.C.c_ulong
    args = (hostlogic.mspack_hip_set_cache_mb, hostlogic.mspack_hip_cache_mb, L.mspack_standin_jobs_begun)
    b0 = L.mspack_standin_jobs_begun()
    one_batch_sequences(hostlogic, "cpu, jobs", *args)
    assert L.mspack_standin_jobs_begun() >= b0 + 6                            # the own batches and the shared ones ran as (lazy) jobs
    b0 = L.mspack_standin_jobs_begun()
    os.environ["MSPACK_HIP_JOBS"] = "0"
    try:
        one_batch_sequences(hostlogic, "cpu, no jobs", *args)
    finally:
        del os.environ["MSPACK_HIP_JOBS"]
    old = hostlogic.mspack_hip_default_devices()
    try:
        assert hostlogic.mspack_hip_set_default_devices(2) == 0
        one_batch_sequences(hostlogic, "cpu, two devices", *args)
    finally:
        assert hostlogic.mspack_hip_set_default_devices(old) == 0
    assert L.mspack_standin_jobs_begun() == b0


SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
       "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "include")]
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")


def test_chm_prefetch_check_under_asan_ubsan(built, tmp_path):
    """tests/csrc/chm_prefetch_check.c: a program of its own (no python in the process, nothing preloaded) on the drivers + the stand-in
    + the oracle, all compiled with -fsanitize=address,undefined: the lifetime sequences above on lazy jobs, without jobs and on
    two devices, the argument cases, a budget of 1 MiB; and one_batch_sequences above, over the CHMs behind "--", with one more:
    the eviction of a chunk whose own job still runs.  For that chmd.c is built with chunks of 1 MiB (as tests/test_chm_digest.py
    does) and the last CHM has three of them; every other CHM decodes to 768 KiB at most and is one chunk as in the library.  Any
    report -- leaks included -- fails."""
    names = ["lzx16-r2", "w15-r1", "lzx21-r2-cut", "w16-r2-small", "lzx21-r2-e8", "lzx21-r2-badwindow"]
    blobs = [blob_of(n) for n in names] + [None] + [blob_of(n) for n in ONE_BATCH[:3]] + [one_interval(), blob_of("lzx21-r2"), three_chunks()]
    paths = []
    for k, blob in enumerate(blobs):
        if blob is None:
            paths.append("--")
            continue
        (tmp_path / ("c%d.chm" % k)).write_bytes(blob)
        paths.append(str(tmp_path / ("c%d.chm" % k)))
    exe = str(tmp_path / "chm_prefetch_check")
    srcs = [os.path.join(HERE, "csrc", "chm_prefetch_check.c")] + \
        sorted(glob.glob(os.path.join(ROOT, "libmspack_amd", "csrc", "host", "*.c"))) + \
        [os.path.join(HERE, "csrc", "batch_standin.c")] + sorted(glob.glob(os.path.join(ROOT, "oracle", "*_oracle.c")))
    subprocess.check_call(["gcc"] + SAN + ["-DCHM_CHUNK_BYTES=((off_t)1<<20)", "-o", exe] + srcs + ["-lpthread"])
    env = dict(os.environ, **SAN_ENV)
    env.pop("MSPACK_HIP_JOBS", None)
    p = subprocess.run([exe, str(tmp_path)] + paths, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "CHM_PREFETCH_CHECK_OK" in out, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out, out[-4000:]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def host_calls(reset=False):
    ms4 = (api.C.c_double * 4)()
    api.lib().mspack_hip_host_path_stats(ms4, int(reset))
    return int(ms4[3])


@pytest.mark.gpu
def test_mixed_set_three_orders_gpu(built):
    assert check_mixed(None, "gpu") > 100


@pytest.mark.gpu
def test_goldens_behind_one_prefetch_gpu(built):
    check_goldens(None, "gpu")


@pytest.mark.gpu
def test_one_batch_call_for_prefetch_and_clean_extracts_gpu(built):
    """mspack_hip_host_path_stats(): the prefetch and every extract() of clean CHMs behind it are ONE call of the host path"""
    names = ["lzx21-r2", "w15-r1", "lzx16-r2", "lzx21-r64", "w16-r2-small", "sec0"]
    blobs = [blob_of(n) for n in names]
    with api.ChmSet(blobs) as a, api.ChmSet(blobs) as b:
        ops = orders(a, len(blobs))["interleaved"]
        want = run_ops(a, ops, None)
        host_calls(reset=True)
        assert b.prefetch() == 0
        got = run_ops(b, ops, None)
        assert host_calls() == 1
        assert strip(got) == strip(want)


@pytest.mark.gpu
def test_neighbours_of_a_cut_and_a_damaged_chm_gpu(built):
    check_isolation(None, "gpu")


@pytest.mark.gpu
def test_budget_leaves_the_rest_to_extract_gpu(built):
    L = api.lib()
    check_budget(None, "gpu", L.mspack_hip_set_cache_mb, L.mspack_hip_cache_mb)


@pytest.mark.gpu
def test_digests_of_a_prefetched_set_gpu(built):
    check_digests(None, "gpu", on_device=True)


@pytest.mark.gpu
def test_own_batch_and_shared_batch_meet_gpu(built):
    """one_batch_sequences 1 to 4 on the library's real jobs: close and destroy while a chunk's own batch may still run, on demand
    beside a batch of many CHMs and at a budget of 1 MiB (every CHM decodes to 768 KiB at most: one chunk each, so no chunk is
    evicted here)"""
    L = api.lib()
    one_batch_sequences(None, "gpu", L.mspack_hip_set_cache_mb, L.mspack_hip_cache_mb)


@pytest.mark.gpu
def test_64_chms_of_one_interval_share_a_launch_gpu(built):
    """64 CHMs of one 32 KiB interval each, windows 15 to 21 in turn: one batch of 64 units, one call of the host path"""
    import libmspack_amd as M
    blobs, plain = [], []
    for k in range(64):
        case = dict(seed=100 + k, text=k % 3, n_bytes=R.FRAME, window_bits=15 + k % 7, reset_frames=1,
                    files=[["/a.bin", 0, 20000 + 37 * k], ["/b.bin", 20000 + 37 * k, R.FRAME - 20000 - 37 * k]])
        chm, d, _files = R.build(case)
        blobs.append(chm); plain.append(bytes(d))
    with api.ChmSet(blobs) as s:
        api.chmd_batch_counts(reset=True)
        host_calls(reset=True)
        assert s.prefetch() == 0 and api.chmd_batch_counts() == (1, 64)
        for k in list(range(0, 64, 2)) + list(range(63, 0, -2)):
            cut = 20000 + 37 * k
            assert s.extract(k, 1) == (0, plain[k][cut:]) and s.extract(k, 0) == (0, plain[k][:cut]), k
        assert api.chmd_batch_counts() == (1, 64) and host_calls() == 1 and not s.messages
