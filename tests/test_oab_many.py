"""mspack_oabd_decompress_many (include/mspack.h): many OAB files -- full files and patches -- in ONE call, their blocks in as few
batches as the three batch-ending rules allow, against what the REAL reference answered for the same files (tests/golden/oab.json,
the goldens of tests/test_oab.py) and against the loop of decompress() / decompress_incremental() over the same jobs.

Every check runs twice, as in test_oab.py: on the CPU (`hostlogic`: csrc/host/oabd.c on tests/csrc/batch_standin.c, LZX DELTA units
decoded by the oracle, CRCs on the host) and on the GPU (units flagged MSPACK_HIP_UF_CRC32).  What a batch of several files does
when the batch call itself fails is seen on the CPU only (tests/csrc/oab_poison_provider.c): no GPU run is made to fail."""
import glob
import hashlib
import json
import os
import shutil
import struct
import subprocess
import tempfile

import ctypes as C
import numpy as np
import pytest

import libmspack_amd as M
from libmspack_amd import api
import oab_recipe as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = {e["name"]: e for e in json.load(open(os.path.join(HERE, "golden", "oab.json")))}
ERR_OK, ERR_ARGS, ERR_OPEN, ERR_SIGNATURE, ERR_DECRUNCH = 0, 1, 2, 7, 11
_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = R.cases()
        for name, blob, _base, _want in _CASES:
            assert hashlib.md5(blob).hexdigest() == G[name]["blob_md5"]          # the very files the reference saw
    return _CASES


def sig(err, out):
    return [err, len(out), hashlib.md5(out).hexdigest()]


def a16(n):
    return (n + 15) & ~15


# ---- the driver's arena layout, written down a second time: what one job adds to a batch's arenas (csrc/host/oabd.c, gather) -------
def job_arena(blob, base, in_bytes=0, out_bytes=0):
    """-> (input arena bytes, output arena bytes, units that go into the batch) after this job, from the totals before it"""
    patch = base is not None
    hs = 0x1c if patch else 0x10
    if len(blob) < hs:
        return in_bytes, out_bytes, 0
    w = struct.unpack_from("<7I" if patch else "<4I", blob)
    if w[0] != 3 or w[1] != (2 if patch else 1):
        return in_bytes, out_bytes, 0
    block_max, target = (max(w[2], 16), w[4]) if patch else (w[2], w[3])
    pos, blocks = hs, []
    while target:
        if len(blob) - pos < 16:
            break
        a, b, c, _crc = struct.unpack_from("<4I", blob, pos)
        pos += 16
        if patch:
            csize, dsize, ssize, comp = a, b, c, 1
            if dsize > block_max or dsize > target or ssize > block_max:
                break
        else:
            comp, csize, dsize, ssize = a, b, c, 0
            if dsize > block_max or dsize > target or comp > 1 or (not comp and dsize != csize):
                break
        got = min(csize, len(blob) - pos)
        pos += got
        in_bytes = a16(in_bytes) + got + 16
        blocks.append((comp, dsize, ssize))
        target -= dsize
        if got < csize:
            break
    units, left = 0, len(base) if patch else 0
    for comp, dsize, ssize in blocks:
        if not comp:
            continue
        out_bytes = a16(out_bytes) + a16(ssize) + dsize
        ok = ssize <= left                     # (a reference slice the base does not hold: the block and those behind it stay out)
        left = left - ssize if ok else -1
        units += 1 if ok and dsize else 0
    return in_bytes, out_bytes, units


def batches_by_budget(items, budget):
    """the batch calls the budget rule gives for items = [(blob, base)]: a job that takes input + output past `budget` starts the next
    batch; batches without a unit are not issued"""
    n, inb, outb, units, members = 0, 0, 0, 0, 0
    for blob, base in items:
        i2, o2, u = job_arena(blob, base, inb, outb)
        if members and i2 + o2 > budget:
            n += 1 if units else 0
            i2, o2, u = job_arena(blob, base)
            units, members = 0, 0
        inb, outb, units, members = i2, o2, units + u, members + 1
    return n + (1 if units else 0)


# ---- the checks, for either library ----------------------------------------------------------------------------------------------------
def check_undamaged(L):
    api.oab_batch_counts(reset=True, L=L)
    got = api.oab_decompress_many([(blob, base) for _n, blob, base, _w in cases()], L=L)
    assert [(e, o == want) for (e, o), (_n, _b, _ba, want) in zip(got, cases())] == [(0, True)] * 6
    assert api.oab_batch_counts(L=L) == (1, 6, 0)               # the six files went out as one batch


def check_damaged(L):
    items, want = [], []
    for name, blob, base, plain in cases():
        g = G[name]
        rng = np.random.default_rng(len(blob))                    # test_oab.py's seeding: the copies the goldens were recorded for
        items.append((blob, base)); want.append(sig(0, plain))
        for i, m in enumerate(R.damaged(blob, rng, len(g["damaged"]))):
            items.append((bytes(m), base)); want.append(g["damaged"][i])
    assert len(items) == 6 + sum(len(g["damaged"]) for g in G.values()) > 240
    order = np.random.default_rng(258).permutation(len(items))
    items, want = [items[k] for k in order], [want[k] for k in order]
    budget = M.lib().mspack_hip_cache_mb() << 20 if L is None else L.mspack_hip_cache_mb() << 20
    inb, outb = 0, 0
    for blob, base in items:
        inb, outb, _u = job_arena(blob, base, inb, outb)
    api.oab_batch_counts(reset=True, L=L)
    got = api.oab_decompress_many(items, L=L)
    counts = api.oab_batch_counts(L=L)
    print("damaged: arenas %d + %d bytes of a budget of %d; counts %r" % (inb, outb, budget, counts))
    for k, (e, o) in enumerate(got):
        assert sig(e, o) == want[k], (int(order[k]), sig(e, o), want[k])
    assert counts[2] == 0 and 200 < counts[1] <= len(items)
    if inb + outb <= budget:
        assert 1 <= counts[0] <= 4
    else:
        assert counts[0] == batches_by_budget(items, budget)


def check_truncated_and_short_base(L):
    got = api.oab_decompress_many([(blob[:len(blob) * 2 // 3], base) for _n, blob, base, _w in cases()], decompbuf=1000, L=L)
    for (name, _b, _ba, _w), (e, o) in zip(cases(), got):
        assert sig(e, o) == G[name]["truncated_buf1000"], name
    patches = [c for c in cases() if c[2] is not None]
    got = api.oab_decompress_many([(blob, base[:len(base) // 2]) for _n, blob, base, _w in patches], L=L)
    assert len(patches) == 2
    for (name, _b, _ba, _w), (e, o) in zip(patches, got):
        assert sig(e, o) == G[name]["short_base"], name


class Dir:
    """files of a temporary directory, by name"""

    def __enter__(self):
        self.d = tempfile.mkdtemp(prefix="oab_many_test_")
        return self

    def __exit__(self, *a):
        shutil.rmtree(self.d, ignore_errors=True)

    def path(self, name):
        return os.fsencode(os.path.join(self.d, name))

    def put(self, name, data):
        with open(os.path.join(self.d, name), "wb") as fh:
            fh.write(data)
        return self.path(name)

    def get(self, name):
        p = os.path.join(self.d, name)
        return open(p, "rb").read() if os.path.exists(p) else None


def check_chain(L):
    """base + patch1 -> P, then P + patch2 -> v3 in one call: job 1 reads what job 0 writes, so job 0's batch is replayed first"""
    c = {x[0]: x for x in cases()}
    _n, patch1, base, v2 = c["patch_one_block"]
    other = M.gen_plaintext(21, 0, 150000).tobytes()
    patch2 = R.oab_patch(v2, other, 262144)
    with Dir() as t:
        jobs = [(t.put("p1.oab", patch1), t.put("base", base), t.path("P")),
                (t.put("p2.oab", patch2), t.path("P"), t.path("v3"))]
        api.oab_batch_counts(reset=True, L=L)
        assert api.oab_decompress_paths(jobs, L=L) == (ERR_OK, [0, 0])
        assert t.get("P") == v2 and t.get("v3") == other
        assert api.oab_batch_counts(L=L) == (2, 2, 0)
        # the other direction is no dependence: a job may overwrite what an earlier job of its batch has read
        t.put("base2", base)
        jobs = [(t.path("p1.oab"), t.path("base2"), t.path("Q")), (t.put("f.oab", c["full_tiny"][1]), None, t.path("base2"))]
        api.oab_batch_counts(reset=True, L=L)
        assert api.oab_decompress_paths(jobs, L=L) == (ERR_OK, [0, 0])
        assert t.get("Q") == v2 and t.get("base2") == c["full_tiny"][3]
        assert api.oab_batch_counts(L=L) == (1, 2, 0)


def check_budget(L, set_mb, get_mb):
    items = [(blob, base) for _n, blob, base, _w in cases()]
    before = get_mb()
    assert set_mb(1) == 0
    try:
        api.oab_batch_counts(reset=True, L=L)
        got = api.oab_decompress_many(items, L=L)
        counts = api.oab_batch_counts(L=L)
    finally:
        assert set_mb(before) == 0
    assert [(e, o == want) for (e, o), (_n, _b, _ba, want) in zip(got, cases())] == [(0, True)] * 6
    assert counts[0] == batches_by_budget(items, 1 << 20) > 1 and counts[1:] == (6, 0)


def check_arguments(L):
    api._setup_oab(L)
    c = {x[0]: x for x in cases()}
    tiny, tiny_plain = c["full_tiny"][1], c["full_tiny"][3]
    with Dir() as t:
        pin = t.put("tiny.oab", tiny)
        api.oab_batch_counts(reset=True, L=L)
        assert api.oab_decompress_paths([], L=L) == (ERR_OK, [])                               # n == 0: nothing is issued
        d = (L or M.lib()).mspack_create_oab_decompressor(None)
        try:
            many = (L or M.lib()).mspack_oabd_decompress_many
            arr = (api.MsoabdJob * 1)()
            arr[0].input, arr[0].output = pin, t.path("never")
            assert many(d, None, 1) == ERR_ARGS and many(d, arr, -1) == ERR_ARGS and many(None, arr, 1) == ERR_ARGS
            assert many(d, None, 0) == ERR_OK
        finally:
            (L or M.lib()).mspack_destroy_oab_decompressor(d)
        # a job without input (or output): ERR_ARGS, and no job is started -- the sound job before it writes nothing
        assert api.oab_decompress_paths([(pin, None, t.path("never")), (None, None, t.path("x"))], L=L)[0] == ERR_ARGS
        assert api.oab_decompress_paths([(pin, None, t.path("never")), (pin, None, None)], L=L)[0] == ERR_ARGS
        assert t.get("never") is None and api.oab_batch_counts(L=L) == (0, 0, 0)
        # per-job answers: an input that does not exist, a patch given as a full file, a base that does not exist -- between sound jobs
        jobs = [(pin, None, t.path("o0")), (t.path("missing.oab"), None, t.path("o1")),
                (t.put("patch.oab", c["patch_one_block"][1]), None, t.path("o2")),
                (t.path("patch.oab"), t.path("missing.base"), t.path("o3")), (pin, None, t.path("o4"))]
        assert api.oab_decompress_paths(jobs, L=L) == (ERR_OK, [0, ERR_OPEN, ERR_SIGNATURE, ERR_OPEN, 0])
        assert [t.get("o%d" % k) for k in range(5)] == [tiny_plain, None, None, None, tiny_plain]   # (no output is created for them, as ever)
        assert api.oab_batch_counts(L=L) == (1, 2, 0)
    assert api.oab_decompress_many([(b"\x03\0\0\0\x02\0\0\0" + b"\0" * 8, None)], L=L) == [(ERR_SIGNATURE, b"")]


def fresh_items():
    """about 40 template-sized full files of one to three blocks, and 8 patches between pairs of them"""
    rng = np.random.default_rng(77)
    plains = [M.gen_plaintext(900 + k, (0, 2)[k & 1], int(rng.integers(2048, 40960))).tobytes() for k in range(40)]
    items = [(R.oab_full(p, 16384), None) for p in plains]
    for k in range(8):
        a, b = plains[5 * k], plains[5 * k + 3]
        items.insert(6 * k + 2, (R.oab_patch(a, b, 16384), a))
    return items


_FRESH = None


def check_equivalence(L):
    global _FRESH
    if _FRESH is None:
        _FRESH = fresh_items()
    items = _FRESH
    assert len(items) == 48
    api.oab_batch_counts(reset=True, L=L)
    alone = [api.oab_decompress(blob, base, L=L) for blob, base in items]
    assert api.oab_batch_counts(L=L) == (48, 0, 0) and all(e == 0 and o for e, o in alone)
    api.oab_batch_counts(reset=True, L=L)
    assert api.oab_decompress_many(items, L=L) == alone
    assert api.oab_batch_counts(L=L) == (1, 48, 0)


def check_messages_and_calls(L):
    """through an in-memory mspack_system: the loop and the one call say the same lines, and the call keeps at most three files open"""
    c = {x[0]: x for x in cases()}
    picks = [c["full_tiny"], c["patch_one_block"], c["full_mixed_stored"]]
    mem = api.MemSystem(L or M.lib())
    jobs = []
    for k, (_n, blob, base, _w) in enumerate(picks):
        mem.files[b"in%d" % k] = blob
        if base is not None:
            mem.files[b"base%d" % k] = base
        jobs.append((b"in%d" % k, None if base is None else b"base%d" % k, b"out%d" % k))
    most = [0]
    opened = mem._cbs[0]

    def watch(*a):
        h = opened(*a)
        most[0] = max(most[0], len(mem._open))
        return h
    cb = type(opened)(watch)
    mem.sys.open = C.cast(cb, C.c_void_p).value
    assert api.oab_decompress_paths(jobs * 4, L=L, sys=mem) == (ERR_OK, [0] * 12)
    assert [bytes(mem.outputs[b"out%d" % k]) for k in range(3)] == [p[3] for p in picks]
    assert mem.messages == [] and 1 <= most[0] <= 3


def check_own_output(L):
    """a job that names its own input (or base) as its output has it opened where the lone call opens it -- before the blocks are
    read -- and runs alone, between the batches of its neighbours"""
    c = {x[0]: x for x in cases()}
    tiny, tiny_plain = c["full_tiny"][1], c["full_tiny"][3]
    _n, patch, base, v2 = c["patch_one_block"]
    mem = api.MemSystem(L or M.lib())
    mem.files.update({b"a": tiny, b"b": tiny, b"c": tiny, b"p": patch, b"base": base})
    api.oab_batch_counts(reset=True, L=L)
    jobs = [(b"a", None, b"oa"), (b"b", None, b"b"), (b"c", None, b"oc"), (b"p", b"base", b"base"), (b"a", None, b"oa2")]
    assert api.oab_decompress_paths(jobs, L=L, sys=mem) == (ERR_OK, [0] * 5)
    assert [bytes(mem.outputs[k]) for k in (b"oa", b"b", b"oc", b"base", b"oa2")] == [tiny_plain] * 3 + [v2, tiny_plain]
    assert api.oab_batch_counts(L=L) == (5, 5, 0)


TESTS = [check_undamaged, check_damaged, check_truncated_and_short_base, check_chain, check_arguments, check_equivalence,
         check_messages_and_calls, check_own_output]


@pytest.mark.parametrize("check", TESTS, ids=[t.__name__[6:] for t in TESTS])
def test_many_host_logic_cpu(built, hostlogic, check):
    check(hostlogic)


@pytest.mark.gpu
@pytest.mark.parametrize("check", TESTS, ids=[t.__name__[6:] for t in TESTS])
def test_many_gpu(built, check):
    assert M.features() & M.FEAT_CRC32
    check(None)


def test_budget_host_logic_cpu(built, hostlogic):
    check_budget(hostlogic, hostlogic.mspack_hip_set_cache_mb, hostlogic.mspack_hip_cache_mb)


@pytest.mark.gpu
def test_budget_gpu(built):
    L = M.lib()
    check_budget(None, L.mspack_hip_set_cache_mb, L.mspack_hip_cache_mb)


# ---- a shared batch that fails (CPU only) -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poisonable(hostlogic):
    """the host drivers on the stand-in, behind a batch call that fails for a batch holding a unit that begins with "POISONED" """
    bdir = os.path.join(HERE, "_build")
    so = os.path.join(bdir, "libhostlogic_oab_poison.so")
    srcs = sorted(glob.glob(os.path.join(ROOT, "libmspack_amd", "csrc", "host", "*.c"))) + \
        [os.path.join(HERE, "csrc", "oab_poison_provider.c"), os.path.join(HERE, "csrc", "batch_standin.c")] + \
        sorted(glob.glob(os.path.join(ROOT, "oracle", "*_oracle.c")))
    deps = srcs + glob.glob(os.path.join(ROOT, "include", "*.h")) + glob.glob(os.path.join(ROOT, "oracle", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        objs = []
        for s in srcs:
            o = os.path.join(bdir, "oab_poison_" + os.path.basename(s) + ".o")
            rename = ["-Dmspack_hip_decode_batch=standin_decode_batch"] if s.endswith("batch_standin.c") else []
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "include")] + rename +
                                  ["-c", s, "-o", o])
            objs.append(o)
        subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-lpthread"])
    return C.CDLL(so)


def poisoned_file():
    """a full file of one compressed block whose stream begins with the word the provider fails on"""
    return struct.pack("<IIII", 3, 1, 4096, 10) + struct.pack("<IIII", 1, 16, 10, 0) + b"POISONED" + b"\0" * 8


def test_a_shared_batch_that_fails(built, poisonable):
    """one bad file must not change its neighbours' answers: each job of the failed batch is decoded again alone, and only the job
    whose own batch fails says so and answers MSPACK_ERR_DECRUNCH -- lines and answers as the loop of lone calls gives them"""
    L = poisonable
    c = {x[0]: x for x in cases()}
    files = [c["full_tiny"][1], poisoned_file(), c["full_mixed_stored"][1], poisoned_file(), c["full_tiny"][1]]
    plains = [c["full_tiny"][3], b"", c["full_mixed_stored"][3], b"", c["full_tiny"][3]]

    def system():
        mem = api.MemSystem(L)
        for k, f in enumerate(files):
            mem.files[b"in%d" % k] = f
        return mem
    alone = system()
    api.oab_batch_counts(reset=True, L=L)
    errs = [api.oab_decompress_paths([(b"in%d" % k, None, b"out%d" % k)], L=L, sys=alone)[1][0] for k in range(5)]
    assert errs == [0, ERR_DECRUNCH, 0, ERR_DECRUNCH, 0] and api.oab_batch_counts(L=L) == (5, 5, 0)
    assert alone.messages == [b"GPU batch decode failed: %s"] * 2
    mem = system()
    api.oab_batch_counts(reset=True, L=L)
    assert api.oab_decompress_paths([(b"in%d" % k, None, b"out%d" % k) for k in range(5)], L=L, sys=mem) == (ERR_OK, errs)
    assert api.oab_batch_counts(L=L) == (6, 5, 5)               # the shared batch, then each of its five jobs alone
    assert mem.messages == alone.messages
    assert [bytes(mem.outputs[b"out%d" % k]) for k in range(5)] == plains == [bytes(alone.outputs[b"out%d" % k]) for k in range(5)]
    # ... and decompress() itself says and answers what it always did
    d = api._setup_oab(L).mspack_create_oab_decompressor(mem.ptr())
    try:
        assert d.contents.decompress(d, b"in1", b"lone") == ERR_DECRUNCH and mem.messages == alone.messages + alone.messages[:1]
        assert bytes(mem.outputs[b"lone"]) == b""
    finally:
        L.mspack_destroy_oab_decompressor(d)
