"""mspack_cabd_prefetch (include/mspack.h): the folders of MANY cabinets in one batch, said by the caller before the extract() calls.

It is advice: every extract() must return, write and say what it does without the call -- so the yardstick of every test here is the
same extracts on a fresh decompressor with no prefetch (and, where it is built, the real reference per cabinet; for the driver
goldens and the split sets what the reference answered when they were recorded).  What the call adds is counted: the stand-in's
jobs (tests/csrc/batch_standin.c: lazy, nothing is decoded before it is waited for) on the CPU, mspack_hip_host_path_stats() calls
on the GPU.  CPU tests run the drivers (csrc/host/cabd.c) on that stand-in; the `gpu` ones the same scenarios on the real library."""
import collections
import ctypes as C
import glob
import hashlib
import os
import subprocess
import zlib

import numpy as np
import pytest

import libmspack_amd as M
from libmspack_amd import api
import helpers
import test_gpu_drivers as GD
import test_cabsets as CS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = 32768
MSZIP, QTM, LZX = 1, 2, 3
MSPACK_ERR_DECRUNCH = 11


# ---- cabinets -------------------------------------------------------------------------------------------------------------
def mszip_folder(data):
    data = bytes(data)
    blocks, usz, d = [], [], None
    for p in range(0, len(data), FB):
        co = zlib.compressobj(6, zlib.DEFLATED, -15) if d is None else zlib.compressobj(6, zlib.DEFLATED, -15, zdict=d)
        d = data[p:p + FB]
        blocks.append(b"CK" + co.compress(d) + co.flush())
        usz.append(len(d))
    return (MSZIP, blocks, usz)


def lzx_folder(data, wb, intel_filesize=0):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    lz, fo = M.lzx_encode(data, wb, 0, M.lzx_opts(intel_filesize=intel_filesize) if intel_filesize else None)
    blocks = [lz[int(fo[i]):int(fo[i + 1])].tobytes() for i in range(len(fo) - 1)]
    return (LZX | (wb << 8), blocks, [min(FB, data.size - i * FB) for i in range(len(blocks))])


def qtm_folder(data, wb):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    qs, fs = M.qtm_encode(data, wb)
    pos, blocks = 0, []
    for k in fs:                                              # (the encoder's stream carries the feeder's 0xFF behind each frame)
        blocks.append(qs[pos:pos + int(k)]); pos += int(k) + 1
    return (QTM | (wb << 8), blocks, [min(FB, data.size - i * FB) for i in range(len(blocks))])


def stored_folder(data):
    data = bytes(data)
    return (0, [data[p:p + FB] for p in range(0, len(data), FB)], [len(data[p:p + FB]) for p in range(0, len(data), FB)])


def flip_payload_byte(cab, folder, block, at=10):
    """damage one payload byte of a CFDATA block (cabinets of M.cab_write: CFHEADER without reserve fields) -- its checksum fails"""
    import struct
    b = bytearray(cab)
    p = struct.unpack_from("<I", b, 36 + 8 * folder)[0]
    for _ in range(block):
        p += 8 + struct.unpack_from("<H", b, p + 4)[0]
    b[p + 8 + at] ^= 0x40
    return bytes(b)


_MIXED = None


def mixed_cabinets():
    """scenario 1's eight small cabinets -> [(image, [plaintext of every file])]; built once, never changed"""
    global _MIXED
    if _MIXED is not None:
        return _MIXED
    out = []

    def add(folders, files, damage=None):
        img = M.cab_write([f for f, _d in folders], files)
        if damage:
            img = flip_payload_byte(img, *damage)
        out.append((img, [bytes(folders[fi][1][off:off + ln]) for _nm, ln, off, fi in files]))
    pt = lambda seed, kind, n: M.gen_plaintext(seed, kind, n).tobytes()
    # three cabinets of one MSZIP folder, 1 - 3 blocks
    d = pt(11, 0, 20001); add([(mszip_folder(d), d)], [(b"m1.txt", len(d), 0, 0)])
    d = pt(12, 0, 50000); add([(mszip_folder(d), d)], [(b"m2a.txt", 30000, 0, 0), (b"m2b.txt", 20000, 30000, 0)])
    d = pt(13, 2, 2 * FB + 777); add([(mszip_folder(d), d)], [(b"m3.bin", len(d), 0, 0)])
    # two LZX cabinets, windows 15 and 16, two folders of 2 - 3 frames; one folder with the E8 translation on
    a, b = pt(14, 0, 2 * FB), pt(15, 1, 2 * FB + 14097)
    add([(lzx_folder(np.frombuffer(a, np.uint8), 15), a), (lzx_folder(np.frombuffer(b, np.uint8), 15), b)],
        [(b"l15a.txt", len(a), 0, 0), (b"l15b.txt", 70000, 0, 1), (b"l15c.txt", len(b) - 70000, 70000, 1)])
    a, b = pt(16, 2, 2 * FB + 5), pt(17, 0, FB + 12345)
    add([(lzx_folder(np.frombuffer(a, np.uint8), 16, intel_filesize=len(a)), a), (lzx_folder(np.frombuffer(b, np.uint8), 16), b)],
        [(b"l16a.bin", len(a), 0, 0), (b"l16b.txt", len(b), 0, 1)])
    # one Quantum folder with two files: it carries marks
    d = pt(18, 0, 50000); add([(qtm_folder(np.frombuffer(d, np.uint8), 12), d)], [(b"q1.txt", 33000, 0, 0), (b"q2.txt", 17000, 33000, 0)])
    # one stored folder
    d = pt(19, 0, 3000); add([(stored_folder(d), d)], [(b"s1.txt", 1000, 0, 0), (b"s2.txt", 2000, 1000, 0)])
    # MSZIP with a damaged payload byte in the second folder's second block: that CFDATA checksum fails
    a, b = pt(20, 0, 40000), pt(21, 0, 2 * FB)
    add([(mszip_folder(a), a), (mszip_folder(b), b)], [(b"ok.txt", len(a), 0, 0), (b"bad1.txt", FB, 0, 1), (b"bad2.txt", FB, FB, 1)],
        damage=(1, 1))
    _MIXED = out
    return out


# ---- running -----------------------------------------------------------------------------------------------------------------
def jobs_counter(L):
    if L is None:
        return lambda: 0
    L.mspack_standin_jobs_begun.restype = C.c_ulong
    return lambda: L.mspack_standin_jobs_begun()


def close_cab(s, i):
    """close() cabinet i of the CabSet now (none of these is joined to another); the others stay open"""
    s.d.contents.close(s.d, s.cabs[i])
    s.cabs[i] = None


def run_session(images, order, L=None, prefetch=None, params=(), close_first=(), **kw):
    """one decompressor over `images` (bytes in an in-memory mspack_system, or paths); prefetch: None = no call, else a list of
    cabinet indices ("all" = every one); then extract `order` = [(cabinet, file index)].
    -> dict(res=[(err, bytes)], rc=prefetch's return, jobs=(begun by the prefetch, begun by the extracts), messages=[...],
            listing=[per cabinet: [(name, length, offset)] of its file list, None where it did not open])"""
    begun = jobs_counter(L)
    mem = not isinstance(images[0], str)
    with api.CabSet(images, mem=mem, L=L, **kw) as s:
        for p, v in params:
            assert s.d.contents.set_param(s.d, p, v) == 0
        listing = [[(f[0].decode("latin1"), f[1], f[2]) for f in s.files(c)] if s.cabs[c] else None for c in range(len(images))]
        b0 = begun()
        rc = None
        if prefetch is not None:
            rc = s.prefetch(None if prefetch == "all" else prefetch)
            assert s.d.contents.last_error(s.d) == rc
        b1 = begun()
        for c in close_first:
            close_cab(s, c)
        ptrs = {}
        res = []
        for c, i in order:
            if c not in ptrs:
                ptrs[c] = s.file_ptrs(c)
            res.append(s.extract(ptrs[c][i]))
        b2 = begun()
        msgs = list(s.mem.messages) if mem else []
        open_errors = list(s.open_errors)
    return dict(res=res, rc=rc, jobs=(b1 - b0, b2 - b1), messages=msgs, open_errors=open_errors, listing=listing)


def orders_of(cabs):
    n = [len(pl) for _img, pl in cabs]
    asc = [(c, i) for c in range(len(cabs)) for i in range(n[c])]
    inter = [(c, i) for i in range(max(n)) for c in range(len(cabs)) if i < n[c]]
    return dict(ascending=asc, descending=asc[::-1], interleaved=inter)


_REF = {}


def ref_per_cabinet(ci, image, idx):
    """the real reference, one decompressor per cabinet, the files `idx` in that order (computed once per cabinet and order)"""
    key = (ci, tuple(idx))
    if key not in _REF:
        rc, outs = helpers.ref_cab_extract(image, list(idx), cap=len(idx) * 4 * FB + 4096)
        assert rc == 0
        _REF[key] = outs
    return _REF[key]


def ref_one_decompressor(images, order):
    """the real reference as a library (oracle/_ref/libmspack_ref.so, the same method table: tests/test_abi.py): every cabinet
    opened on ONE of its decompressors over the in-memory mspack_system, the files of `order` = [(cabinet, file index)] -> [(err, bytes)]"""
    R = C.CDLL(os.path.join(helpers.ORACLE_DIR, "_ref", "libmspack_ref.so"))
    R.mspack_create_cab_decompressor.restype = api._P(api.MscabDecompressor)
    R.mspack_create_cab_decompressor.argtypes = [C.c_void_p]
    R.mspack_destroy_cab_decompressor.argtypes = [api._P(api.MscabDecompressor)]
    mem = api.MemSystem(R)
    d = R.mspack_create_cab_decompressor(mem.ptr())
    assert d
    m = d.contents
    names = [b"mem:in%d" % k for k in range(len(images))]          # (they must outlive the cabinets: mspack.h)
    cabs = []
    for nm, img in zip(names, images):
        mem.files[nm] = bytes(img)
        cabs.append(m.open(d, nm))
        assert cabs[-1]
    files = [list(api._walk(c.contents.files)) for c in cabs]
    res = []
    for c, i in order:
        mem.outputs.clear()
        err = m.extract(d, files[c][i], b"mem:out")
        res.append((err, bytes(mem.outputs.get(b"mem:out", b""))))
    for c in cabs:
        m.close(d, c)
    R.mspack_destroy_cab_decompressor(d)
    return res


def scenario_one_batch(L):
    cabs = mixed_cabinets()
    images = [img for img, _pl in cabs]
    for name, order in orders_of(cabs).items():
        base = run_session(images, order, L=L)
        got = run_session(images, order, L=L, prefetch="all")
        assert got["rc"] == 0 and got["open_errors"] == [0] * len(cabs)
        for (c, i), a, b in zip(order, base["res"], got["res"]):
            assert a == b, (name, c, i, a[0], b[0], len(a[1]), len(b[1]))
            if c != 7 or i == 0:
                assert b == (0, cabs[c][1][i]), (name, c, i, b[0])
            else:
                assert b[0] != 0, (name, c, i)
        if L is not None:
            assert got["jobs"][0] == 1 and got["jobs"][1] <= 1, (name, got["jobs"])      # (<= 1: the bad folder's re-gather)
        if helpers.have_ref():
            # the reference with all eight cabinets on one decompressor, the same calls in the same order
            assert ref_one_decompressor(images, order) == got["res"], name
        if helpers.have_ref() and name != "interleaved":
            # ... and one reference decompressor per cabinet (per cabinet the files come one behind the other in these two orders,
            # so it sees the calls that cabinet sees here)
            for c in range(len(cabs)):
                idx = [i for cc, i in order if cc == c]
                want = ref_per_cabinet(c, images[c], idx)
                mine = [r for (cc, _i), r in zip(order, got["res"]) if cc == c]
                assert [(e, bytes(d)) for e, d in want] == mine, (name, c)


def test_one_batch_same_answers_cpu(built, hostlogic):
    scenario_one_batch(hostlogic)


@pytest.mark.gpu
def test_one_batch_same_answers_gpu(built):
    scenario_one_batch(None)


# ---- the driver goldens, all in one batch -----------------------------------------------------------------------------------
def scenario_goldens(vecs, L):
    groups = collections.OrderedDict()
    for v in vecs:
        p = v["params"]
        groups.setdefault((p.get("fix_mszip", 0), p.get("salvage", 0)), []).append(v)
    for (fix, salv), vs in groups.items():
        # every recorded run is one cabinet object of its own (it was recorded on a fresh decompressor: no state of an earlier run
        # of the same cabinet may reach it), all of them on ONE decompressor
        images, plan = [], []
        for v in vs:
            for run in (v["runs"] or [None]):
                plan.append((v, run, len(images)))
                images.append(GD.cab_bytes(v))
        order = [(c, i) for _v, run, c in plan if run for i in run["order"]]
        sess = {}
        for pf in (None, "all"):
            sess[pf] = run_session(images, order, L=L, prefetch=pf, fix_mszip=fix, salvage=salv)
        got = sess["all"]
        assert got["rc"] == 0
        k = 0
        for v, run, c in plan:
            assert got["open_errors"][c] == v["open_err"], v["tag"]
            if not run:
                continue
            assert got["listing"][c] == [(f["name"], f["length"], f["offset"]) for f in v["files"]], v["tag"]
            for idx, exp in zip(run["order"], run["results"]):
                err, data = got["res"][k]; k += 1
                tag = "%s file %d (order %s)" % (v["tag"], idx, run["order"])
                assert err == exp["err"], (tag, err, exp)
                if exp["err"] == 0:
                    assert len(data) == exp["n"] and hashlib.md5(data).hexdigest() == exp["md5"], tag
        assert got["res"] == sess[None]["res"]
        # the prefetch says nothing of its own, and nothing is said twice
        assert collections.Counter(got["messages"]) == collections.Counter(sess[None]["messages"]), (fix, salv)
        if L is not None:
            assert got["jobs"][0] == 1


def test_driver_goldens_in_one_batch_cpu(built, hostlogic):
    scenario_goldens(GD.CPU_VECS, hostlogic)


@pytest.mark.gpu
def test_driver_goldens_in_one_batch_gpu(built):
    scenario_goldens(GD.VECS, None)


# ---- sets ---------------------------------------------------------------------------------------------------------------------
def chain_of(cab):
    """the addresses of the cabinets joined to this one, itself included (prevcab / nextcab)"""
    out = {C.addressof(cab.contents)}
    for step in ("prevcab", "nextcab"):
        w = getattr(cab.contents, step)
        while w:
            out.add(C.addressof(w.contents)); w = getattr(w.contents, step)
    return out


@pytest.mark.parametrize("which", ["head", "middle"])
@pytest.mark.parametrize("sc", CS.CODED, ids=[s["name"] for s in CS.CODED])
def test_prefetch_of_a_set_cpu(built, hostlogic, sc, which):
    """Answers: the goldens.  Batches: the prefetch of a member is the batch that the first extract() of the set's list would have
    started -- so a set that extracts whole (every golden answer OK, several folders) is exactly one job at the prefetch and none
    at the extracts; in general, where the prefetched cabinet is joined to the listed one, the prefetch starts as many jobs as the
    same extracts start without it and the extracts start none; where the join was refused and it is a cabinet of its own, the
    listed one's extracts start what they start without the call."""
    begun = jobs_counter(hostlogic)
    jobs, out = {}, {}
    for pf in (False, True):
        with api.CabSet([CS.fixture(c) for c in sc["cabs"]], L=hostlogic) as s:
            CS.run_ops(s, sc["ops"])
            member = 0 if which == "head" else len(sc["cabs"]) // 2
            joined = C.addressof(s.cabs[member].contents) in chain_of(s.cabs[sc["list_cab"]])
            folders = {f[4] for f in s.files(sc["list_cab"])}
            b0 = begun()
            if pf:
                assert s.prefetch([member]) == 0
            b1 = begun()
            out[pf] = []
            for fp, f in zip(s.file_ptrs(sc["list_cab"]), sc["files"]):
                err, data = s.extract(fp)
                out[pf].append((f["name"], err, len(data), hashlib.md5(data).hexdigest()))
            jobs[pf] = (b1 - b0, begun() - b1)
    want = [(f["name"], f["err"], f["out_len"], f["md5"]) for f in sc["files"]]
    assert out[True] == want and out[False] == want
    if joined:
        assert jobs[True] == (jobs[False][1], 0), (jobs, which)
        if len(folders) >= 2 and all(f["err"] == 0 for f in sc["files"]):
            assert jobs[True] == (1, 0), (jobs, which)
    else:
        assert jobs[True][1] == jobs[False][1] and jobs[True][0] <= 1, (jobs, which)


# ---- budget ---------------------------------------------------------------------------------------------------------------------
def test_prefetch_keeps_to_the_cache_budget_cpu(built, hostlogic):
    """MSCABD_PARAM_HIP_CACHE_MB = 1: 32 blocks' worth of estimate.  Six cabinets of three MSZIP folders of four blocks (128 KiB
    estimated per folder, 2.25 MiB in all): the prefetch takes the first eight folders -- cabinets 0 and 1 and two folders of
    cabinet 2 -- and leaves the rest to their extract(): cabinet 2's last folder alone (one folder: no job), cabinets 3 - 5 as one
    job each, started by their first extract()."""
    nc, nf, nb = 6, 3, 4
    cabs = []
    for c in range(nc):
        datas = [M.gen_plaintext(100 + c * nf + f, 0, nb * FB).tobytes() for f in range(nf)]
        cabs.append((M.cab_write([mszip_folder(d) for d in datas], [(b"f%d" % f, nb * FB, 0, f) for f in range(nf)]), datas))
    images = [img for img, _d in cabs]
    begun = jobs_counter(hostlogic)
    with api.CabSet(images, mem=True, L=hostlogic) as s:
        assert s.d.contents.set_param(s.d, api.MSCABD_PARAM_HIP_CACHE_MB, 1) == 0
        b0 = begun()
        assert s.prefetch() == 0
        assert begun() == b0 + 1
        for c in range(nc):
            for f in range(nf):
                before = begun()
                err, data = s.extract(s.file_ptrs(c)[f])
                assert (err, data) == (0, cabs[c][1][f]), (c, f, err)
                assert begun() - before == (1 if (c >= 3 and f == 0) else 0), (c, f)
    base = run_session(images, [(c, f) for c in range(nc) for f in range(nf)], L=hostlogic,
                       params=[(api.MSCABD_PARAM_HIP_CACHE_MB, 1)])
    assert base["res"] == [(0, cabs[c][1][f]) for c in range(nc) for f in range(nf)]


# ---- the synchronous path -------------------------------------------------------------------------------------------------------
class CountingFiles(dict):
    """api.MemSystem.files that counts the opens for reading: the driver opens a cabinet once per folder it gathers"""
    opens = 0

    def __getitem__(self, k):
        self.opens += 1
        return dict.__getitem__(self, k)


_BUDGET = None


def budget_cabinets():
    """the damaged cabinet of scenario 1 (two folders of two blocks, the second with a bad CFDATA checksum), then six cabinets of
    three MSZIP folders of four blocks"""
    global _BUDGET
    if _BUDGET is None:
        _BUDGET = [mixed_cabinets()[7]]
        for c in range(6):
            datas = [M.gen_plaintext(300 + c * 3 + f, 0, 4 * FB).tobytes() for f in range(3)]
            _BUDGET.append((M.cab_write([mszip_folder(d) for d in datas], [(b"f%d" % f, 4 * FB, 0, f) for f in range(3)]), datas))
    return _BUDGET


def sync_session(L, mode, prefetch, fix_mszip=0):
    cabs = budget_cabinets()
    with api.CabSet([img for img, _d in cabs], mem=True, L=L, fix_mszip=fix_mszip) as s:
        s.mem.files = CountingFiles(s.mem.files)
        if mode == "two_devices":
            assert s.d.contents.set_param(s.d, api.MSCABD_PARAM_HIP_DEVICES, 2) == 0
        assert s.d.contents.set_param(s.d, api.MSCABD_PARAM_HIP_CACHE_MB, 1) == 0
        rc = None
        if prefetch:
            rc = s.prefetch()
            assert s.d.contents.last_error(s.d) == rc
        pf_opens, pf_msgs = s.mem.files.opens, list(s.mem.messages)
        res, opens = [], {}
        for c in range(len(cabs)):
            for i, fp in enumerate(s.file_ptrs(c)):
                o = s.mem.files.opens
                res.append(s.extract(fp))
                opens[(c, i)] = s.mem.files.opens - o
        return dict(rc=rc, res=res, pf_opens=pf_opens, pf_msgs=pf_msgs, opens=opens, messages=list(s.mem.messages))


@pytest.mark.parametrize("mode", ["jobs_off", "two_devices"])
def test_synchronous_prefetch_cpu(built, hostlogic, monkeypatch, mode):
    """MSPACK_HIP_JOBS=0, or devices = 2: the prefetch decodes before it returns, with a budget of 1 MiB = 32 blocks of estimate.
    Round one takes the damaged cabinet's two folders (2 + 2 blocks) and seven folders of four: cabinets 1 and 2 and folder 0 of
    cabinet 3 -- nine folders, nine opens.  The damaged folder comes back flagged and is gathered again on the host in a second
    round, which starts from what round one kept (30 blocks): the flagged folder's 2 blocks fit, no other folder does -- ten opens
    in all.  The extracts then open a cabinet only for what the prefetch left: folders 1 and 2 of cabinet 3 in one batch (two opens
    at the first of them), cabinets 4 - 6 whole (three opens at their first file).  No job is ever begun.  Answers and messages are
    those of the same extracts without the call."""
    if mode == "jobs_off":
        monkeypatch.setenv("MSPACK_HIP_JOBS", "0")
    begun = jobs_counter(hostlogic)
    b0 = begun()
    base = sync_session(hostlogic, mode, False)
    got = sync_session(hostlogic, mode, True)
    assert begun() == b0
    assert got["rc"] == 0 and got["pf_opens"] == 10 and got["pf_msgs"] == []
    assert got["res"] == base["res"]
    cabs = budget_cabinets()
    want = [(0, cabs[0][1][0])] + [(0, d) for _img, datas in cabs[1:] for d in datas]
    assert [r for r in got["res"] if r[0] == 0] == want and [r[0] != 0 for r in got["res"][:3]] == [False, True, True]
    assert collections.Counter(got["messages"]) == collections.Counter(base["messages"])
    left = {(3, 1): 2, (4, 0): 3, (5, 0): 3, (6, 0): 3}
    assert got["opens"] == {k: left.get(k, 0) for k in got["opens"]}, got["opens"]
    assert base["opens"] == {(c, i): (3 if i == 0 else 0) for c, i in base["opens"]}, base["opens"]     # (every cabinet at its first file)


def test_synchronous_prefetch_that_fails_cpu(built, hostlogic, monkeypatch):
    """a synchronous batch call that fails (the stand-in has no MSZIP repair mode: fix_mszip = 1 makes its call fail) is
    MSPACK_ERR_DECRUNCH with the driver's message, nothing is kept of it, and the extracts answer what they answer without the call"""
    monkeypatch.setenv("MSPACK_HIP_JOBS", "0")
    base = sync_session(hostlogic, "jobs_off", False, fix_mszip=1)
    got = sync_session(hostlogic, "jobs_off", True, fix_mszip=1)
    assert got["rc"] == MSPACK_ERR_DECRUNCH
    assert got["pf_msgs"] == [b"GPU batch decode failed: %s"]
    assert [e for e, _d in got["res"]] == [e for e, _d in base["res"]] == [MSPACK_ERR_DECRUNCH] * len(base["res"])
    assert got["messages"][1:] == base["messages"]


# ---- close while the job runs -----------------------------------------------------------------------------------------------------
def small_cabinets(n, seed=500, folders=2):
    out = []
    for c in range(n):
        datas = [M.gen_plaintext(seed + c * folders + f, 0, FB).tobytes() for f in range(folders)]
        out.append((M.cab_write([mszip_folder(d) for d in datas], [(b"f%d" % f, FB, 0, f) for f in range(folders)]), datas))
    return out


def test_closing_one_cabinet_leaves_the_batch_to_the_others_cpu(built, hostlogic):
    cabs = small_cabinets(4)
    order = [(c, f) for c in (3, 1, 2) for f in (1, 0)]
    got = run_session([img for img, _d in cabs], order, L=hostlogic, prefetch="all", close_first=[0])
    assert got["rc"] == 0 and got["jobs"] == (1, 0)
    assert got["res"] == [(0, cabs[c][1][f]) for c, f in order]


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_prefetch_arguments_cpu(built, hostlogic):
    cabs = small_cabinets(2, seed=600)
    d = M.gen_plaintext(7, 0, 3000).tobytes()
    stored = M.cab_write([stored_folder(d)], [(b"s", len(d), 0, 0)])
    begun = jobs_counter(hostlogic)
    L = api._setup(hostlogic)
    assert L.mspack_cabd_prefetch(None, None, 0) == api.MSPACK_ERR_ARGS
    with api.CabSet([cabs[0][0], cabs[1][0], stored], mem=True, L=hostlogic) as s:
        last = lambda: s.d.contents.last_error(s.d)
        b0 = begun()
        arr = (api._P(api.MscabdCabinet) * 2)(s.cabs[0], None)
        assert L.mspack_cabd_prefetch(s.d, arr, 2) == api.MSPACK_ERR_ARGS and last() == api.MSPACK_ERR_ARGS
        assert L.mspack_cabd_prefetch(s.d, arr, -1) == api.MSPACK_ERR_ARGS and last() == api.MSPACK_ERR_ARGS
        assert L.mspack_cabd_prefetch(s.d, None, 1) == api.MSPACK_ERR_ARGS and last() == api.MSPACK_ERR_ARGS
        assert s.prefetch([]) == 0 and last() == 0
        assert L.mspack_cabd_prefetch(s.d, None, 0) == 0
        assert s.prefetch([2]) == 0                              # only stored folders
        assert begun() == b0                                     # (none of these gathered anything)
        assert s.prefetch([0, 1, 1, 0]) == 0 and begun() == b0 + 1
        assert s.prefetch([0, 1, 1, 0]) == 0 and begun() == b0 + 1        # nothing left to decode
        for c in (1, 0):
            for f in (0, 1):
                assert s.extract(s.file_ptrs(c)[f]) == (0, cabs[c][1][f])
        assert s.prefetch() == 0 and begun() == b0 + 1
        assert s.extract(s.file_ptrs(2)[0]) == (0, d)


# ---- sanitizers, stand-alone ---------------------------------------------------------------------------------------------------------
def test_prefetch_check_under_asan_ubsan(built, tmp_path):
    """tests/csrc/prefetch_check.c: a program of its own (no python in the process) on the drivers + the stand-in + the oracle, all
    compiled with -fsanitize=address,undefined; it reads the cabinets this test writes and checks the extracts against the
    plaintext files beside them.  Any report -- leaks included -- fails.  The runtimes are linked statically, so the program starts
    the same whatever else the environment has the loader bring in; a gcc without them fails the test."""
    exe = str(tmp_path / "prefetch_check")
    srcs = [os.path.join(ROOT, "tests", "csrc", "prefetch_check.c")] + \
        sorted(glob.glob(os.path.join(ROOT, "libmspack_amd", "csrc", "host", "*.c"))) + \
        [os.path.join(ROOT, "tests", "csrc", "batch_standin.c")] + sorted(glob.glob(os.path.join(ROOT, "oracle", "*_oracle.c")))
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-o", exe] + srcs + ["-lpthread"])
    args = []
    for k, (img, plains) in enumerate(mixed_cabinets()):
        (tmp_path / ("mixed%d.cab" % k)).write_bytes(img)
        for i, pl in enumerate(plains):
            (tmp_path / ("mixed%d.cab.%d" % (k, i))).write_bytes(pl)
        args.append(str(tmp_path / ("mixed%d.cab" % k)))
    for c in ("split-1.cab", "split-2.cab", "split-3.cab"):          # a set: its last member's file is removed by the program
        (tmp_path / c).write_bytes(open(CS.fixture(c), "rb").read())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, str(tmp_path)] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0 and "PREFETCH_CHECK_OK" in out, out[-4000:]
    assert "Sanitizer" not in out and "runtime error" not in out, out[-4000:]


# ---- GPU: larger batches ---------------------------------------------------------------------------------------------------------------
def host_path_calls():
    L = M.lib()
    ms = (C.c_double * 4)()
    L.mspack_hip_host_path_stats.restype = None
    L.mspack_hip_host_path_stats.argtypes = [C.POINTER(C.c_double), C.c_int]
    L.mspack_hip_host_path_stats(ms, 0)
    return ms[3]


@pytest.mark.gpu
def test_256_cabinets_are_one_batch_gpu(built):
    n = 256
    plain = M.gen_plaintext(0xC0FFEE, 0, n * FB)
    images = []
    for c in range(n):
        images.append(M.cab_write([mszip_folder(plain[c * FB:(c + 1) * FB].tobytes())], [(b"f%04d.bin" % c, FB, 0, 0)]))
    with api.CabSet(images, mem=True) as s:
        c0 = host_path_calls()
        assert s.prefetch() == 0
        for c in list(range(n - 1, n - 9, -1)) + list(range(n)):
            err, data = s.extract(s.file_ptrs(c)[0])
            assert err == 0 and data == plain[c * FB:(c + 1) * FB].tobytes(), c
        assert host_path_calls() - c0 == 1


@pytest.mark.gpu
def test_mixed_lzx_and_quantum_prefetch_gpu(built):
    """32 LZX-16 cabinets of two 2-frame folders and 8 Quantum cabinets (window 12, 64 KiB) in one prefetch, every byte against the
    CPU oracle's decoding of the same folder streams (and so against the plaintext they were made from)"""
    cabs = []
    for c in range(32):
        ds = [M.gen_plaintext(900 + 2 * c + f, c % 3, 2 * FB) for f in range(2)]
        fo = [lzx_folder(d, 16) for d in ds]
        want = []
        for d, (_ct, blocks, _u) in zip(ds, fo):
            e, o, _r = helpers.oracle_lzx(b"".join(blocks), d.size, 16, 0)
            assert e == 0
            want.append(o)
        cabs.append((M.cab_write(fo, [(b"a", 2 * FB, 0, 0), (b"b", 2 * FB, 0, 1)]), want))
    for c in range(8):
        d = M.gen_plaintext(990 + c, c % 2, 2 * FB)
        fo = qtm_folder(d, 12)
        e, o, _r = helpers.oracle_qtm(b"".join(b + b"\xff" for b in fo[1]), d.size, 12)
        assert e == 0
        cabs.append((M.cab_write([fo], [(b"q1", 40000, 0, 0), (b"q2", 2 * FB - 40000, 40000, 0)]), [o[:40000], o[40000:]]))
    with api.CabSet([img for img, _w in cabs], mem=True) as s:
        assert s.prefetch() == 0
        for c in reversed(range(len(cabs))):
            for i, w in enumerate(cabs[c][1]):
                err, data = s.extract(s.file_ptrs(c)[i])
                assert err == 0 and data == bytes(w), (c, i, err)


# ---- the measurement leg's harness (csrc/bench/api_bench.c: mspk_api_bench_cabs) ------------------------------------------------------
from test_api_bench import harness_cpu  # noqa: E402,F401  (the fixture: api_bench.c + the drivers + the stand-in in one CPU library)


def test_many_cabinets_harness_cpu(harness_cpu):
    from libmspack_amd import apibench
    L = harness_cpu
    L.mspk_api_bench_cabs.restype = C.c_int
    L.mspk_api_bench_cabs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(apibench.Stats)]
    begun = jobs_counter(L)
    images, plain = apibench.build_small_cabs(M, n=24)
    for pf in (0, 1):
        b0 = begun()
        rc, out, d = apibench.run_cabs(images, plain.size, pf, L=L)
        assert rc == 0 and d["n_errors"] == 0 and d["n_files"] == 24 and np.array_equal(out, plain), (pf, rc, d)
        assert begun() - b0 == pf              # (one folder per cabinet: without the prefetch no batch is large enough to be a job)
