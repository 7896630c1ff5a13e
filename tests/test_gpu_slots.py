"""GPU: context slots (include/mspack_hip.h: mspack_hip_set_slots) -- batches of several application threads side by side on one
device, each in a slot with arenas, staging, streams and events of its own.  What must hold: every byte and every result of a batch
are those it has alone with one slot, whatever runs beside it; never more batches hold slots of the device than slots are
configured; with more than one slot batches of different threads really meet; with one slot they never do.

    batch level   four Python threads (ctypes gives the GIL up for the call), each with a batch of its own -- 64 LZX-16 units of two
                  frames, 64 MSZIP units, 8 Quantum units of 64 KiB, a mixed batch with MD5 and SHA digest units --, a barrier in
                  front of each of 8 rounds; with 2, with 4 and with 1 slot, against the same batches decoded by one thread, one slot
    object level  four threads, each with a decompressor of its own: two cabinets and two CHMs of the driver goldens, every
                  extraction order the goldens hold (the CHMs' chunks run as jobs), 2 slots: the goldens' bytes and error codes
    jobs          a job beside another thread's synchronous call, 2 slots: _wait_unit answers before _end, both results correct
    entry points  _to_device beside another thread's batch, and _multi cut into 3 shards on one device (a process of its own),
                  with 2 slots against 1
Shapes: small on purpose (a batch far below the chip is the case slots exist for); every test takes a few seconds."""
import hashlib
import os
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

import libmspack_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ROUNDS = 8
HASH = {M.KIND_MD5: hashlib.md5, M.KIND_SHA1: hashlib.sha1, M.KIND_SHA256: hashlib.sha256}


def lzx16_batch():
    n, ub = 64, 65536
    plain, comp, off, ln, tab = M.corpus_lzx_units(0x510, M.TEXT_MIX, n, ub, 16, n_threads=4, frame_tables=True)
    units, out_bytes = M.make_units(M.KIND_LZX, off, ln + 4, np.full(n, ub), window_bits=16, reset_frames=2, frame_tabs=tab)
    return units, comp, out_bytes


def mszip_batch():
    streams = []
    lens = []
    for i in range(64):
        d = M.gen_plaintext(0x2000 + i, i % 4, 32768 * (1 + i % 3) - 100 * (i % 5))
        blocks, prev = [], None
        for k in range(0, d.size, 32768):
            b = d[k:k + 32768].tobytes()
            c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, 0, prev) if prev else zlib.compressobj(6, zlib.DEFLATED, -15)
            blocks.append(b"CK" + c.compress(b) + c.flush()); prev = b
        streams.append(b"".join(blocks)); lens.append(d.size)
    return pack(M.KIND_MSZIP, streams, lens, 0, out_slack=32768)


def qtm_batch():
    streams = []
    for i in range(8):
        qs, _fs = M.qtm_encode(M.gen_plaintext(0x3000 + i, 0, 65536), 17)
        streams.append(bytes(qs))
    return pack(M.KIND_QUANTUM, streams, [65536] * 8, 17)


def pack(kind, streams, out_lens, wb, out_slack=0):
    offs, pos = [], 0
    for s in streams:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(s)
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for s, o in zip(streams, offs):
        arena[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    units, out_bytes = M.make_units(kind, offs, [len(s) for s in streams], out_lens, window_bits=wb, out_slack=out_slack)
    return units, arena, out_bytes


def digest_batch():
    """a mixed batch (LZX, MSZIP, Quantum with marks) with one digest unit per decoding unit's bytes, MD5 / SHA-1 / SHA-256 in turn"""
    import test_gpu_hostpath as T
    units, arena, out_bytes, items = T.mixed_batch(n_each=8, seed=23)
    kinds = [(M.KIND_MD5, M.KIND_SHA1, M.KIND_SHA256)[i % 3] for i in range(len(units))]
    dg, heads = M.digest_units([(int(u["out_off"]), int(u["out_len"])) for u in units], kinds)
    want = [HASH[k](it[5].tobytes()).digest() for k, it in zip(kinds, items)]
    return np.concatenate([units, dg]), arena, out_bytes, (len(units), dg, want)


@pytest.fixture(scope="module")
def batches(built):
    """the four batches and what one thread with one slot makes of them (computed once, never written again)"""
    M.set_slots(1)
    bs = [lzx16_batch(), mszip_batch(), qtm_batch()]
    du, da, dob, (n_dec, dg, want) = digest_batch()
    bs.append((du, da, dob))
    ref = [M.decode_batch(u, a, ob) for u, a, ob in bs]
    for (u, _a, _ob), (_out, res) in zip(bs[:3], ref[:3]):
        assert (res["err"] == 0).all() and (res["out_len"] == u["out_len"]).all()
    assert M.result_wide_digests(ref[3][1][n_dec:], dg) == want, "the reference run's digests are not the plaintext's"
    for out, res in ref:
        out.setflags(write=False); res.setflags(write=False)
    yield bs, ref
    M.set_slots(1)
    M.lib().mspack_hip_release()           # (the slots beyond the first give their memory back)


def same(units, got, ref):
    """every unit's bytes and every result (the bytes between units are unspecified)"""
    out, res = got
    rout, rres = ref
    if not np.array_equal(res, rres):
        return False
    for u in units:
        if int(u["kind"]) <= M.KIND_XORSUM:
            o, n = int(u["out_off"]), int(u["out_len"])
            if not np.array_equal(out[o:o + n], rout[o:o + n]):
                return False
    return True


def run_threads(bs, rounds):
    """one thread per batch, a barrier in front of every round -> got[t][r]"""
    bar = threading.Barrier(len(bs))
    got = [[None] * rounds for _ in bs]
    errs = []

    def body(t):
        try:
            u, a, ob = bs[t]
            for r in range(rounds):
                bar.wait(timeout=60)
                got[t][r] = M.decode_batch(u, a, ob)
        except BaseException as e:          # (a failing thread must not leave the others at the barrier)
            errs.append((t, repr(e)))
            bar.abort()
    th = [threading.Thread(target=body, args=(t,)) for t in range(len(bs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    return got


@pytest.mark.parametrize("slots", [2, 4, 1])
def test_four_threads_four_batches(batches, slots):
    bs, ref = batches
    try:
        M.set_slots(slots)
        M.slot_stats(reset=True)
        got = run_threads(bs, ROUNDS)
        s = M.slot_stats()
    finally:
        M.set_slots(1)
    print("slots %d: batches %d, at most %d at once, %d waited" % ((slots,) + s))
    for t, (u, _a, _ob) in enumerate(bs):
        for r in range(ROUNDS):
            assert same(u, got[t][r], ref[t]), "slots %d: batch %d differs in round %d from its run alone" % (slots, t, r)
    assert s[0] == len(bs) * ROUNDS
    assert s[1] <= slots
    if slots == 1:
        assert s[1] == 1
    else:
        assert s[1] >= 2, "no two batches ever held slots at the same time"


def test_four_decompressors_of_four_threads(built):
    """the object API as the threading contract has it: a decompressor per thread, here with two slots behind them"""
    import test_gpu_drivers as D
    import test_chm_extract as X
    from libmspack_amd import api
    api._setup()
    cabs = [next(v for v in D.VECS if v["tag"] == t) for t in ("syn:clean", "syn:flip@110799")]
    chms = [next(v for v in X.VECS if v["tag"] == t) for t in ("lzx21-r2", "lzx16-r2-flip@f6")]
    jobs = [(D.replay, cabs[0]), (X.replay, chms[0]), (D.replay, cabs[1]), (X.replay, chms[1])]
    errs = []
    bar = threading.Barrier(len(jobs))

    def body(fn, v):
        try:
            bar.wait(timeout=60)
            fn(v)
        except BaseException as e:
            errs.append((v["tag"], repr(e)))
            bar.abort()
    try:
        M.set_slots(2)
        M.slot_stats(reset=True)
        th = [threading.Thread(target=body, args=j) for j in jobs]
        for t in th:
            t.start()
        for t in th:
            t.join()
        s = M.slot_stats()
    finally:
        M.set_slots(1)
    assert not errs, errs
    print("objects, slots 2: batches %d, at most %d at once, %d waited" % s)
    assert s[0] >= len(jobs) and s[1] <= 2


def test_job_beside_a_synchronous_call(batches):
    bs, ref = batches
    L = M.lib()
    u = np.ascontiguousarray(bs[0][0]).copy(); a = bs[0][1]; ob = bs[0][2]
    out = np.zeros(ob, dtype=np.uint8)
    res = np.zeros(len(u), dtype=M.RESULT_DTYPE)
    other = {}
    bar = threading.Barrier(2)

    def sync_call():
        bar.wait(timeout=60)
        other["got"] = M.decode_batch(*bs[1])
    try:
        M.set_slots(2)
        M.slot_stats(reset=True)
        th = threading.Thread(target=sync_call)
        th.start()
        res["err"] = 0x7777
        bar.wait(timeout=60)
        job = L.mspack_hip_decode_batch_begin(u.ctypes.data, len(u), a.ctypes.data, a.size, out.ctypes.data, out.size, res.ctypes.data)
        assert job
        # out of order, and each unit looked at the moment its wait returns -- before _end
        for i in (len(u) - 1, 0, len(u) // 2):
            assert L.mspack_hip_job_wait_unit(job, i) == 0, L.mspack_hip_last_error()
            assert res[i] == ref[0][1][i]
            o, n = int(u["out_off"][i]), int(u["out_len"][i])
            assert np.array_equal(out[o:o + n], ref[0][0][o:o + n])
        assert L.mspack_hip_job_end(job) == 0, L.mspack_hip_last_error()
        th.join()
        s = M.slot_stats()
    finally:
        M.set_slots(1)
    assert same(bs[0][0], (out, res), ref[0])
    assert same(bs[1][0], other["got"], ref[1])
    assert s[0] == 2 and s[1] <= 2


def test_to_device_beside_another_batch(batches):
    import test_gpu_hostpath as T
    bs, ref = batches
    L = M.lib()
    u0, a, ob = bs[2]

    def to_device():
        d_out = T.DevBuf(ob + 64)
        res = np.zeros(len(u0), dtype=M.RESULT_DTYPE)
        u = np.ascontiguousarray(u0).copy()
        rc = L.mspack_hip_decode_batch_to_device(u.ctypes.data, len(u), a.ctypes.data, a.size, d_out.ptr, ob + 64, res.ctypes.data)
        assert rc == 0, L.mspack_hip_last_error()
        out = d_out.to_host()
        d_out.free()
        return out, res
    one = to_device()
    assert same(u0, one, ref[2])
    other = {}
    bar = threading.Barrier(2)

    def sync_call():
        bar.wait(timeout=60)
        other["got"] = M.decode_batch(*bs[0])
    try:
        M.set_slots(2)
        th = threading.Thread(target=sync_call)
        th.start()
        bar.wait(timeout=60)
        two = to_device()
        th.join()
    finally:
        M.set_slots(1)
    assert same(u0, two, one), "_to_device with two slots differs from one slot"
    assert same(bs[0][0], other["got"], ref[0])


MULTI_WORKER = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np
import libmspack_amd as M
import test_gpu_hostpath as T
import test_gpu_slots as S
units, arena, out_bytes, items = T.mixed_batch(n_each=16, seed=31)
assert M.slots() == 1
one = M.decode_batch(units.copy(), arena, out_bytes, n_devices=2)
T.check(units, one[0], one[1], items)
M.set_slots(2)
M.slot_stats(reset=True)
two = M.decode_batch(units.copy(), arena, out_bytes, n_devices=2)
s = M.slot_stats()
assert S.same(units, two, one), "three shards in two slots differ from one slot"
assert s[0] == 3 and 1 <= s[1] <= 2, s
print("MULTI_SLOTS_OK", s)
'''


def test_multi_three_shards_two_slots(built, tmp_path):
    """mspack_hip_decode_batch_multi cut into three shards on one device: its shard threads share the device's two slots"""
    script = tmp_path / "w.py"
    script.write_text(MULTI_WORKER % (ROOT, ROOT))
    env = dict(os.environ, MSPACK_HIP_FORCE_SHARDS="3")
    env.pop("MSPACK_HIP_SLOTS", None)
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0 and b"MULTI_SLOTS_OK" in p.stdout, p.stdout.decode()[-3000:]
