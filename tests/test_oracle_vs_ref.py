"""CPU, development container only (needs oracle/_ref built from /root/reference): the oracle and
our encoders against the REAL reference codecs on synthetic streams -- every block type, windows,
reset intervals, E8, truncation and bit flips (error codes and byte counts included)."""
import zlib

import numpy as np
import pytest

import libmspack_amd as M
from helpers import have_ref, oracle_lzx, oracle_mszip, oracle_qtm, oracle_qtm_marks, ref_lzx, ref_mszip, ref_qtm, ref_qtm_carry

pytestmark = pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built (reference sources absent)")

MODES = [dict(mode=1), dict(mode=2), dict(mode=3), dict(mode=4, block_size=20000),
         dict(mode=4, block_size=50001), dict(mode=0, block_size=9999), dict(repeats=0, lazy=0),
         dict(intel_filesize=250000)]


@pytest.mark.parametrize("kw", MODES)
def test_lzx_encoder_and_oracle_vs_reference(built, kw):
    data = M.gen_plaintext(7, M.TEXT_MIX, 150000)
    for wb, reset in [(21, 2), (16, 0), (17, 3), (15, 1)]:
        comp, _fo = M.lzx_encode(data, wb, reset, M.lzx_opts(**kw))
        s = comp.tobytes() + b"\0" * 8
        e1, o1, w1 = ref_lzx(s, data.size, wb, reset)
        e2, o2, r = oracle_lzx(s, data.size, wb, reset)
        assert e1 == e2 == 0 and o1 == o2 == data.tobytes() and w1 == r.out_len


def test_lzx_errors_match_reference(built):
    data = M.gen_plaintext(5, M.TEXT_MIX, 70000)
    comp = M.lzx_encode(data, 17, 0, M.lzx_opts(mode=4, block_size=12345))[0].tobytes()
    rng = np.random.default_rng(1)
    cases = [comp[:c] for c in (0, 1, 2, 3, 5, 17, 100, 1000, len(comp) // 2, len(comp) - 2, len(comp))]
    for _ in range(60):
        b = bytearray(comp); k = int(rng.integers(0, len(b))); b[k] ^= 1 << int(rng.integers(0, 8))
        cases.append(bytes(b))
    for s in cases:
        e1, o1, w1 = ref_lzx(s, data.size, 17, 0)
        e2, o2, r = oracle_lzx(s, data.size, 17, 0)
        assert (e1, w1) == (e2, r.out_len)
        if e1 == 0 and o1 == data.tobytes():
            assert o2 == o1


def test_qtm_encoder_and_oracle_vs_reference(built):
    for kind in range(6):
        for wb, n in [(21, 120000), (10, 40000), (15, 33000), (12, 2000)]:
            d = M.gen_plaintext(50 + kind, kind, n)
            s, _ = M.qtm_encode(d, wb)
            e1, o1, _w = ref_qtm(s, n, wb)
            e2, o2, _r = oracle_qtm(s, n, wb)
            assert e1 == e2 == 0 and o1 == o2 == d.tobytes()
    d = M.gen_plaintext(9, 0, 80000)
    s, _ = M.qtm_encode(d, 16)
    rng = np.random.default_rng(2)
    for _ in range(40):
        b = bytearray(s); k = int(rng.integers(0, len(b))); b[k] ^= 1 << int(rng.integers(0, 8))
        e1, o1, w1 = ref_qtm(bytes(b), d.size, 16)
        e2, o2, r = oracle_qtm(bytes(b), d.size, 16)
        assert (e1, w1) == (e2, r.out_len)


def test_qtm_what_a_request_holds_back_oracle_vs_reference(built):
    """qtmd decodes whole tokens: the match that covers a request's last byte usually runs past it, and the rest waits in the window
    for the NEXT call, which writes it before it decodes anything (qtmd.c:268-276).  The oracle reports that length (in_next) -- the
    ground truth of MSPACK_HIP_UF_QTM_MARKS -- and the real qtmd's o_end - o_ptr after the same request must agree: windows smaller
    and larger than a frame, requests that end at frame and window boundaries, and in damaged streams (both must fail alike)."""
    rng = np.random.default_rng(5)
    for kind, wb, n in [(0, 16, 90000), (2, 12, 40000), (4, 21, 70000), (1, 10, 9000)]:
        d = M.gen_plaintext(60 + kind, kind, n)
        s, _ = M.qtm_encode(d, wb)
        ps = sorted(set([1, 2, 32767, 32768, 32769, n - 1, n] + [int(x) for x in rng.integers(1, n, 40)] +
                        [(k << wb) + j for k in range(1, (n >> wb) + 1) for j in (-3, -2, -1, 0, 1)][:100]))
        seen = 0
        ps = [p for p in ps if p <= n]
        e, log = oracle_qtm_marks(s, n, wb, [p for p in ps if p < n])        # ONE decode, every boundary marked
        assert e == 0
        wraps = 0
        for i, p in enumerate(ps):
            e1, c1 = ref_qtm_carry(s, p, wb)
            e2, _o, r = oracle_qtm(s, p, wb)
            assert e1 == e2 and (e1 != 0 or c1 == r.in_next), (kind, wb, p, e1, c1, e2, r.in_next)
            # (an undamaged stream: the only requests that fail end inside a match that crosses the window's end, qtmd.c:366-374)
            assert p == n or log[i] == (c1 if e1 == 0 else 0xFFFFFFFF), (kind, wb, p, log[i], e1, c1)
            seen += e1 == 0 and c1 != 0
            wraps += e1 != 0
        assert wraps or wb >= 16, (kind, wb)
        assert seen > 5 or kind == 4, (kind, wb, seen)         # (requests do end inside matches; kind 4 has next to none)
        b = bytearray(s); b[len(b) // 2] ^= 0x20
        e, log = oracle_qtm_marks(bytes(b), n, wb, [p for p in ps if p < n])
        for i, p in enumerate(ps):
            e1, c1 = ref_qtm_carry(bytes(b), p, wb)
            e2, _o, r = oracle_qtm(bytes(b), p, wb)
            assert e1 == e2 and (e1 != 0 or c1 == r.in_next), (kind, wb, p, e1, c1, e2, r.in_next)
            assert p == n or log[i] in ((c1,) if e1 == 0 else (0, 0xFFFFFFFF)), (kind, wb, p, log[i], e1, c1)       # (never reached: 0)


def test_mszip_oracle_vs_reference(built):
    data = M.gen_plaintext(11, 0, 100000).tobytes()

    def folder(hist, lvl=6, strat=0, bs=32768):
        out, prev = [], None
        for k in range(0, len(data), bs):
            c = zlib.compressobj(lvl, zlib.DEFLATED, -15, 9, strat, prev) if (hist and prev) else \
                zlib.compressobj(lvl, zlib.DEFLATED, -15, 9, strat)
            out.append(b"CK" + c.compress(data[k:k + bs]) + c.flush())
            prev = data[max(0, k + bs - 32768):k + bs]
        return b"".join(out)
    rng = np.random.default_rng(3)
    # history across blocks is only well defined when every earlier block filled the window: with
    # short blocks a far distance lands in window bytes the reference never initialised
    cases = [folder(h, lv, st, bs) for h in (0, 1) for lv, st in ((0, 0), (6, 0), (6, zlib.Z_FIXED))
             for bs in (32768, 10000) if not (h and bs != 32768)]
    s = cases[3]
    cases += [s[:c] for c in (0, 1, 2, 3, 10, 100, len(s) // 2, len(s) - 1)]
    for _ in range(40):
        b = bytearray(s); k = int(rng.integers(0, len(b))); b[k] ^= 1 << int(rng.integers(0, 8))
        cases.append(bytes(b))
    for c in cases:
        for want in (len(data), 40000):
            e1, o1, w1 = ref_mszip(c, want)
            e2, o2, r, _ = oracle_mszip(c, want)
            assert (e1, w1) == (e2, r.out_len)
            # a corrupted stream may copy from window bytes the reference never initialised (its
            # window is malloc'ed): contents are only comparable when the result is the plaintext
            if e1 == 0 and o1 == data[:want]:
                assert o1 == o2


def _mutations():
    from test_gpu_fuzz import mutations
    return mutations


def test_fuzz_oracle_vs_reference_lzx(built):
    """The damaged-stream corpus of tests/test_gpu_fuzz.py (same generator, same seeds): the oracle's error
    code and byte count against the REAL reference -- this is what makes the GPU-vs-oracle fuzz a
    GPU-vs-reference statement."""
    mutations = _mutations()
    rng = np.random.default_rng(20240926)
    cfgs = [(17, 0, dict(mode=4, block_size=12345)), (21, 2, dict()), (16, 1, dict(mode=2)),
            (18, 0, dict(mode=1)), (15, 0, dict(mode=3)), (21, 2, dict(intel_filesize=200000)),
            (19, 4, dict(mode=4, block_size=40001, intel_filesize=5000, e8_base=1000))]
    n_bad = 0
    for ci, (wb, rf, kw) in enumerate(cfgs):
        n = 90000 if rf == 0 else 32768 * max(rf, 1) * 2
        data = M.gen_plaintext(100 + ci, ci % 6, n)
        comp = M.lzx_encode(data, wb, rf, M.lzx_opts(**kw))[0].tobytes()
        if kw.get("e8_base"):
            continue                                   # the memory-to-memory reference driver starts E8 at 0
        for m in [comp] + mutations(comp, rng, 350):
            s = m + b"\0" * 4 if rf else m
            e1, o1, w1 = ref_lzx(s, n, wb, rf)
            e2, o2, r = oracle_lzx(s, n, wb, rf)
            assert (e1, w1) == (e2, r.out_len), (ci, len(s), e1, w1, e2, r.out_len)
            n_bad += e1 != 0
            if e1 == 0 and o1 == data.tobytes():
                assert o2 == o1
    assert n_bad > 300


def test_sweep_oracle_vs_reference_lzx(built):
    """The random-configuration sweep of tests/test_gpu_fuzz.py (same generator, same seeds), oracle against
    the REAL reference: error code, byte count and -- for streams that decode to the plaintext prefix --
    bytes.  (A request shorter than the stream: the reference driver here sets output_length = the request.)"""
    from test_gpu_fuzz import lzx_sweep, SWEEP_SEEDS
    from helpers import ref
    n = 0
    ref().refh_zero_alloc(1)        # a damaged stream may read window bytes nobody wrote: zeros on both sides
    try:
        for seed in SWEEP_SEEDS:
            streams, params = lzx_sweep(seed)
            for st, p in zip(streams, params):
                e1, o1, w1 = ref_lzx(st, p[0], p[1], p[2])
                e2, o2, r = oracle_lzx(st, p[0], p[1], p[2], length=p[0])
                assert (e1, w1) == (e2, r.out_len), (seed, p, e1, w1, e2, r.out_len)
                if e1 == 0:
                    assert o1 == o2
                n += 1
    finally:
        ref().refh_zero_alloc(0)
    assert n > 1000


def test_fuzz_oracle_vs_reference_mszip_qtm(built):
    mutations = _mutations()
    from test_gpu_mszip import folder as zip_folder
    rng = np.random.default_rng(777)
    for ci, (level, strat, hist, bs) in enumerate([(6, zlib.Z_DEFAULT_STRATEGY, False, 32768), (9, zlib.Z_DEFAULT_STRATEGY, True, 32768),
                                                   (1, zlib.Z_FIXED, True, 32768), (6, zlib.Z_HUFFMAN_ONLY, False, 32768),
                                                   (6, zlib.Z_DEFAULT_STRATEGY, True, 20000), (0, zlib.Z_DEFAULT_STRATEGY, False, 32768),
                                                   (6, zlib.Z_RLE, True, 32768)]):
        data = M.gen_plaintext(300 + ci, ci % 6, 98304 if bs == 32768 else 80000).tobytes()
        s = zip_folder(data, level, strat, history=hist, bs=bs)
        for m in [s] + mutations(s, rng, 350):
            e1, o1, w1 = ref_mszip(m, len(data))
            e2, o2, r, _ = oracle_mszip(m, len(data))
            assert (e1, w1) == (e2, r.out_len), ("mszip", ci, e1, w1, e2, r.out_len)
    rng = np.random.default_rng(4242)
    for ci, wb in enumerate([16, 21, 10, 13]):
        data = M.gen_plaintext(500 + ci, ci % 6, 100000)
        s, _ = M.qtm_encode(data, wb)
        for m in [s] + mutations(s, rng, 150):
            e1, o1, w1 = ref_qtm(m, data.size, wb)
            e2, o2, r = oracle_qtm(m, data.size, wb)
            assert (e1, w1) == (e2, r.out_len), ("qtm", ci, e1, w1, e2, r.out_len)


def test_fuzz_oracle_vs_reference_mszip_repair(built):
    """Repair mode, several feeder chunk sizes: error, length AND contents against the real reference (its
    allocator zeroed for this test, so that window bytes it never wrote read as the oracle's zeros)."""
    from test_gpu_fuzz import repair_corpus
    from helpers import ref
    streams, lens, chunks = repair_corpus()
    ref().refh_zero_alloc(1)
    try:
        repaired = 0
        for m, n, c in zip(streams, lens, chunks):
            rp = c if c else 1
            e1, o1, w1 = ref_mszip(m, n, rp)
            e2, o2, r, _ = oracle_mszip(m, n, rp)
            assert (e1, w1) == (e2, r.out_len) and o1 == o2, (len(m), rp, e1, w1, e2, r.out_len)
            repaired += e1 == 0 and ref_mszip(m, n, 0)[0] != 0
        assert repaired > len(streams) // 8
    finally:
        ref().refh_zero_alloc(0)


DELTA_CASES = [(70000, 17, 0, {}), (200000, 18, 0, dict(mode=4, block_size=20000)), (100000, 19, 50000, {}),
               (300000, 21, 100000, dict(mode=2)), (5000, 17, 3000, dict(mode=3)),
               (65536, 17, 65536, dict(mode=4, block_size=9999)), (1 << 20, 22, 1 << 20, {}), (100000, 25, 0, {})]


def delta_case(n, wb, refn, kw):
    """plaintext sharing content with its reference data, with a long run (extended match lengths)"""
    data = M.gen_plaintext(7 + n, 0, n).copy()
    ref = b""
    if refn:
        r = M.gen_plaintext(99, 0, refn)
        k = min(n, refn) // 2
        data[1000:1000 + k // 2] = r[500:500 + k // 2]
        ref = r.tobytes()
    data[n // 3:n // 3 + 5000] = 0x41
    return data, ref, M.lzxd_encode(data, wb, ref, **kw).tobytes()


def far_offset_case():
    """10.4 MB whose tail repeats parts of its first megabyte: match offsets of about 9.5 MB (> 2^23)"""
    a = M.gen_plaintext(77, 0, 9_500_000)
    data = np.concatenate([a, a[:600_000], a[100_000:400_000]])
    return data, M.lzxd_encode(data, 25).tobytes()


def test_lzx_delta_far_offsets(built):
    from helpers import ref_lzxd, oracle_lzxd
    data, comp = far_offset_case()
    assert len(comp) < 0.36 * data.size          # the far copies were found (the tail costs next to nothing)
    e1, o1, w1 = ref_lzxd(comp + b"\0" * 8, data.size, 25)
    e2, o2, r = oracle_lzxd(comp + b"\0" * 8, data.size, 25)
    assert e1 == e2 == 0 and w1 == r.out_len == data.size and o1 == o2 == data.tobytes()


@pytest.mark.parametrize("case", DELTA_CASES, ids=[str(c[:3]) for c in DELTA_CASES])
def test_lzx_delta_encoder_and_oracle_vs_reference(built, case):
    """LZX DELTA: our encoder's streams through the real lzxd (is_delta, reference data)
    and through the oracle; plus damaged copies for error codes and byte counts."""
    from helpers import ref_lzxd, oracle_lzxd
    n, wb, refn, kw = case
    data, ref, comp = delta_case(n, wb, refn, kw)
    e1, o1, w1 = ref_lzxd(comp + b"\0" * 8, n, wb, ref)
    e2, o2, r = oracle_lzxd(comp + b"\0" * 8, n, wb, ref)
    assert e1 == e2 == 0 and o1 == o2 == data.tobytes() and w1 == r.out_len
    if n > 400000:
        return
    mutations = _mutations()
    rng = np.random.default_rng(n + wb)
    for m in mutations(comp, rng, 120):
        e1, o1, w1 = ref_lzxd(m, n, wb, ref)
        e2, o2, r = oracle_lzxd(m, n, wb, ref)
        assert (e1, w1) == (e2, r.out_len), (len(m), e1, w1, e2, r.out_len)


def test_szdd_kwaj_corpus_and_oracle_vs_reference(built):
    """SZDD / KWAJ: every file of the test recipe decodes through the REAL szddd / kwajd to its
    plaintext, and the LZSS / KWAJ-LZH oracles agree with the reference on the payloads and on damaged ones."""
    import struct
    from helpers import ref_szdd_kwaj, oracle_lzss, oracle_kwaj_lzh
    from test_szdd_kwaj import file_cases, damaged_files
    for name, kind, blob, want in file_cases():
        r = ref_szdd_kwaj(kind, blob)
        assert r["open_err"] == 0 and r["err"] == 0 and r["data"] == want, name
        variants = [blob] + damaged_files(name, kind, blob, 25)
        for v in variants:
            r = ref_szdd_kwaj(kind, v)
            if r["open_err"]:
                continue
            if kind == 0:
                off, mode = (14, 0) if r["comp_type"] == 0 else (12, 2)
                e, o, _ = oracle_lzss(v[off:], mode)
            elif r["comp_type"] == 2:
                e, o, _ = oracle_lzss(v[struct.unpack_from("<H", v, 10)[0]:], 2)
            elif r["comp_type"] == 3:
                e, o, _ = oracle_kwaj_lzh(v[struct.unpack_from("<H", v, 10)[0]:])
            else:
                continue
            assert (e, o) == (r["err"], r["data"]), (name, len(v))


def test_lzx_open_block_at_reset_warning_vs_reference(built):
    """lzxd.c:423-431: a block still open at a reset point makes the reference say "WARNING; invalid reset interval detected
    during LZX decompression" (once per lzxd_decompress call) and decode on.  The oracle's list of such reset points
    (oracle_lzx_open_resets -- what the kernels' MSPACK_HIP_UF_LZX_LOG is tested against) must be non-empty exactly when the
    reference warns, and both must produce the same bytes and error code."""
    import libmspack_amd as M
    from helpers import lzx_set_bits, oracle_lzx_open_resets, ref_messages
    F = 32768
    for seed, wb, rf, nfr, patches in ((1, 16, 1, 6, {1: 100, 3: 7}), (2, 17, 2, 8, {3: 50}), (3, 16, 2, 6, {}), (4, 16, 3, 9, {2: 11, 8: 5})):
        d = M.gen_plaintext(4000 + seed, seed & 1, nfr * F)
        lz, fo = M.lzx_encode(d, wb, rf)
        lz = bytearray(lz.tobytes())
        for fr, extra in patches.items():
            lzx_set_bits(lz, int(fo[fr]), 4 if fr % rf == 0 else 3, 24, F + extra)
        ref_messages()
        re_, rb, _ = ref_lzx(bytes(lz), nfr * F, wb, rf)
        said = [l for l in ref_messages() if "invalid reset interval" in l]
        oe, ob, _r = oracle_lzx(bytes(lz), nfr * F, wb, rf)
        cnt, frames = oracle_lzx_open_resets()
        assert (oe, ob) == (re_, rb), seed
        assert (cnt > 0) == (len(said) > 0) and len(said) <= 1, (seed, cnt, said)
        assert frames == sorted((fr // rf + 1) * rf for fr in patches), (seed, frames)


def _history_cases():
    import crafted_streams as CS
    return CS.mszip_history_cases(), CS.kwaj_mszip_cases()


def test_mszip_history_cases_oracle_vs_reference(built):
    """the deep-history streams (CAB framing) through the real mszipd: error, bytes written, every byte.  The two streams that
    read window bytes no frame wrote are left out: the reference reads uninitialised memory there."""
    import crafted_streams as CS
    left_out = 0
    for c in _history_cases()[0]:
        if c.props["never"]:
            left_out += 1
            continue
        repair = (c.props["in_chunk"] or 1) if c.props["uflags"] & CS.UF_MSZIP_REPAIR else 0
        e1, o1, w1 = ref_mszip(c.stream, c.out_len, repair)
        e2, o2, r, _ = oracle_mszip(c.stream, c.out_len, repair)
        assert (e1, w1) == (e2, r.out_len) and o1 == o2 == c.plain, (c.name, e1, w1, e2, r.out_len)
    assert left_out == 2


def test_mszip_kwaj_oracle_vs_reference(built):
    """oracle_mszip_kwaj_decode against the real kwajd (method 4) on every KWAJ case: error code and every byte written -- a
    failing stream has written the frames before the failure.  The real driver has neither a failing feeder nor a room: the
    cases that differ only in those are the same file, compared once with ample room."""
    from helpers import oracle_mszip_kwaj, ref_szdd_kwaj
    import crafted_streams as CS
    seen, left_out = set(), 0
    for c in _history_cases()[1]:
        if c.props["never"]:
            left_out += 1
            continue
        if c.stream in seen:
            continue
        seen.add(c.stream)
        total = sum(c.props["blocks"])
        g = ref_szdd_kwaj(1, CS.kwaj_container(c.stream, 4, total))
        e, o, r = oracle_mszip_kwaj(c.stream, total + 65536)
        assert g["open_err"] == 0 and g["comp_type"] == 4, c.name
        assert (g["err"], len(g["data"])) == (e, r.out_len) and g["data"] == o, (c.name, g["err"], e, len(g["data"]), r.out_len)
        if not (c.props["uflags"] & CS.UF_HARD_EOF) and c.out_len >= total + 32768:
            assert e == c.err and o == c.plain, c.name
    assert left_out == 2 and len(seen) >= 25
