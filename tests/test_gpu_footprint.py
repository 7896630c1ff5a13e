"""Write footprint and placement parity of the LZX, LZX DELTA, MSZIP and Quantum kernels (tests/footprint.py has the layout and the
checker).  Every batch goes through mspack_hip_decode_batch_to_device into a device buffer full of 0xA5 in which every unit lies
between 1024 guard bytes, at byte residues of in_off and out_off that no other test uses, with 0xFF -- or the rest of the real stream --
behind in_len.  Checked: the result words against the oracle, and the WHOLE image: the oracle's bytes where the unit decoded, the
reference data as placed, the fill everywhere else; only what the header calls unspecified (the rest of a unit's own region) is masked.
Groups: lengths and residues of LZX units of every block type, E8 at a unit's last bytes (fill 0xE8 too), CHM-style intervals whose
in_len reaches to the end of the stream (and the reset log), LZX DELTA with reference data of every length below the output, MSZIP
folders with their slack, Quantum with and without marks, in_len ending the stream early for all four codecs, the hand-built cases
of tests/crafted_streams.py, and one mixed batch through the device-resident entry.  tests/test_gpu_fold.py runs this file with the
fold tasks forced on and off, tests/test_emu_kernels.py the small groups on the wavefront emulator.

Wall times of the test bodies on an MI355X (oracle included): crafted[qtm] 5.7 s, crafted[lzx] 2.5 s, crafted[lzxd] 0.9 s, delta 0.9 s,
crafted[mszip] 0.4 s, lengths[tiny] 0.3 s, device entry 0.2 s, mszip 0.15 s, every other one under 0.1 s; the module 12 s.

FOUND BY IT AND FIXED: an LZX unit with a frame table whose out_off is no multiple of 16 came out with single wrong literals (err,
out_len and flags right, frames adopted) -- 8 of the 65536 bytes of gen_plaintext(71, TEXT_MIX)[262144:327680] at residues 1 to 14, 46
bytes in test_lzx_intervals_the_chm_way, 3 in the unit "lzx reset log 1, table".  lzx_parse_emit's literal ring leaves LDS as 16-byte rows;
its first row began at edge_n = the distance to the next 128-byte line of the ADDRESS, which is a multiple of 16 frame positions only
when out_off is one: the row that began at ring index 1009 to 1023 read past the ring's end instead of wrapping, and the literals of
frame positions 1024 to 1038 were lost.  edge_n is now rounded up to 16 positions (lzx_pipe_parse.hpp).  No byte outside a unit's
region, no changed reference byte and no dependence on what lies behind in_len was seen in any group."""
import zlib

import numpy as np
import pytest

import crafted_streams as CS
import footprint as F
import libmspack_amd as M
import szdd_kwaj_recipe as R
import test_gpu_lzx_log as LG
from test_gpu_hostpath import DevBuf
from test_gpu_md5 import dev_write
from test_gpu_mszip_blocks import folder_blocks

pytestmark = pytest.mark.gpu
FILL = 0xA5
FRAME = 32768
KIND = {"lzx": M.KIND_LZX, "lzxd": M.KIND_LZX_DELTA, "mszip": M.KIND_MSZIP, "qtm": M.KIND_QUANTUM}


# ---- running a layout ---------------------------------------------------------------------------------------------------------------
def place_refs(buf, base, L):
    for it, (_lo, ref0, _out, _end, _hi) in zip(L.items, L.span):
        dev_write(buf, base + ref0, np.frombuffer(it.ref, dtype=np.uint8))


def run_to_device(L, fill=FILL):
    """the layout through mspack_hip_decode_batch_to_device into a device buffer full of `fill` -> (the whole image, results)"""
    d = DevBuf(L.out_bytes, fill)
    place_refs(d, 0, L)
    res = np.zeros(len(L.units), dtype=M.RESULT_DTYPE)
    u = np.ascontiguousarray(L.units)
    rc = M.lib().mspack_hip_decode_batch_to_device(u.ctypes.data, len(u), L.arena.ctypes.data, L.arena.size, d.ptr, L.out_bytes, res.ctypes.data)
    assert rc == 0, M.lib().mspack_hip_last_error()
    image = d.to_host()
    d.free()
    return image, res


def run_device(L, fill=FILL):
    """the layout through mspack_hip_decode_batch_device: the output arena is exactly out_bytes long inside a larger allocation of
    `fill` whose other bytes are checked (tests/test_gpu_sha.py run_device_raw) -> (the image, results)"""
    lib, g = M.lib(), 4096
    u = np.ascontiguousarray(L.units)
    big = DevBuf(L.out_bytes + 2 * g, fill)
    place_refs(big, g, L)
    d_units, d_in = DevBuf(u.nbytes), DevBuf(L.arena.size + 64, 0xFF)
    d_res = DevBuf(len(u) * M.RESULT_DTYPE.itemsize, 0x77)
    scratch = DevBuf(max(int(lib.mspack_hip_frame_scratch_bytes(L.n_frames)), 16))
    dev_write(d_units, 0, u.view(np.uint8))
    dev_write(d_in, 0, L.arena)
    mask = M.MASK_CRC32 | 0x80000000                 # MSPACK_HIP_MASK_FRAME_TABLES
    for k in set(int(k) for k in u["kind"]):
        mask |= 1 << k
    rc = lib.mspack_hip_decode_batch_device(d_units.ptr, None, len(u), d_in.ptr, L.arena.size, big.ptr + g, L.out_bytes, d_res.ptr,
                                            scratch.ptr, L.n_frames, mask, None)
    assert rc == 0, lib.mspack_hip_last_error()
    if big.emu is None:
        assert big.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(u) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE).copy()
    after = big.to_host()
    for b in (big, d_units, d_in, d_res, scratch):
        b.free()
    assert (after[:g] == fill).all() and (after[g + L.out_bytes:] == fill).all(), "a byte outside the output arena changed"
    return after[g:g + L.out_bytes], res


def check(items, fill=FILL, run=run_to_device):
    """(a) the results and (b) the whole image of the batch against the oracle"""
    L = F.layout(items)
    assert L.out_bytes < 64 << 20, L.out_bytes
    wants = [F.oracle(it) for it in items]
    exp, mask = F.expected_image(L, wants, fill)
    image, res = run(L, fill)
    F.check_results(L, res, wants)
    F.compare(image, exp, mask, L)
    return L, wants, image, res


# ---- texts and streams ---------------------------------------------------------------------------------------------------------------
def de_bruijn_256_2():
    """65536 bytes in which no pair of bytes occurs twice (the FKM construction of B(256, 2)): an LZ77 encoder finds no match in any
    65537 bytes of its repetition -- a literal-only text"""
    a, seq = [0] * 4, []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]; db(t + 1, p)
            for j in range(a[t - p] + 1, 256):
                a[t] = j; db(t + 1, t)
    db(1, 1)
    assert len(seq) == 65536
    return np.array(seq, dtype=np.uint8)


_TEXTS = {}


def text(which, n):
    """'mix'; 'literal' (no match anywhere); 'fills': repetitive text whose second half is ONE periodic run that ends on the last byte"""
    if not _TEXTS:
        _TEXTS["mix"] = M.gen_plaintext(61, M.TEXT_MIX, 3 * FRAME)
        _TEXTS["literal"] = np.tile(de_bruijn_256_2(), 2)
        _TEXTS["fills"] = M.gen_plaintext(62, M.TEXT_REPETITIVE, 3 * FRAME)
    d = _TEXTS[which][:n].copy()
    if which == "fills":
        d[n - n // 2:] = np.frombuffer((b"abcdefg" * (n // 14 + 1))[:n // 2], dtype=np.uint8)
    return d


def with_and_without_table(name, kind, stream, out_len, tab, **kw):
    return [F.Item(name + ", table", kind, stream, out_len, tab=list(int(x) for x in tab), **kw),
            F.Item(name + ", no table", kind, stream, out_len, **kw)]


def residues(k):
    """the k-th unit's (in_off mod 16, out_off mod 128)"""
    return dict(ri=(5 * k + 3) % 16, ro=F.RESIDUES[k % len(F.RESIDUES)])


# ---- lzx_lengths_and_residues --------------------------------------------------------------------------------------------------------
LENGTHS = {"tiny": [1, 15, 16, 17, 63, 64, 65, 127, 129], "frame": [32767, 32768, 32769], "frames": [65537, 3 * 32768 - 1]}


def lzx_length_items(lengths):
    """every length at every residue of out_off (22 of them); block type, window and text rotate over the pairs so that every length
    meets each of the 18 combinations and every residue several; each with and without its frame table"""
    items, j = [], 0
    for n in lengths:
        for r, ro in enumerate(F.RESIDUES):
            mode, wb, which = (1, 2, 3)[j % 3], (15, 21)[(j // 3) % 2], ("mix", "literal", "fills")[(j // 6) % 3]
            j += 1
            d = text(which, n)
            comp, fo = M.lzx_encode(d, wb, 0, M.lzx_opts(mode=mode))
            name = "lzx %s w%d %s, %d bytes" % (("verbatim", "aligned", "uncompressed")[mode - 1], wb, which, n)
            for it in with_and_without_table(name, M.KIND_LZX, comp.tobytes(), n, fo[:-1], wb=wb, plain=d.tobytes(),
                                             ri=(5 * (j + r) + 3) % 16, ro=ro):
                items.append(it)
        j += 1                     # (22 residues and 18 combinations share a factor: shift the rotation from length to length)
    return items


@pytest.mark.parametrize("lengths", list(LENGTHS))
def test_lzx_lengths_and_residues(built, lengths):
    items = lzx_length_items(LENGTHS[lengths])
    assert set(it.ro for it in items) == set(F.RESIDUES) and len(set(it.ri for it in items)) == 16
    L, wants, _image, _res = check(items)
    assert all(w.err == 0 and w.data == it.plain for it, w in zip(items, wants))         # (the encoder's streams are what they should be)


# ---- lzx_e8_at_the_edge --------------------------------------------------------------------------------------------------------------
def e8_items():
    """intel_filesize set, 0xE8 at out_len - 11 (the last position the translation looks at), - 10 and - 1; last frames of 10 bytes (not
    translated at all, lzxd.c:699-703), 11 and 12, and a full one"""
    items, k = [], 0
    for n in (10, 11, 12, 40, FRAME, FRAME + 10, FRAME + 11, FRAME + 12, 2 * FRAME):
        for wb, mode in ((16, 1), (21, 2), (17, 3)):
            d = text("mix", n)
            for p in (n - 11, n - 10, n - 1):
                if p >= 0:
                    d[p] = 0xE8
                    d[p + 1:min(p + 5, n)] = np.array([0x10, 0x20, 0x00, 0x00], dtype=np.uint8)[:min(p + 5, n) - p - 1]
            comp, fo = M.lzx_encode(d, wb, 0, M.lzx_opts(mode=mode, intel_filesize=250000))
            items += with_and_without_table("lzx E8 w%d mode %d, %d bytes" % (wb, mode, n), M.KIND_LZX, comp.tobytes(), n, fo[:-1], wb=wb,
                                            plain=d.tobytes(), **residues(k))
            k += 1
    return items


@pytest.mark.parametrize("fill", [0xA5, 0xE8], ids=["fill_A5", "fill_E8"])
def test_lzx_e8_at_the_edge(built, fill):
    """with 0xE8 as the fill a translation pass that looks past the unit finds a CALL in the guard and rewrites it"""
    items = e8_items()
    L, wants, _image, _res = check(items, fill)
    assert any(w.flags & M.F_E8_APPLIED for w in wants)
    assert all(w.err == 0 and w.data == it.plain for it, w in zip(items, wants))


# ---- lzx_intervals_the_chm_way -------------------------------------------------------------------------------------------------------
def chm_items():
    """ONE copy of each stream in the arena; every reset interval is a unit whose in_off is the reset-table entry (any even residue)
    and whose in_len reaches to the end of the WHOLE stream, as chmd.c interval_units builds them: the look-ahead frame of
    lzxd.c:419 is decodable and its bytes are the next unit's.  And a copy with one flipped bit in interval 3."""
    items = []
    for s, (wb, reset, n) in enumerate([(16, 1, 6 * FRAME + 5000), (21, 2, 5 * 2 * FRAME + 40000), (17, 2, 4 * 2 * FRAME + 9), (21, 1, 4 * FRAME)]):
        d = M.gen_plaintext(70 + s, M.TEXT_MIX, n)
        comp, fo = M.lzx_encode(d, wb, reset)
        fo = fo.astype(np.int64)
        ib = reset * FRAME
        bad = bytearray(comp.tobytes())
        bad[int(fo[3 * reset]) + 200] ^= 0x10
        for what, c in (("", comp.tobytes()), (" damaged", bytes(bad))):
            for k in range(0, n, ib):
                f0, f1 = k // FRAME, min((k + ib + FRAME - 1) // FRAME, len(fo) - 1)
                m = min(ib, n - k)
                items += with_and_without_table("lzx interval %d of stream %d%s (w%d, reset %d)" % (k // ib, s, what, wb, reset), M.KIND_LZX, c, m,
                                                fo[f0:f1] - fo[f0], wb=wb, reset=reset, e8_base=k, skip=int(fo[f0]), plain=d[k:k + m].tobytes(),
                                                share=("chm", s, what), ri=(5 * s + (7 if what else 0)) % 16, ro=F.RESIDUES[(len(items) // 2) % 22])
    return items


def log_items():
    """serial-span units as chmd.c builds them (MSPACK_HIP_UF_LZX_LOG, in_len to the stream's end): the streams of
    tests/test_gpu_lzx_log.py, whose blocks outlive their frames"""
    items = []
    for s, (lz, fo, wb, rf, nfr, _exp) in enumerate(LG.streams()):
        kw = dict(wb=wb, reset=rf, flags=F.UF_LZX_LOG, log_cap=4, ri=(3 * s + 1) % 16, ro=F.RESIDUES[(7 * s + 5) % 22])
        items.append(F.Item("lzx reset log %d" % s, M.KIND_LZX, lz, nfr * FRAME, **kw))
        items.append(F.Item("lzx reset log %d, table" % s, M.KIND_LZX, lz, nfr * FRAME, tab=[int(x) for x in fo[:nfr]], **kw))
    return items


def test_lzx_intervals_the_chm_way(built):
    items = chm_items()
    L, wants, _image, res = check(items)
    good = [w for it, w in zip(items, wants) if "damaged" not in it.name]
    assert all(w.data == it.plain for it, w in zip(items, wants) if "damaged" not in it.name)
    # (stream 3 ends on a reset point: the look-ahead behind its last interval runs out of input, with and without table)
    assert sum(1 for w in good if w.flags & M.F_LOOKAHEAD_READ) >= 2
    assert all(w.in_next for w in good) and any(w.err for w in wants if w.err != M.ERR_READ)
    assert len(set(int(x) % 16 for x in L.units["in_off"])) >= 6


def test_lzx_reset_log_in_guarded_layout(built):
    items = log_items()
    L, wants, _image, _res = check(items)
    assert any(w.log[0] for w in wants) and all(w.out_len == it.out_len for it, w in zip(items, wants))


# ---- lzx_delta_reference_is_read_only ------------------------------------------------------------------------------------------------
_DELTA = {}


def delta_stream(wb, n, ref):
    """a hand-built DELTA stream (tests/crafted_streams.py Lzx): literals, a match that starts at the FIRST reference byte right at the
    beginning and one that ends on the unit's last byte -> (stream, plaintext)"""
    key = (wb, n, len(ref))
    if key not in _DELTA:
        z = CS.Lzx(wb, n, delta=True, ref=ref)
        z.block(1, n, main=CS.flat_main(wb), lens=CS.TWO_LEN)
        t = CS._text(80 + len(ref), n)
        if n >= 17:
            z.lit(t[:2])
            if len(ref) + z.pos >= 3:
                z.match(9, offset=len(ref) + z.pos)
            last = 4 if n % FRAME >= 4 else n % FRAME          # (no match crosses a frame's end)
            z.lit(t[z.pos:n - last])
            z.match(last, offset=len(ref) + z.pos) if last >= 2 else z.lit(t[z.pos:n])
        else:
            z.lit(t)
        assert z.pos == n and not z.fail
        _DELTA[key] = (z.stream(pad=0), z.plain())
    return _DELTA[key]


def delta_items():
    items, k = [], 0
    for ref_len in (0, 1, 15, 16, 17, 4099):
        ref = CS._rnd(300 + ref_len, ref_len)
        for wb in (17, 25):
            for r, ro in enumerate(F.RESIDUES):
                n = (1, 17, 1000, FRAME + 5)[(k + r) % 4]
                s, plain = delta_stream(wb, n, ref)
                items.append(F.Item("lzx delta w%d, ref_len %d, %d bytes" % (wb, ref_len, n), M.KIND_LZX_DELTA, s, n, wb=wb, ref=ref, plain=plain,
                                    ri=(5 * len(items) + 3) % 16, ro=ro, flags=M.UF_CRC32 if len(items) % 3 == 0 else 0))
            k += 1
    return items


def test_lzx_delta_reference_is_read_only(built):
    items = delta_items()
    L, wants, _image, _res = check(items)
    assert all(w.err == 0 and w.data == it.plain for it, w in zip(items, wants))
    assert len(set((int(u["out_off"]) - int(u["ref_len"])) % 16 for u in L.units)) == 16          # (reference data starts at any residue)


# ---- mszip_blocks_and_slack ----------------------------------------------------------------------------------------------------------
def mszip_items():
    items, k = [], 0
    src = M.gen_plaintext(90, M.TEXT_MIX, 5 * FRAME).tobytes()
    for nb in range(1, 6):
        for last in (1, 17, 32767):
            for what, kw in (("stored", dict(level=0)), ("fixed", dict(strategy=zlib.Z_FIXED)), ("dynamic", {})):
                d = src[:(nb - 1) * FRAME + last]
                s, offs = folder_blocks(d, **kw)
                items += with_and_without_table("mszip %d %s blocks, the last of %d" % (nb, what, last), M.KIND_MSZIP, s, len(d), offs, plain=d,
                                                **residues(k))
                k += 1
    # a request that ends inside the last block: the rest of it lies in the slack (result.in_next), nothing behind the slack
    d = src[:2 * FRAME + 20000]
    s, offs = folder_blocks(d)
    for ask in (len(d) - 1, len(d) - 19999, FRAME + 5, 1):
        items += with_and_without_table("mszip request of %d that ends inside a block" % ask, M.KIND_MSZIP, s, ask, offs[:(ask + FRAME - 1) // FRAME],
                                        plain=d, **residues(k))
        k += 1
    # repair mode with its log, one bad block
    d = src[:4 * FRAME]
    s, offs = folder_blocks(d)
    b = bytearray(s); b[offs[1] + 40] ^= 0x20
    items.append(F.Item("mszip repair with log, block 1 bad", M.KIND_MSZIP, bytes(b), len(d), flags=M.UF_MSZIP_REPAIR | F.UF_MSZIP_LOG, log_cap=4,
                        plain=d, **residues(k)))
    # KWAJ framing: the second block does not fit the room
    d = src[:FRAME + 1000]
    want = F.Want(0, 8, FRAME, 0, 0, d[:FRAME])                               # (8: MSPACK_HIP_F_OUT_FULL)
    items.append(F.Item("mszip KWAJ, room for one block of two", M.KIND_MSZIP, R.kwaj_mszip(d), FRAME + 100, flags=F.UF_MSZIP_KWAJ, plain=d, want=want,
                        **residues(k + 1)))
    return items


def test_mszip_blocks_and_slack(built):
    items = mszip_items()
    L, wants, _image, _res = check(items)
    assert sum(1 for w in wants if w.in_next) >= 6 and all(w.err == 0 for w in wants)
    assert all(w.data == it.plain[:w.out_len] for it, w in zip(items, wants) if not it.flags & M.UF_MSZIP_REPAIR)


# ---- qtm_windows_and_marks -----------------------------------------------------------------------------------------------------------
def qtm_items():
    """in_len exact, 0xFF behind it; with marks (every 97th position and around every window end) out_off % 4 == 0"""
    items = []
    src = M.gen_plaintext(95, M.TEXT_MIX, FRAME + 5)
    for wb in (10, 21):
        for n in (1, 1023, 1024, 1025, FRAME + 5):
            s = M.qtm_encode(src[:n], wb)[0]
            marks = sorted(set(range(97, n, 97)) | set((k << wb) + j for k in range(1, (n >> wb) + 1) for j in range(-4, 2) if 0 < (k << wb) + j < n))
            for ro in F.RESIDUES:
                items.append(F.Item("qtm w%d, %d bytes" % (wb, n), M.KIND_QUANTUM, s, n, wb=wb, plain=src[:n].tobytes(), ri=(5 * len(items) + 3) % 16, ro=ro))
            for ro in (0, 4, 8, 12, 36, 68, 124):
                items.append(F.Item("qtm w%d, %d bytes, %d marks" % (wb, n, len(marks)), M.KIND_QUANTUM, s, n, wb=wb, marks=marks, plain=src[:n].tobytes(),
                                    ri=(5 * len(items) + 3) % 16, ro=ro))
    return items


def test_qtm_windows_and_marks(built):
    items = qtm_items()
    L, wants, _image, _res = check(items)
    assert all(w.err == 0 and w.data == it.plain for it, w in zip(items, wants))
    assert sum(1 for w in wants if w.log and any(w.log)) > 20


# ---- in_len_ends_the_stream ----------------------------------------------------------------------------------------------------------
def cuts_of(n):
    return sorted(set([0, 1, 2, 3, 5, 17, 100, 1000, n // 2, n - 3, n - 2, n - 1, n]))


def truncation_items(codec):
    """the truncations of tests/test_gpu_lzx.py test_lzx_truncated_and_corrupt -- but the WHOLE stream lies in the arena and only in_len
    is shortened: a reader that runs past in_len finds real bits where the reference fabricates two zero bytes.  Each with and without
    a failing feeder (MSPACK_HIP_UF_HARD_EOF), LZX and MSZIP with and without their tables"""
    kw, tab = {}, None
    if codec == "lzx":
        d = M.gen_plaintext(5, M.TEXT_MIX, 70000)
        comp, fo = M.lzx_encode(d, 17, 0, M.lzx_opts(mode=4, block_size=12345))
        s, tab, kw = comp.tobytes(), fo[:-1], dict(wb=17)
    elif codec == "lzxd":
        d = M.gen_plaintext(6, M.TEXT_MIX, 40000)
        ref = M.gen_plaintext(6, M.TEXT_MIX, 3000).tobytes()
        s, kw = M.lzxd_encode(d, 17, ref).tobytes(), dict(wb=17, ref=ref)
    elif codec == "mszip":
        d = M.gen_plaintext(21, M.TEXT_MIX, 100000)
        s, tab = folder_blocks(d.tobytes())
    else:
        d = M.gen_plaintext(9, M.TEXT_MIX, 120000)
        s, kw = M.qtm_encode(d, 16)[0], dict(wb=16)
    items, k = [], 0
    for cut in cuts_of(len(s)):
        for hard in (0, F.UF_HARD_EOF):
            name = "%s with in_len %d of %d%s" % (codec, cut, len(s), ", failing feeder" if hard else "")
            a = dict(kw, in_len=cut, flags=hard, plain=d.tobytes(), **residues(k))
            k += 1
            if tab is not None:
                items += with_and_without_table(name, KIND[codec], s, d.size, tab, **a)
            else:
                items.append(F.Item(name, KIND[codec], s, d.size, **a))
    return items


@pytest.mark.parametrize("codec", list(KIND))
def test_in_len_ends_the_stream(built, codec):
    items = truncation_items(codec)
    L, wants, _image, _res = check(items)
    assert sum(1 for w in wants if w.err == M.ERR_READ) >= len(items) // 2
    assert all(w.trusted for w in wants)


# ---- crafted_cases_in_guarded_layout -------------------------------------------------------------------------------------------------
def crafted_items(codec):
    cases = {"lzx": CS.lzx_cases, "lzxd": CS.lzxd_cases, "mszip": CS.mszip_cases, "qtm": CS.qtm_cases}[codec]()
    items = []
    for c in cases:
        for ri, ro in ((0, 0), (1, 15), (9, 113)):
            kw = dict(wb=c.wb, reset=c.reset, ref=c.ref, plain=c.plain, ri=ri, ro=ro)
            if codec in ("lzx", "mszip"):
                items += with_and_without_table(c.name, KIND[codec], c.stream, c.out_len, c.tab, **kw)
            else:
                items.append(F.Item(c.name, KIND[codec], c.stream, c.out_len, **kw))
    return cases, items


@pytest.mark.parametrize("codec", list(KIND))
def test_crafted_cases_in_guarded_layout(built, codec):
    """every case of tests/crafted_streams.py, valid and failing, at three residue pairs"""
    cases, items = crafted_items(codec)
    per = len(items) // len(cases)
    half = (len(items) + 1) // 2 if codec in ("lzx", "mszip") else len(items)      # (two batches where one image would pass 64 MiB)
    wants = []
    for part in (items[:half], items[half:]):
        if part:
            wants += check(part)[1]
    for j, c in enumerate(cases):
        for w in wants[per * j:per * (j + 1)]:
            assert w.err == c.err, (c.name, w.err, c.err)
            assert c.plain is None or w.data == c.plain[:len(w.data)], c.name


# ---- device_resident_entry -----------------------------------------------------------------------------------------------------------
def mixed_items():
    """about 40 of the items above, every kind, tables, marks, a log, reference data, digests, a cut stream"""
    pick = lambda items, idx: [items[i] for i in idx if i < len(items)]
    items = pick(lzx_length_items([17, 32769]), range(0, 88, 11))
    items += pick(e8_items(), (8, 9, 34, 35, 52))
    items += pick(chm_items(), (0, 1, 6, 13)) + pick(log_items(), (2, 3))
    items += pick(delta_items(), (3, 70, 135, 200, 263))
    items += pick(mszip_items(), (0, 7, 40, 41, 90, 93, 98, 99))
    items += pick(qtm_items(), (0, 25, 57, 86, 116, 203, 289))
    items += pick(truncation_items("lzx"), (20, 21, 46)) + pick(truncation_items("qtm"), (13,))
    return items


def test_device_resident_entry(built):
    """the same image through mspack_hip_decode_batch_device as through mspack_hip_decode_batch_to_device, the arena exactly out_bytes
    long inside a larger allocation whose other bytes stay as they were"""
    items = mixed_items()
    assert 35 <= len(items) <= 50 and set(it.kind for it in items) == set(KIND.values())
    L, wants, image, res = check(items, run=run_device)
    image2, res2 = run_to_device(L)
    exp, mask = F.expected_image(L, wants, FILL)
    F.compare(image2, exp, mask, L)
    for f in ("err", "out_len", "good_len", "in_next"):
        assert np.array_equal(res[f], res2[f]), f
    assert np.array_equal(image[~mask], image2[~mask])


def test_mszip_deep_chains_stay_in_their_regions(built):
    """MSZIP units whose window history is deeper than the kernel's stack decode in a ring in their own slack
    (mszip_kernel.hpp): two such CAB-framed units (one of them with a request that ends inside its last block) and a
    KWAJ-framed one, back to back in a device buffer full of 0xA5 -- every unit's bytes are the oracle's, and outside
    [out_off, out_off + out_len + 32768) of each unit no byte has changed."""
    import test_gpu_mszip_history as H
    names = ("mszip_history_shrinking_chain_depth_12", "mszip_history_shrinking_chain_depth_40_request_ends_in_the_last_block",
             "kwaj_mszip_history_shrinking_chain_depth_12")
    items = [(next(c for c in H.cases() if c.name == n), False) for n in names]
    units, arena, out_bytes = H.batch(items)
    from test_gpu_crafted import to_device
    out, res = to_device(units, arena, out_bytes)
    H.check(items, units, out, res, "footprint")
    owned = np.zeros(out_bytes, dtype=bool)
    for i, (c, _t) in enumerate(items):
        oo = int(units["out_off"][i])
        owned[oo:oo + c.out_len + 32768] = True
    assert (out[~owned] == H.FILL).all(), "a byte outside the units' regions changed: %d" % int(np.flatnonzero((out != H.FILL) & ~owned)[0])
