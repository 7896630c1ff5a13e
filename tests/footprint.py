"""The write footprint of a batch: a layout in which every unit's region lies between guard bytes that belong to nobody, at any byte
residue of in_off and out_off, and the image the output arena must hold afterwards -- test_gpu_crafted.lz_batch / check_lz for every
decoding kind.  What include/mspack_hip.h promises and this pins down:
  * a unit owns [out_off, out_off + out_len) -- an MSZIP unit 32768 bytes of slack behind that, a flagged unit its log or table of
    marks where the header puts it -- and stores nowhere else;
  * an LZX DELTA unit reads its reference data at [out_off - ref_len, out_off) and never writes it;
  * in_len ends the input, whatever lies behind it (here: 0xFF, or the rest of the real stream);
  * no alignment of in_off or out_off (marks: out_off % 4 == 0).
Nothing here needs a GPU: tests/test_footprint_cpu.py shows that the checker can fail, tests/test_gpu_footprint.py runs the kernels."""
import zlib

import numpy as np

import helpers as H
import libmspack_amd as M

GUARD = 1024                       # bytes that belong to nobody in front of and behind every unit: the widest store group (64 lanes x 16 B)
ZIP_SLACK = 32768
UF_HARD_EOF, UF_MSZIP_KWAJ, UF_MSZIP_LOG, UF_LZX_LOG = 2, 4, 16, 32          # MSPACK_HIP_UF_* (include/mspack_hip.h)
ADOPTED = M.F_FRAMES_ADOPTED
NOBODY, REFERENCE, OUTPUT, SLACK, LOG = range(5)
CLASS_NAMES = ["a guard byte (nobody's)", "reference data", "output", "MSZIP slack", "log / marks"]
RESIDUES = list(range(16)) + [17, 31, 33, 63, 65, 127]        # out_off mod 128


class Item:
    """one unit to be: `stream` is what is placed in the input arena (once per `share` key; the unit reads from `skip` on, in_len
    bytes -- default: to the stream's end), `ri` / `ro` the residues of the placed stream mod 16 and of out_off mod 128.  tab: frame /
    block table (MSPACK_HIP_UF_FRAME_TABLE), marks: MSPACK_HIP_UF_QTM_MARKS, log_cap: entries of an LZX / MSZIP log; plain: the
    plaintext where known; want: the expected result where no oracle exists (see oracle())"""

    def __init__(self, name, kind, stream, out_len, wb=0, reset=0, e8_base=0, flags=0, ref=b"", ri=0, ro=0, in_len=None, skip=0,
                 tab=None, marks=None, log_cap=0, in_chunk=0, plain=None, share=None, want=None):
        self.name, self.kind, self.stream, self.out_len = name, kind, bytes(stream), int(out_len)
        self.wb, self.reset, self.e8_base, self.flags, self.ref = wb, reset, e8_base, flags, bytes(ref)
        self.ri, self.ro, self.skip = ri, ro, skip
        self.in_len = len(self.stream) - skip if in_len is None else in_len
        self.tab, self.marks, self.log_cap, self.in_chunk = tab, marks, log_cap, in_chunk
        self.plain, self.share, self.want = (None if plain is None else bytes(plain)), share, want
        if tab is not None:
            self.flags |= M.UF_FRAME_TABLE
        if marks is not None:
            self.flags |= M.UF_QTM_MARKS

    def data(self):
        """the bytes in_len leaves the unit"""
        return self.stream[self.skip:self.skip + self.in_len]

    def owned(self, out):
        """[(first, end, class)] of what the unit owns, from include/mspack_hip.h, for out_off = out"""
        n = self.out_len
        o = [(out, out + n, OUTPUT)]
        if self.kind == M.KIND_MSZIP:
            o.append((out + n, out + n + ZIP_SLACK, SLACK))
        if self.kind == M.KIND_MSZIP and self.flags & UF_MSZIP_LOG:
            lo = out + ((n + 32768 + 15) & ~15)
            o.append((lo, lo + 4 + 8 * self.log_cap, LOG))
        if self.kind == M.KIND_LZX and self.flags & UF_LZX_LOG:
            lo = out + ((n + 32768 + 15) & ~15)
            o.append((lo, lo + 4 + 4 * self.log_cap, LOG))
        if self.kind == M.KIND_QUANTUM and self.marks is not None:
            lo = out + ((n + 15) & ~15)
            o.append((lo, lo + 4 * len(self.marks), LOG))
        return o

    def log_at(self, out):
        return self.owned(out)[-1][0]


class Layout:
    pass


def layout(items):
    """-> Layout: units, arena (0xFF wherever no stream and no table lies, the final 64 bytes included), out_bytes, and per item
    span[i] = (first byte of its leading guard, first reference byte, out_off, end of what it owns, end of its trailing guard);
    cls / owner: per byte of the output image its class and the item it belongs to"""
    L = Layout()
    L.items = items
    n = len(items)
    # ---- input: every stream at its residue mod 16, at least 16 bytes of 0xFF behind it; tables 4-aligned ----
    at, tab_at, parts, pos = {}, [], [], 0
    in_off = []
    for i, it in enumerate(items):
        key = ("own", i) if it.share is None else it.share
        if key not in at:
            pos = ((pos + 31) & ~15) + it.ri
            at[key] = pos
            parts.append((pos, np.frombuffer(it.stream, dtype=np.uint8)))
            pos += len(it.stream)
        in_off.append(at[key] + it.skip)
        t = it.tab if it.tab is not None else it.marks
        if t is not None:
            pos = (pos + 8 + 3) & ~3
            tab_at.append(pos)
            parts.append((pos, np.asarray(t, dtype=np.uint32).view(np.uint8)))
            pos += 4 * len(t)
        else:
            tab_at.append(0)
    L.arena = np.full(pos + 64, 0xFF, dtype=np.uint8)
    for p, a in parts:
        L.arena[p:p + a.size] = a
    # ---- output: GUARD, the reference data (exactly ref_len bytes), the region, GUARD ----
    u = np.zeros(n, dtype=M.UNIT_DTYPE)
    L.span, pos = [], 0
    for i, it in enumerate(items):
        out = pos + GUARD + len(it.ref)
        out += (it.ro - out) % 128
        end = max(b for _a, b, _c in it.owned(out))
        L.span.append((pos, out - len(it.ref), out, end, end + GUARD))
        pos = end + GUARD
        u[i]["in_off"], u[i]["in_len"], u[i]["out_off"], u[i]["out_len"] = in_off[i], it.in_len, out, it.out_len
        u[i]["kind"], u[i]["window_bits"], u[i]["reset_frames"], u[i]["flags"] = it.kind, it.wb, it.reset, it.flags
        u[i]["e8_base"] = it.log_cap if it.flags & UF_MSZIP_LOG and it.kind == M.KIND_MSZIP else it.e8_base
        u[i]["ref_len"] = len(it.ref) if it.kind == M.KIND_LZX_DELTA else it.log_cap if it.flags & UF_LZX_LOG else \
            len(it.marks) if it.marks is not None else 0
        u[i]["in_chunk"] = tab_at[i] // 4 if (it.tab is not None or it.marks is not None) else it.in_chunk
        assert in_off[i] % 16 == (it.ri + it.skip) % 16 or it.share is not None
        assert out % 128 == it.ro % 128
    fr = M.frames_of(u)
    u["frame_base"] = np.concatenate([[0], np.cumsum(fr)[:-1]]) if n else 0
    L.units, L.out_bytes, L.n_frames = u, pos, int(fr.sum())
    L.cls = np.zeros(pos, dtype=np.uint8)
    L.owner = np.zeros(pos, dtype=np.int32)
    for i, (it, (lo, ref0, out, _end, hi)) in enumerate(zip(items, L.span)):
        L.owner[lo:hi] = i
        L.cls[ref0:out] = REFERENCE
        for a, b, c in it.owned(out):
            L.cls[a:b] = c
    return L


class Want:
    """what the oracle says of one item: the result words, the bytes, the log / marks entries that are compared (uint32s from the
    log's first byte on) and whether the bytes can be held against the kernel's (trusted)"""

    def __init__(self, err, flags, out_len, in_next, in_used, data, log=None, trusted=True):
        self.err, self.flags, self.out_len, self.in_next, self.in_used = int(err), int(flags), int(out_len), int(in_next), int(in_used)
        self.data, self.log, self.trusted = data, log, trusted


def oracle(it):
    """the oracle's answer for the item given stream[skip : skip + in_len] (with a failing feeder where the unit says so).  An item
    no oracle covers (KWAJ-framed MSZIP) brings its own: it.want"""
    if it.want is not None:
        return it.want
    data = it.data()
    H.oracle_set_hard_eof(bool(it.flags & UF_HARD_EOF))
    try:
        log = None
        if it.kind == M.KIND_LZX:
            e, o, r = H.oracle_lzx(data, it.out_len, it.wb, it.reset, length=it.out_len, e8_base=it.e8_base)
            if it.flags & UF_LZX_LOG:                                    # (tests/test_gpu_lzx_log.py: the count, then the entries that fit)
                cnt, frames = H.oracle_lzx_open_resets(max(it.log_cap, 1))
                log = [cnt] + frames[:min(cnt, it.log_cap)]
        elif it.kind == M.KIND_LZX_DELTA:
            e, o, r = H.oracle_lzxd(data, it.out_len, it.wb, it.ref)
        elif it.kind == M.KIND_MSZIP:
            e, o, r, _bl = H.oracle_mszip(data, it.out_len, 0 if not it.flags & M.UF_MSZIP_REPAIR else (it.in_chunk or 1))
        else:
            assert it.kind == M.KIND_QUANTUM
            if it.marks is not None:                                     # (tests/test_gpu_qtm.py: every entry)
                _e, log = H.oracle_qtm_marks(data, it.out_len, it.wb, it.marks)
            e, o, r = H.oracle_qtm(data, it.out_len, it.wb)
    finally:
        H.oracle_set_hard_eof(0)
    n = min(int(r.out_len), it.out_len)
    # A damaged stream may copy from window bytes the reference never wrote (tests/test_gpu_fuzz.py): where the plaintext is known
    # and the oracle's bytes are not its beginning, a FAILING unit's bytes are not held against the kernel's
    complete = e == 0 and r.out_len == it.out_len
    trusted = complete or it.plain is None or o[:n] == it.plain[:n]
    return Want(e, r.flags, r.out_len, r.in_next, r.in_used, o[:n], log, trusted)


def expected_image(L, wants, fill):
    """-> (expected bytes, mask): `fill` everywhere, the reference data as placed, the oracle's bytes in [out_off, out_off + its
    out_len), the compared log entries; True in mask = unspecified (the rest of what the unit owns).  Asserts the two conditions on
    masking: nothing of a completely decoded unit's output is masked, nothing outside owned regions is"""
    exp = np.full(L.out_bytes, fill, dtype=np.uint8)
    mask = np.zeros(L.out_bytes, dtype=bool)
    for it, (_lo, ref0, out, _end, _hi), w in zip(L.items, L.span, wants):
        exp[ref0:out] = np.frombuffer(it.ref, dtype=np.uint8)
        for a, b, _c in it.owned(out):
            mask[a:b] = True
        n = min(w.out_len, it.out_len)
        if w.trusted:
            exp[out:out + n] = np.frombuffer(w.data[:n], dtype=np.uint8)
            mask[out:out + n] = False
        if it.kind == M.KIND_MSZIP and w.err == 0 and w.in_next and it.plain is not None and not it.flags & UF_MSZIP_KWAJ:
            # (tests/test_gpu_mszip.py: what the last block inflated to beyond the request lies in the slack)
            more = it.plain[it.out_len:it.out_len + w.in_next]
            exp[out + it.out_len:out + it.out_len + len(more)] = np.frombuffer(more, dtype=np.uint8)
            mask[out + it.out_len:out + it.out_len + len(more)] = False
        if w.log is not None:
            raw = np.asarray(w.log, dtype=np.uint32).view(np.uint8)
            a = it.log_at(out)
            exp[a:a + raw.size] = raw
            mask[a:a + raw.size] = False
        if w.err == 0 and w.out_len == it.out_len:
            assert not mask[out:out + it.out_len].any(), ("output of a completely decoded unit is masked", it.name)
    assert not mask[(L.cls == NOBODY) | (L.cls == REFERENCE)].any(), "a byte outside every owned region is masked"
    return exp, mask


def compare(image, exp, mask, L):
    """the whole image against the expected one; the first differing byte and how many differ, with the unit it belongs to"""
    image = np.asarray(image, dtype=np.uint8)
    assert image.size == exp.size == mask.size == L.out_bytes, (image.size, exp.size, L.out_bytes)
    bad = np.flatnonzero((image != exp) & ~mask)
    if bad.size:
        p = int(bad[0])
        i = int(L.owner[p])
        it, u = L.items[i], L.units[i]
        raise AssertionError(
            "byte %d of the image is 0x%02X, not 0x%02X: %s of unit %d (%s), %+d from its out_off (out_off %% 128 = %d, in_off %% 16 = %d, "
            "out_len %d, ref_len %d, flags 0x%X); %d bytes differ, the last one at %d" % (
                p, image[p], exp[p], CLASS_NAMES[L.cls[p]], i, it.name, p - int(u["out_off"]), int(u["out_off"]) % 128,
                int(u["in_off"]) % 16, it.out_len, len(it.ref), it.flags, bad.size, int(bad[-1])))


def qtm_good_len_ok(it, r):
    """a failing Quantum unit's good_len: a request that ends there succeeds in the reference, the next longer one fails as the unit did"""
    g = int(r["good_len"])
    H.oracle_set_hard_eof(bool(it.flags & UF_HARD_EOF))
    try:
        if g > it.out_len or H.oracle_qtm(it.data(), g, it.wb)[0] != 0:
            return False
        return g == it.out_len or H.oracle_qtm(it.data(), g + 1, it.wb)[0] == r["err"]
    finally:
        H.oracle_set_hard_eof(0)


def check_results(L, res, wants):
    """err, flags without FRAMES_ADOPTED, out_len, good_len, in_next against the oracle; in_used for Quantum units (the reference's
    i_ptr) and for units with MSPACK_HIP_UF_CRC32 (the digest of the oracle's bytes)"""
    for i, (it, w) in enumerate(zip(L.items, wants)):
        r = res[i]
        what = (i, it.name, "out_off %% 128 = %d, in_off %% 16 = %d" % (int(L.units["out_off"][i]) % 128, int(L.units["in_off"][i]) % 16),
                r, "oracle:", w.err, w.flags, w.out_len, w.in_next, w.in_used)
        assert r["err"] == w.err and (int(r["flags"]) & ~ADOPTED) == w.flags and r["out_len"] == w.out_len, what
        if it.kind != M.KIND_QUANTUM:                       # (the header gives in_next a meaning for LZX and MSZIP only)
            assert r["in_next"] == w.in_next, what
        if it.kind == M.KIND_QUANTUM and w.err != 0:
            assert qtm_good_len_ok(it, r), ("good_len",) + what
        else:
            assert r["good_len"] == w.out_len, what
        if it.flags & M.UF_CRC32:
            if w.trusted:
                assert r["in_used"] == (zlib.crc32(w.data[:w.out_len]) ^ 0xFFFFFFFF) & 0xFFFFFFFF, ("digest",) + what
        elif it.kind == M.KIND_QUANTUM and it.want is None:
            assert r["in_used"] == w.in_used, what
