"""mspack_lzx_pipe's UNIFORM launches (entry_kernels.hpp: every unit of the launch carries a frame table and all have the same number
of real frames, so F != 0) fed with damaged, hand-built and other-mode streams: a frame's parse and resolve tasks are separate tickets
of different waves there, and everything between them goes through the status words of LzxFrameRec.  Every other test that feeds the
pipe anything but clean one-block-per-frame streams mixes frame counts and so runs in frame-slot order (parse and resolve by one wave).

Uniformity is asserted before every launch (uniform_frames: the map kernel's rule restated), F <= 3 keeps the fold tasks out
(LZX_FOLD_MIN_FRAMES == 4), and every batch stays below the host path's chunking thresholds (one_chunk: plan_chunks' rule restated),
so one call is one LZX launch.

Batches, built once by the module's fixture and handed to the child processes as pickle files:
  * crafted_{1,2,3}f_k{4,40}: crafted_streams.lzx_cases() by frame count -- 20 / 8 / 10 cases, 7 / 1 / 0 of them failing (asserted) --,
    every case k times, case-minor in the unit table.  (The host path launches longest unit first, equal lengths in table order: there
    a case's copies are neighbours again.  The device-resident entry launches in table order; the k = 4 batches go through it too.)
  * corpus_{96x2,400x2,64x3}: corpus_lzx_units with frame tables, window 21, one reset interval per unit.  Every third unit is clean,
    the others cycle through CYCLE: one bit flipped in the first 40 bytes of frame 0 (header, pretree), in the middle of frame 0's
    tokens, 300 bytes behind tab[1]; in_len cut at tab[1], tab[1] + 1, a third of frame 0, 5 bytes before the end; tab[1] +- 2, 0,
    tab[0], beyond in_len; the same plaintext encoded with mode 3, mode 4 / block_size 20000, block_size 9999.
    The flip behind tab[1] stands four times in the cycle: the oracle counts its out_len in whole frames, so a unit whose frame 0
    is damaged has NO prefix to compare, and "at least half of the bit-flipped units compared over a non-empty prefix" can only be
    met by units damaged behind frame 0 (four of six flips, their bit the first of a seeded order at which the oracle notices the
    damage; asserted per batch from the oracle's results alone: 13 of 22, 54 of 89 and 8 of 15).
  * all_bad_96x2: every unit damaged in frame 0 (header flip, token flip, cut at a third of frame 0), so hardly a chain survives its
    first link.  A flipped unit has a prefix to compare only where the flip did no harm to frame 0 (4 of its 64 flipped units: a
    code length no token of frame 0 uses): the share of one half cannot be met by any seed here and is NOT asked of this batch; err,
    out_len, in_next, flags and whatever prefix there is are.

Compared, always against the oracle (helpers.oracle_lzx, computed once in the parent) and never against another GPU run: err, out_len,
in_next, flags without FRAMES_ADOPTED of every unit; all bytes of clean, wrong-table and other-mode units against the plaintext; of
truncated units the oracle's whole out_len prefix against the plaintext (asserted to be the plaintext's); of bit-flipped units the
prefix where the oracle's own output is the plaintext (the rule of test_damaged_streams_with_tables); of crafted units every byte up
to the oracle's out_len against the oracle's, and against the case's own plaintext.  Every environment's results and a digest of
its compared bytes must also equal the first environment's.  Through mspack_hip_decode_batch_device (own scratch, output arena between
guard bytes of 0xA5) go corpus_96x2 and the k = 4 crafted batches in every child: same parity, nothing outside the arena changes.

Path evidence (mspack_hip_debug_frame_words behind the device-resident entry; a pipe that hands every frame to the serial decoder
passes every parity check).  What the code says (lzx_pipe_resolve.hpp, lzx_pipe_parse.hpp, lzx_unit.hpp):
  * the first frame that is not whole, or the unit's LAST frame when all are whole, writes rs_* into the unit's first record: in a
    uniform launch EVERY unit ends with rs_valid == 1, and rs_frame is the number of leading frames with chain == LZX_CH_DONE (1);
    every frame behind the first that is not DONE has chain == LZX_CH_ENDED (2);
  * a parse task whose predecessor in the same reset interval published LZX_ST_FAILED (4) publishes FAILED itself, speculative header
    or not (lzx_pipe_parse: the chain of code lengths ends there);
  * clean units: every frame LZX_ST_EMITTED (7), FRAMES_ADOPTED set, chain == 1 in every frame but the last.  The last frame is NOT
    always whole: the last 64 bytes of a unit's input belong to the serial decoder's EOF-exact reader, so the last frame's record
    usually ends a few tokens early -- then its chain word is ENDED, rs_frame names it and rs_partial == 1 (the serial decoder goes on
    behind the record's last token); a last frame that is whole has chain == 1 and rs_frame == the unit's frames;
  * damaged 300 bytes behind tab[1] and the oracle stops in frame 1: frame 0 EMITTED with chain == 1, rs_frame == 1;
  * damaged in frame 0's header and the oracle stops in frame 0: rs_frame == 0;
  * other-mode units: rs_valid != 0 (mode 3 / 4: stored blocks end the chain; block_size 9999 in mode 0 is several verbatim blocks per
    frame, which the parse tasks take since round 5 -- those units come out whole and adopted, which is evidence too).

Environments, one fresh child process each (the knobs are read when the library loads): as it is; MSPACK_HIP_STREAM_RESOLVE=0;
MSPACK_HIP_TICKET_ORDER=0, 1, 2; MSPACK_HIP_PIPE_WAVES_PER_CU=1 (256 waves on this part: the k = 40 batches and corpus_400x2 then have
more tickets than waves and no stream resolve) alone and with MSPACK_HIP_TICKET_ORDER=1 and 2.

Wall times on an MI355X: building the batches and the first child 3.8 s (the module's fixtures), every further child 0.8 to 0.95 s
from start to end, test_chunked_batch_with_truncated_units 2.2 s.

tests/test_emu_kernels.py runs run_child on the wavefront emulator with small batches (emu_batches)."""
import hashlib
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

import crafted_streams as CS
import libmspack_amd as M
from helpers import oracle_lzx

pytestmark = pytest.mark.gpu
ADOPTED = M.F_FRAMES_ADOPTED
FRAME = 32768
GUARD, FILL = 4096, 0xA5
MASK_FRAME_TABLES = 0x80000000
ST_FAILED, ST_EMITTED, CH_DONE, CH_ENDED = 4, 7, 1, 2          # lzx_pipe.hpp LZX_ST_*, lzx_pipe_resolve.hpp LZX_CH_*
W_STATUS, W_BYTES, W_CHAIN, W_RS_VALID, W_RS_FRAME, W_RS_PARTIAL = 0, 2, 3, 5, 6, 7      # mspack_hip_debug_frame_words: the words of a slot

FLIPS = ("flip_header", "flip_tokens", "flip_behind_tab1")
CUTS = ("cut_tab1", "cut_tab1_plus_1", "cut_third_of_frame0", "cut_5_before_end")
TABLES = ("tab1_plus_2", "tab1_minus_2", "tab1_zero", "tab1_is_tab0", "tab1_beyond_in_len")
MODES = {"mode3": dict(mode=3), "mode4_bs20000": dict(mode=4, block_size=20000), "bs9999": dict(block_size=9999)}
CYCLE = ["flip_header", "flip_behind_tab1", "cut_tab1", "tab1_plus_2", "mode3", "flip_tokens", "flip_behind_tab1", "cut_tab1_plus_1",
         "tab1_minus_2", "mode4_bs20000", "flip_behind_tab1", "cut_third_of_frame0", "tab1_zero", "bs9999", "cut_5_before_end",
         "tab1_is_tab0", "flip_behind_tab1", "tab1_beyond_in_len"]
ALL_BAD_CYCLE = ["flip_header", "flip_tokens", "cut_third_of_frame0"]
assert set(CYCLE) == set(FLIPS) | set(CUTS) | set(TABLES) | set(MODES)

ENVS = [("as_it_is", {}),
        ("no_stream_resolve", {"MSPACK_HIP_STREAM_RESOLVE": "0"}),
        ("level_order", {"MSPACK_HIP_TICKET_ORDER": "0"}),
        ("mixed_sections", {"MSPACK_HIP_TICKET_ORDER": "1"}),
        ("unit_major", {"MSPACK_HIP_TICKET_ORDER": "2"}),
        ("one_wave_per_cu", {"MSPACK_HIP_PIPE_WAVES_PER_CU": "1"}),
        ("one_wave_per_cu_mixed_sections", {"MSPACK_HIP_PIPE_WAVES_PER_CU": "1", "MSPACK_HIP_TICKET_ORDER": "1"}),
        ("one_wave_per_cu_unit_major", {"MSPACK_HIP_PIPE_WAVES_PER_CU": "1", "MSPACK_HIP_TICKET_ORDER": "2"})]
KNOBS = ("MSPACK_HIP_STREAM_RESOLVE", "MSPACK_HIP_TICKET_ORDER", "MSPACK_HIP_PIPE_WAVES_PER_CU", "MSPACK_HIP_NO_FRAME_PARSE", "MSPACK_HIP_FOLD")


# ---- a batch: items (a stream, how much of it the unit may read, a frame table, the oracle's word on it) and the units' items -----
class Batch:
    def __init__(self, name, device=False):
        self.name, self.device = name, device          # device: goes through the device-resident entry too
        self.host = True                               # ... and through the host entry (the emulator's twin drops it for one batch)
        self.items, self.unit_item = [], []
        self.plain = None                              # corpus batches: the units' plaintexts back to back

    def add(self, stream, in_len, tab, out_len, wb, reset, kind, what, plain=None, plain_off=None):
        """the item and the oracle's result for it; what may be compared of its bytes (the module's docstring)"""
        e, o, r = oracle_lzx(stream[:in_len], out_len, wb, reset)
        it = dict(stream=stream, in_len=in_len, tab=[int(t) & 0xFFFFFFFF for t in tab], out_len=out_len, wb=wb, reset=reset, kind=kind,
                  what=what, err=e, r_out_len=int(r.out_len), r_in_next=int(r.in_next), r_flags=int(r.flags), ref=None, plain_off=plain_off,
                  cmp_len=0)
        n = int(r.out_len)
        if kind == "crafted":
            it["ref"], it["cmp_len"] = o[:n], n
            assert plain is None or (e == 0 and o[:n] == plain), what
        else:
            p = bytes(self.plain[plain_off:plain_off + out_len])
            same = o[:n] == p[:n]
            if kind == "clean" or kind in TABLES or kind in MODES:
                assert e == 0 or n == out_len, (what, kind, e, n)     # (a stream that ends on a reset point: ERR_READ behind every byte)
                assert n == out_len and same, (what, kind)
                it["cmp_len"] = n
            elif kind in CUTS:
                assert same, (what, kind, "a cut stream decodes correctly until its input ends")
                it["cmp_len"] = n
            else:
                assert kind in FLIPS
                it["cmp_len"] = n if same else 0
        self.items.append(it)
        return len(self.items) - 1


def uniform_frames(units):
    """mspack_lzx_pipe_map's rule restated: every unit is KIND_LZX, carries UF_FRAME_TABLE, and all have the same number of real frames
    -> that number (ctl[0] == ctl[1] != 0, so F != 0); below LZX_FOLD_MIN_FRAMES (4), so the fold rule cannot take the launch"""
    assert len(units) and (units["kind"] == M.KIND_LZX).all() and ((units["flags"] & M.UF_FRAME_TABLE) != 0).all()
    fr = (units["out_len"].astype(np.int64) + FRAME - 1) // FRAME
    assert fr.min() == fr.max() and 1 <= fr[0] <= 3, (int(fr.min()), int(fr.max()))
    return int(fr[0])


def one_chunk(units):
    """plan_chunks' rule restated (host_plan.hpp; the knobs' defaults, which no variable may have changed): as many chunks as 8 MiB of
    input and 256 units each allow -- fewer than two here"""
    assert not [k for k in os.environ if k.startswith("MSPACK_HIP_CHUNK") or k == "MSPACK_HIP_NCHUNKS"]
    assert min(int(units["in_len"].astype(np.int64).sum()) // (8 << 20), len(units) // 256) < 2


def lay_out(b):
    """-> (units, arena, out_bytes): every item's stream and table once in the arena (8 zero bytes behind a stream)"""
    offs, toffs, pos = [], [], 0
    for it in b.items:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(it["stream"]) + 8
        pos = (pos + 3) & ~3
        toffs.append(pos); pos += 4 * len(it["tab"])
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for it, o, to in zip(b.items, offs, toffs):
        arena[o:o + len(it["stream"])] = np.frombuffer(it["stream"], dtype=np.uint8)
        arena[to:to + 4 * len(it["tab"])] = np.asarray(it["tab"], dtype=np.uint32).view(np.uint8)
    ix = np.asarray(b.unit_item)
    col = lambda v: np.asarray(v)[ix]
    units, out_bytes = M.make_units(M.KIND_LZX, col(offs), col([it["in_len"] for it in b.items]), col([it["out_len"] for it in b.items]),
                                    window_bits=col([it["wb"] for it in b.items]), reset_frames=col([it["reset"] for it in b.items]),
                                    frame_tabs=col(toffs))
    return units, arena, out_bytes


# ---- the batches ------------------------------------------------------------------------------------------------------------------
def crafted_batches(ks, frames=(1, 2, 3)):
    cases = CS.lzx_cases()
    by = {}
    for c in cases:
        by.setdefault((c.out_len + FRAME - 1) // FRAME, []).append(c)
    # (the case list as the suite's author counted it: a change there should be looked at here)
    assert {f: (len(v), sum(c.err != 0 for c in v)) for f, v in by.items()} == {1: (20, 7), 2: (8, 1), 3: (10, 0), 4: (1, 0), 6: (1, 0)}
    assert all(c.err in (0, M.ERR_DECRUNCH) for f in (1, 2, 3) for c in by[f])
    out = []
    for f in frames:
        first = None
        for k in ks:
            b = Batch("crafted_%df_k%d" % (f, k), device=k <= 4)
            if first is None:
                for c in by[f]:
                    b.add(c.stream, len(c.stream), c.tab, c.out_len, c.wb, c.reset, "crafted", c.name, plain=c.plain)
                first = b
            else:
                b.items = first.items
            b.unit_item = [j for _ in range(k) for j in range(len(b.items))]          # case-minor
            out.append(b)
    return out


def corpus_batch(name, n, frames, seed, cycle=CYCLE, every_third_clean=True, device=False, kinds=None):
    """n units of `frames` frames (window 21, one reset interval each); kinds: the units' kinds spelled out (the emulator's batch)"""
    ub = frames * FRAME
    plain, comp, off, ln, tab = M.corpus_lzx_units(seed, M.TEXT_MIX, n, ub, 21, n_threads=8, frame_tables=True)
    rng = np.random.default_rng(seed)
    b = Batch(name, device=device)
    b.plain = plain
    damaged = 0
    for i in range(n):
        s = comp[int(off[i]):int(off[i]) + int(ln[i]) + 4].tobytes()                 # (the stream goes on behind an interval, as in a CHM)
        t = comp[int(tab[i]):int(tab[i]) + 4 * frames].view(np.uint32).astype(np.int64)
        assert t[0] == 0 and (np.diff(t) > 400).all() and t[-1] + 400 < len(s)
        if kinds is not None:
            kind = kinds[i]
        elif every_third_clean and i % 3 == 0:
            kind = "clean"
        else:
            kind = cycle[damaged % len(cycle)]; damaged += 1
        in_len, t1 = len(s), int(t[1])
        if kind in FLIPS:
            at = {"flip_header": int(rng.integers(0, 40)), "flip_tokens": t1 // 2 + int(rng.integers(-200, 200)), "flip_behind_tab1": t1 + 300}[kind]
            bits = [int(x) for x in rng.permutation(8)]
            if kind == "flip_behind_tab1":
                # (the seed's choice, made from the oracle alone: the first bit of the order at which the reference notices the damage --
                # a flip that only turns one literal into another leaves nothing to compare; the module's docstring)
                bits = [x for x in bits if oracle_lzx(s[:at] + bytes([s[at] ^ (1 << x)]) + s[at + 1:], ub, 21, frames)[0] != 0][:1] or bits
            sb = bytearray(s); sb[at] ^= 1 << bits[0]; s = bytes(sb)
        elif kind in CUTS:
            in_len = {"cut_tab1": t1, "cut_tab1_plus_1": t1 + 1, "cut_third_of_frame0": t1 // 3, "cut_5_before_end": in_len - 5}[kind]
        elif kind in TABLES:
            t = t.copy()
            t[1] = {"tab1_plus_2": t1 + 2, "tab1_minus_2": t1 - 2, "tab1_zero": 0, "tab1_is_tab0": int(t[0]), "tab1_beyond_in_len": in_len + 1000}[kind]
        elif kind in MODES:
            c2, f2 = M.lzx_encode(plain[i * ub:(i + 1) * ub], 21, frames, M.lzx_opts(**MODES[kind]))
            s, t = c2.tobytes() + bytes(4), f2.astype(np.int64)[:-1]
            in_len = len(s)
        else:
            assert kind == "clean"
        b.unit_item.append(b.add(s, in_len, t, ub, 21, frames, kind, "%s unit %d" % (name, i), plain_off=i * ub))
    return b


def flip_share(b):
    """of the batch's bit-flipped units: (how many, how many of them are byte-compared over a non-empty prefix)"""
    fl = [b.items[j] for j in b.unit_item if b.items[j]["kind"] in FLIPS]
    return len(fl), sum(it["cmp_len"] > 0 for it in fl)


def gpu_batches():
    out = crafted_batches((4, 40))
    shapes = [corpus_batch("corpus_96x2", 96, 2, 0x0F96, device=True), corpus_batch("corpus_400x2", 400, 2, 0x0F400), corpus_batch("corpus_64x3", 64, 3, 0x0F64)]
    for b in shapes:
        kinds = [b.items[j]["kind"] for j in b.unit_item]
        assert all(k == "clean" for k in kinds[::3]) and set(kinds) == set(CYCLE) | {"clean"}
        n, cmp_ = flip_share(b)
        assert n >= 10 and 2 * cmp_ >= n, (b.name, "bit-flipped units", n, "compared over a non-empty prefix", cmp_)
    bad = corpus_batch("all_bad_96x2", 96, 2, 0x0BAD, cycle=ALL_BAD_CYCLE, every_third_clean=False)
    for it in bad.items:
        # (every unit damaged in frame 0; what the oracle leaves of a flipped one is nothing, or not the plaintext)
        assert it["kind"] in ALL_BAD_CYCLE, it["what"]
        assert it["r_out_len"] == 0 or it["kind"] in FLIPS, it["what"]
    return out + shapes + [bad]


EMU_KINDS = ["clean", "flip_header", "flip_tokens", "flip_behind_tab1", "cut_tab1", "cut_third_of_frame0", "cut_5_before_end", "tab1_plus_2",
             "tab1_zero", "tab1_beyond_in_len", "mode3", "bs9999"]


def emu_batches():
    """the emulator's twin: the two-frame crafted batch at k = 1 (k = 2 did not fit the twin's time) and twelve corpus units, one per
    damage kind"""
    crafted = crafted_batches((1,), frames=(2,))
    crafted[0].device = False                  # (host entry only: the emulator's time)
    corpus = corpus_batch("corpus_12x2", len(EMU_KINDS), 2, 0x0E12, device=True, kinds=EMU_KINDS)
    corpus.host = False                        # (device-resident entry only, with the path evidence: the emulator's time)
    return crafted + [corpus]


# ---- one launch and its checks ------------------------------------------------------------------------------------------------------
def check(b, units, out, res, how, digest):
    oo = units["out_off"].astype(np.int64)
    for i, j in enumerate(b.unit_item):
        it = b.items[j]
        what = (how, b.name, i, it["what"], it["kind"], res[i], it["err"], it["r_out_len"], it["r_in_next"], it["r_flags"])
        assert res["err"][i] == it["err"] and res["out_len"][i] == it["r_out_len"] and res["in_next"][i] == it["r_in_next"], what
        assert (int(res["flags"][i]) & ~ADOPTED) == it["r_flags"], what
        n = it["cmp_len"]
        got = out[oo[i]:oo[i] + n]
        ref = np.frombuffer(it["ref"], dtype=np.uint8) if it["ref"] is not None else b.plain[it["plain_off"]:it["plain_off"] + n]
        if not np.array_equal(got, ref):
            k = int(np.flatnonzero(got != ref)[0])
            raise AssertionError("%s, %s, unit %d (%s, %s): byte %d (frame %d + %d) is 0x%02X, not 0x%02X; %d bytes differ" % (
                how, b.name, i, it["what"], it["kind"], k, k // FRAME, k % FRAME, got[k], ref[k], int((got != ref).sum())))
        digest.update(got.tobytes())


def run_host(b, digest):
    units, arena, out_bytes = lay_out(b)
    uniform_frames(units); one_chunk(units)
    out, res = M.decode_batch(units, arena, out_bytes)
    check(b, units, out, res, "host entry", digest)
    return res


def run_device(b, digest):
    """the batch through mspack_hip_decode_batch_device with the test's own scratch, the output arena inside a larger buffer of FILL
    (tests/test_gpu_fold_crafted.py): parity, guards intact -> (results, per unit the frame words of its real frames)"""
    from test_gpu_hostpath import DevBuf
    from test_gpu_md5 import dev_write
    lib = M.lib()
    units, arena, out_bytes = lay_out(b)
    nreal = uniform_frames(units)
    u = np.ascontiguousarray(units)
    n_frames = int(M.frames_of(u).sum())
    big = DevBuf(out_bytes + 2 * GUARD, FILL)
    d_units, d_in = DevBuf(u.nbytes), DevBuf(arena.size + 64, 0xFF)
    d_res = DevBuf(len(u) * M.RESULT_DTYPE.itemsize, 0x77)
    scratch = DevBuf(max(int(lib.mspack_hip_frame_scratch_bytes(n_frames)), 16))
    dev_write(d_units, 0, u.view(np.uint8))
    dev_write(d_in, 0, arena)
    rc = lib.mspack_hip_decode_batch_device(d_units.ptr, None, len(u), d_in.ptr, arena.size, big.ptr + GUARD, out_bytes, d_res.ptr,
                                            scratch.ptr, n_frames, MASK_FRAME_TABLES | (1 << M.KIND_LZX), None)
    assert rc == 0, lib.mspack_hip_last_error()
    if big.emu is None:
        assert big.hip.hipDeviceSynchronize() == 0
    res = d_res.to_host()[:len(u) * M.RESULT_DTYPE.itemsize].view(M.RESULT_DTYPE).copy()
    words = [M.debug_frame_words(scratch.ptr, n_frames, int(u["frame_base"][i]), nreal) for i in range(len(u))]
    after = big.to_host()
    for x in (big, d_units, d_in, d_res, scratch):
        x.free()
    assert (after[:GUARD] == FILL).all() and (after[GUARD + out_bytes:] == FILL).all(), (b.name, "a byte outside the output arena changed")
    check(b, units, after[GUARD:GUARD + out_bytes], res, "device entry", digest)
    return res, words


def check_words(b, res, words):
    """the path evidence of the module's docstring"""
    seen = {}
    for i, j in enumerate(b.unit_item):
        it, w = b.items[j], words[i]
        nreal, reset = len(w), it["reset"]
        what = (b.name, i, it["what"], it["kind"], w.tolist(), res[i])
        done = 0
        while done < nreal and w[done][W_CHAIN] == CH_DONE:
            done += 1
        assert w[0][W_RS_VALID] == 1 and w[0][W_RS_FRAME] == done, what
        assert all(w[f][W_CHAIN] == CH_ENDED for f in range(done, nreal)), what
        assert all(w[f][W_STATUS] == ST_EMITTED for f in range(done)), what
        for f in range(1, nreal):
            if w[f - 1][W_STATUS] == ST_FAILED and (f % reset if reset else f) != 0:
                assert w[f][W_STATUS] == ST_FAILED, what
        # (what the oracle says of the stream bounds what the pipe may have finished: frames the oracle did not reach are not DONE)
        if it["err"] != 0:
            assert done * FRAME <= it["r_out_len"], what
        k = it["kind"]
        if k == "clean":
            assert all(w[f][W_STATUS] == ST_EMITTED for f in range(nreal)) and (res["flags"][i] & ADOPTED), what
            assert done == nreal or (done == nreal - 1 and w[0][W_RS_PARTIAL] == 1 and w[done][W_BYTES] > FRAME // 2), what
        elif k == "flip_behind_tab1" and it["err"] != 0 and it["r_out_len"] == FRAME:
            assert done == 1 and w[0][W_STATUS] == ST_EMITTED and (res["flags"][i] & ADOPTED), what
            seen["behind_tab1"] = seen.get("behind_tab1", 0) + 1
        elif k == "flip_header" and it["err"] != 0 and it["r_out_len"] == 0:
            assert done == 0, what
            seen["header"] = seen.get("header", 0) + 1
        seen[k] = seen.get(k, 0) + 1
    if b.plain is not None:
        assert seen.get("clean") and seen.get("behind_tab1") and seen.get("header") and any(seen.get(m) for m in MODES), (b.name, seen)


def run_child(directory, names, result_file):
    """every batch of `names` through the host entry, the `device` ones through the device-resident entry with the path evidence; what
    other environments' runs are held against goes into result_file"""
    t0 = time.time()
    assert not [k for k in os.environ if k == "MSPACK_HIP_NO_FRAME_PARSE" or k == "MSPACK_HIP_FOLD"]
    summary = {}
    for name in names:
        with open(os.path.join(directory, name + ".pickle"), "rb") as f:
            b = pickle.load(f)
        t1 = time.time()
        dig = hashlib.sha256()
        keep = []
        if b.host:
            res = run_host(b, dig)
            keep += [res["err"].copy(), res["out_len"].copy(), res["in_next"].copy(), res["flags"] & ~np.uint32(ADOPTED)]
        if b.device:
            res2, words = run_device(b, dig)
            check_words(b, res2, words)
            keep += [res2["err"].copy(), res2["out_len"].copy(), res2["in_next"].copy(), res2["flags"] & ~np.uint32(ADOPTED)]
        summary[name] = ([a.tolist() for a in keep], dig.hexdigest())
        print("%s: %d units, %.2f s" % (name, len(b.unit_item), time.time() - t1), flush=True)
    with open(result_file, "wb") as f:
        pickle.dump(summary, f)
    print("UNIFORM_OK in %.2f s" % (time.time() - t0))


def write_batches(directory, batches):
    for b in batches:
        with open(os.path.join(directory, b.name + ".pickle"), "wb") as f:
            pickle.dump(b, f, protocol=4)
    return [b.name for b in batches]


def start_child(directory, names, env_name, env, timeout, extra_env=None, text=None):
    """a fresh process for one environment -> its summary (what it printed is appended to `text`); a child that fails, dies or runs
    into its time limit fails the test"""
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env); e.update(extra_env or {})
    result = os.path.join(directory, "result_%s.pickle" % env_name)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), directory, result] + names, cwd=ROOT, env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout)
    assert p.returncode == 0 and b"UNIFORM_OK" in p.stdout, (env_name, p.returncode, p.stdout.decode()[-4000:])
    if text is not None:
        text.append(p.stdout.decode())
    with open(result, "rb") as f:
        return pickle.load(f)


# ---- the test: one process per environment ---------------------------------------------------------------------------------------------
_STATE = {"dead": None}


@pytest.fixture(scope="module")
def batch_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lzx_uniform"))
    return d, write_batches(d, gpu_batches())


@pytest.fixture(scope="module")
def first_run(built, batch_dir):
    """the first environment's run: what every other environment's results must equal besides the oracle's"""
    if _STATE["dead"]:
        pytest.fail("no further child is started: %s" % _STATE["dead"])
    try:
        return start_child(batch_dir[0], batch_dir[1], ENVS[0][0], ENVS[0][1], 240)
    except BaseException as ex:
        _STATE["dead"] = "the first environment's child failed (%s)" % type(ex).__name__
        raise


@pytest.mark.parametrize("env_name,env", ENVS, ids=[e[0] for e in ENVS])
def test_uniform_launches_vs_oracle(built, batch_dir, first_run, env_name, env):
    if env_name == ENVS[0][0]:
        return                                                  # (the fixture's run: it passed, or this test has failed with it)
    if _STATE["dead"]:
        pytest.fail("no further child is started: %s" % _STATE["dead"])
    try:
        got = start_child(batch_dir[0], batch_dir[1], env_name, env, 240)
    except BaseException as ex:
        _STATE["dead"] = "the child of %s failed (%s)" % (env_name, type(ex).__name__)
        raise
    assert got.keys() == first_run.keys()
    for name in got:
        assert got[name] == first_run[name], (env_name, name, "differs from the first environment's run")


def test_chunked_batch_with_truncated_units(built):
    """test_gpu_md5.chunked_batch(): 640 units of two frames that the planner cuts into chunks (asserted, as test_chunked_host_path
    does), so every chunk is a uniform launch that runs BESIDE the others: alone == false, a third as many waves as tickets
    (MSPACK_HIP_CHUNK_WAVE_DIV), no stream resolve.  Every seventh unit is truncated through in_len (at tab[1] + 1, a third of frame 0,
    5 bytes before the end in turn; the arena is untouched, so the stream goes on behind in_len): those against the oracle -- err,
    out_len, in_next, flags, and the oracle's whole prefix, which is the plaintext's --, the others against the plaintext."""
    from test_gpu_md5 import chunked_batch
    units, comp, out_bytes, plain, _ranges = chunked_batch()
    n, ub = len(units), 65536
    assert n == 640 and uniform_frames(units) == 2
    cut = np.arange(3, n, 7)
    for k, i in enumerate(cut):
        t1 = int(comp[int(units["in_chunk"][i]) * 4 + 4:int(units["in_chunk"][i]) * 4 + 8].view(np.uint32)[0])
        units["in_len"][i] = (t1 + 1, t1 // 3, int(units["in_len"][i]) - 5)[k % 3]
    assert not [k for k in os.environ if k.startswith("MSPACK_HIP_CHUNK") or k == "MSPACK_HIP_NCHUNKS"]
    assert min(4, int(units["in_len"].sum()) // (8 << 20), n // 256) >= 2
    out, res = M.decode_batch(units, comp, out_bytes)
    whole = np.ones(n, dtype=bool); whole[cut] = False
    assert (res["err"][whole] == 0).all() and (res["out_len"][whole] == ub).all()
    for i in range(n):
        o0 = int(units["out_off"][i])
        if whole[i]:
            assert np.array_equal(out[o0:o0 + ub], plain[i * ub:(i + 1) * ub]), i
            continue
        s = comp[int(units["in_off"][i]):int(units["in_off"][i]) + int(units["in_len"][i])].tobytes()
        e, o, r = oracle_lzx(s, ub, 17, 2)
        what = (i, res[i], e, r.out_len, r.in_next, r.flags)
        assert e != 0 and o[:r.out_len] == plain[i * ub:i * ub + r.out_len].tobytes(), what
        assert res["err"][i] == e and res["out_len"][i] == r.out_len and res["in_next"][i] == r.in_next, what
        assert (int(res["flags"][i]) & ~ADOPTED) == r.flags, what
        assert out[o0:o0 + r.out_len].tobytes() == o[:r.out_len], what


if __name__ == "__main__":
    run_child(sys.argv[1], sys.argv[3:], sys.argv[2])
