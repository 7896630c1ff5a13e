"""The hand-built streams of tests/crafted_streams.py through the kernels.  Every case in one batch per codec -- LZX and MSZIP
with and without their frame tables -- against the oracle (error, out_len, in_next, flags without FRAMES_ADOPTED, every byte
up to out_len) and against the helper's own plaintext; the multi-frame cases with one block per frame must really take the
frame-parallel path.  Then every valid LZX case 600 times in one batch with its frame table, so that the pipe's tickets no
longer all find a wave at once (the speculative header path and the other ticket orders run): ~16 000 units, ~900 MB of
output, 2.5 s on an MI355X."""
import numpy as np
import pytest

import crafted_streams as CS
import libmspack_amd as M
from helpers import oracle_lzx, oracle_lzxd, oracle_mszip
import test_gpu_lzx_frames as T
import test_gpu_lzxd as D
import test_gpu_mszip_blocks as B

pytestmark = pytest.mark.gpu
ADOPTED = M.F_FRAMES_ADOPTED
# several frames, one block per frame, a right table: the frame-parallel parse must adopt them
MUST_ADOPT = {"lzx_fixed_8_bit_literals_w21", "lzx_fixed_8_bit_literals_w15", "lzx_258_byte_matches_over_three_frames",
              "lzx_parse_wave_sub_tables_beyond_their_cap", "lzx_repeats_right_after_resets"}


def check_lzx(cases):
    streams, params, tabs, plains = [], [], [], []
    for c in cases:
        for tab in (np.asarray(c.tab, dtype=np.int64), None):
            streams.append(c.stream); params.append((c.out_len, c.wb, c.reset, 0)); tabs.append(tab); plains.append(c.plain)
    units, out, res = T.run(streams, params, tabs)
    T.check(streams, params, units, out, res)
    for i, p in enumerate(plains):
        if p is not None:
            assert res["err"][i] == 0 and out[units["out_off"][i]:units["out_off"][i] + len(p)].tobytes() == p, i
    for j, c in enumerate(cases):
        if c.name in MUST_ADOPT:
            assert res["flags"][2 * j] & ADOPTED, (c.name, res[2 * j])


def check_lzxd(cases):
    units, out, res = D.run_delta([c.stream for c in cases], [(c.out_len, c.wb) for c in cases], [c.ref for c in cases])
    for i, c in enumerate(cases):
        e, o, r = oracle_lzxd(c.stream, c.out_len, c.wb, c.ref)
        assert res["err"][i] == e == c.err, (c.name, res[i], e)
        assert res["out_len"][i] == r.out_len and res["flags"][i] == r.flags and res["in_next"][i] == r.in_next, (c.name, res[i])
        got = out[units["out_off"][i]:units["out_off"][i] + r.out_len].tobytes()
        assert got == o[:r.out_len], c.name
        assert c.plain is None or got == c.plain, c.name


def check_mszip(cases):
    streams, lens, tabs, plains = [], [], [], []
    for c in cases:
        for tab in (c.tab, None):
            streams.append(c.stream); lens.append(c.out_len); tabs.append(tab); plains.append(c.plain)
    units, out, res = B.run(streams, lens, tabs)
    B.check(streams, lens, units, out, res, plains)
    for i, s in enumerate(streams):
        c = cases[i // 2]
        e, _o, r, _bl = oracle_mszip(s, lens[i])
        assert res["err"][i] == e == c.err, (c.name, res[i])
        assert res["in_next"][i] == r.in_next and (int(res["flags"][i]) & ~ADOPTED) == r.flags, (c.name, res[i], r.in_next, r.flags)


def check_all(cases):
    check_lzx([c for c in cases if c.codec == "lzx"])
    check_lzxd([c for c in cases if c.codec == "lzxd"])
    check_mszip([c for c in cases if c.codec == "mszip"])


def test_crafted_streams_vs_oracle(built):
    check_all(CS.all_cases())


def test_valid_lzx_cases_600_times_in_one_batch(built):
    """(the 600 units of a case share one copy of its stream and its table in the arena)"""
    cases = [c for c in CS.lzx_cases() if c.err == 0]
    n = 600
    offs, toffs, pos = [], [], 0
    for c in cases:
        pos = (pos + 15) & ~15
        offs.append(pos); pos += len(c.stream) + 8
        pos = (pos + 3) & ~3
        toffs.append(pos); pos += 4 * len(c.tab)
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for c, o, to in zip(cases, offs, toffs):
        arena[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
        arena[to:to + 4 * len(c.tab)] = np.asarray(c.tab, dtype=np.uint32).view(np.uint8)
    rep = lambda v: np.repeat(np.asarray(v), n)
    units, out_bytes = M.make_units(M.KIND_LZX, rep(offs), rep([len(c.stream) for c in cases]), rep([c.out_len for c in cases]),
                                    window_bits=rep([c.wb for c in cases]), reset_frames=rep([c.reset for c in cases]),
                                    frame_tabs=rep(toffs))
    out, res = M.decode_batch(units, arena, out_bytes)
    for j, c in enumerate(cases):
        e, _o, r = oracle_lzx(c.stream, c.out_len, c.wb, c.reset)
        want = np.frombuffer(c.plain, dtype=np.uint8)
        for i in range(j * n, (j + 1) * n):
            assert res["err"][i] == e == 0 and res["out_len"][i] == r.out_len and res["in_next"][i] == r.in_next, (c.name, i, res[i])
            assert (int(res["flags"][i]) & ~ADOPTED) == r.flags, (c.name, i, res[i])
            assert c.name not in MUST_ADOPT or res["flags"][i] & ADOPTED, (c.name, i, res[i])
            assert np.array_equal(out[units["out_off"][i]:units["out_off"][i] + c.out_len], want), (c.name, i)
