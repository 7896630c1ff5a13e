"""The hand-built streams of tests/crafted_streams.py without a GPU: the helper's own plaintext against the oracle, the oracle
against the compiled reference (where it exists), each case's named property, and the whole set through the kernels on the
wavefront emulator (tests/test_emu_kernels.py builds it)."""
import os
import subprocess
import sys

import pytest

import crafted_streams as CS
from helpers import emu_so, have_ref, oracle_kwaj_lzh, oracle_lzss, oracle_lzx, oracle_lzxd, oracle_mszip, oracle_qtm, ref_lzx, \
    ref_lzxd, ref_mszip, ref_qtm, ref_szdd_kwaj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = CS.all_cases()


def run_oracle(c):
    if c.codec == "lzx":
        e, o, r = oracle_lzx(c.stream, c.out_len, c.wb, c.reset)
    elif c.codec == "lzxd":
        e, o, r = oracle_lzxd(c.stream, c.out_len, c.wb, c.ref)
    elif c.codec == "qtm":
        e, o, r = oracle_qtm(c.stream, c.out_len, c.wb)
    elif c.codec == "lzss":
        e, o, r = oracle_lzss(c.stream, c.wb, c.rooms[0])
    elif c.codec == "lzh":
        e, o, r = oracle_kwaj_lzh(c.stream, c.rooms[0])
    else:
        e, o, r, _ = oracle_mszip(c.stream, c.out_len)
    return e, o, r


def containers(c):
    """the files of the reference's drivers that carry the stream: -> [(kind 0 SZDD / 1 KWAJ, file bytes)].  SZDD files carry LZSS
    modes 0 and 2, KWAJ method 2 mode 2, KWAJ method 3 LZH; mode 1 (MS Help) has no container there"""
    if c.codec == "lzh":
        return [(1, CS.kwaj_container(c.stream, 3, c.out_len))]
    if c.wb == 0:
        return [(0, CS.szdd_container(c.stream, c.out_len))]
    if c.wb == 2:
        return [(0, CS.szdd_container(c.stream, c.out_len, qbasic=True)), (1, CS.kwaj_container(c.stream, 2, c.out_len))]
    return []


def test_case_names_are_unique():
    assert len({c.name for c in CASES}) == len(CASES) >= 40 + 70 + 25 + 35
    assert sum(c.codec == "qtm" for c in CASES) >= 70
    assert sum(c.codec == "lzss" for c in CASES) >= 25 and sum(c.codec == "lzh" for c in CASES) >= 35
    assert sum(len(c.plain) for c in CASES if c.codec in ("lzss", "lzh")) < 2 << 20


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_helper_plaintext_equals_the_oracle(built, c):
    e, o, r = run_oracle(c)
    assert e == c.err, (e, c.err)
    if c.plain is not None:
        assert r.out_len == c.out_len == len(c.plain)
        assert o == c.plain, "differs at byte %d" % next(k for k in range(len(o)) if o[k] != c.plain[k])
    if c.codec in ("lzss", "lzh"):
        assert r.in_used == c.props["in_used"], (r.in_used, c.props["in_used"])


# (an LZSS stream in mode 1 or 3 has no container in the reference: helper against oracle above is all there is for it)
REF_CASES = [c for c in CASES if not (c.codec == "lzss" and c.wb not in (0, 2))]


@pytest.mark.skipif(not have_ref(), reason="the compiled reference is not built")
@pytest.mark.parametrize("c", REF_CASES, ids=[c.name for c in REF_CASES])
def test_oracle_equals_the_reference(built, c):
    e, o, r = run_oracle(c)
    if c.codec in ("lzss", "lzh"):
        if c.props.get("ref_undefined"):
            pytest.skip("the reference reads uninitialised code lengths here: its answer is not defined")
        for kind, blob in containers(c):
            g = ref_szdd_kwaj(kind, blob)
            assert g["open_err"] == 0 and g["err"] == e and len(g["data"]) == r.out_len and g["data"] == o, (kind, g["err"], e, len(g["data"]), r.out_len)
        return
    if c.codec == "lzx":
        re, ro, rw = ref_lzx(c.stream, c.out_len, c.wb, c.reset)
    elif c.codec == "lzxd":
        re, ro, rw = ref_lzxd(c.stream, c.out_len, c.wb, c.ref)
    elif c.codec == "qtm":
        re, ro, rw = ref_qtm(c.stream, c.out_len, c.wb)
        if c.props["before_start"]:       # qtmd_init does not clear its window: what lies before the start is undefined there
            ro = o[:rw]
    else:
        re, ro, rw = ref_mszip(c.stream, c.out_len)
    assert re == e and rw == r.out_len and ro == o[:rw], (re, e, rw, r.out_len)


def by_name(name):
    return next(c for c in CASES if c.name == name)


def test_cases_have_the_property_they_name():
    """measured on what the builders wrote, not declared"""
    # pretree runs past the end of the table: non-zero lengths at and beyond `last`
    p = by_name("lzx_pretree_run_past_main_tree_end").props
    assert (512, 515) in p["overshoot"] and all(p["main_lens"][512:515])
    assert (256, 258) in by_name("lzx_pretree_run_past_literals_changes_delta_base").props["overshoot"]
    # window 2^25: entries 2576..2579 non-zero; the code is complete over 2576 symbols and over-subscribed over 2580
    p = by_name("lzxd_w25_main_tree_run_into_entries_2576_2579").props
    m = p["main_lens"]
    assert all(m[2576:2580]) and CS.kraft(m[:2576]) == 65536 < CS.kraft(m[:2580])
    # length symbol 249 has a code, and 258-byte matches were written (DELTA: and extended lengths)
    for name in ("lzx_258_byte_match_type1", "lzx_258_byte_match_type2", "lzx_258_byte_matches_over_three_frames",
                 "lzxd_extended_lengths_and_symbol_249"):
        p = by_name(name).props
        assert p["len_lens"][249] and 258 in p["lengths"], name
    assert max(by_name("lzxd_extended_lengths_and_symbol_249").props["lengths"]) >= 257 + 0x1500
    # main codes of every length; short codes that fill the table beside lengths that get no code
    assert by_name("lzx_main_codes_of_every_length_1_to_16").props["max_code_len"] == 16
    for name, longest in (("8_bit", 8), ("9_bit", 9), ("11_12_bit", 12)):
        p = by_name("lzx_short_codes_fill_longer_unreachable_" + name).props
        lens = p["main_lens"][:CS.MAIN_MAX]
        codes = CS.canon(lens, 12)
        assert p["max_code_len"] == longest and any(l > 12 and codes[s] is None for s, l in enumerate(lens)), name
    # fixed-width literals: every literal at 8 bits, nothing else in the tree, no match
    for name in ("lzx_fixed_8_bit_literals_w21", "lzx_fixed_8_bit_literals_w15"):
        p = by_name(name).props
        assert set(p["main_lens"][:256]) == {8} and not any(p["main_lens"][256:]) and "lengths" not in p
    # blocks of length 0 and odd uncompressed blocks
    bl = by_name("lzx_zero_length_and_odd_uncompressed_blocks").props["blocks"]
    assert (1, 0) in bl and (3, 0) in bl and (3, 1001) in bl and (3, 3) in bl
    # every slot behind the first frame (all of them at 2^15), verbatim and aligned
    for wb in (15, 17, 21):
        want = {s for s in range(3, CS.SLOTS[wb]) if CS.BASE[s] - 2 + (1 << CS.EXTRA[s]) - 1 <= CS.FRAME}
        assert wb != 15 or want == set(range(3, 30))
        for t in (1, 2):
            assert by_name("lzx_every_slot_w%d_type%d" % (wb, t)).props["slots"] >= want, (wb, t)
    # R1 / R2 swaps at the very start of every reset interval, while R0 = R1 = R2 = 1
    reps = by_name("lzx_repeats_right_after_resets").props["reps"]
    assert {(f * CS.FRAME + 1, 1, 1) for f in range(3)} <= set(reps)
    # E8: translation from frame 1 on only; the edges translate; filesize 0 translates nothing
    assert by_name("lzx_e8_switched_on_by_a_later_block").props["e8_translated"][0] == 0
    assert all(by_name("lzx_e8_switched_on_by_a_later_block").props["e8_translated"][1:])
    for name in ("lzx_e8_edges_last_frame_32768", "lzx_e8_edges_last_frame_5000"):
        assert all(by_name(name).props["e8_translated"])
    assert not any(by_name("lzx_uncompressed_e8_without_filesize").props["e8_translated"])
    # the parse waves' second-level table: beyond LZX_SUB_CAP (the fallback) in one case, within it in another
    p = by_name("lzx_parse_wave_sub_tables_beyond_their_cap").props
    assert CS.sub_table_total(p["main_lens"][:CS.main_syms(21)]) > CS.LZX_SUB_CAP and p["max_code_len"] == 16
    assert len(p["blocks"]) == 4 and len(by_name("lzx_parse_wave_sub_tables_beyond_their_cap").tab) == 4
    p = by_name("lzx_258_byte_matches_over_three_frames").props
    assert 256 < CS.sub_table_total(p["main_lens"][:CS.main_syms(21)]) <= CS.LZX_SUB_CAP
    # runs past the end: a zero run; and DELTA at 2^22..2^24, where the entries past the end count in the reference's table
    assert (CS.main_syms(16), CS.main_syms(16) + 17) in by_name("lzx_zero_run_18_past_main_tree_end").props["ran_past"]
    for wb in (22, 23, 24):
        p = by_name("lzxd_w%d_main_tree_run_past_its_end" % wb).props
        nm = CS.main_syms(wb)
        assert (nm, nm + 3) in p["overshoot"] and CS.kraft(p["main_lens"][:nm + 3]) == 65536 and (1 << (wb - 1)) in \
            {o for o, _pos in p["offsets"]}
    assert by_name("lzx_last_block_longer_than_the_output").props["blocks"] == [(1, 100000)]
    assert by_name("lzx_e8_in_a_last_frame_of_10_bytes").props["e8_translated"][1] == 0
    assert by_name("lzx_e8_in_a_last_frame_of_11_bytes").props["e8_translated"][1] == 1
    # MSZIP
    p = by_name("mszip_hlit_257_hdist_2").props
    assert p["max_hlit"] == 257 and p["max_hdist"] == 2
    p = by_name("mszip_stored_32768_empty_frame_distance_32768_code_284").props
    assert p["stored_lens"] == [32768, 0] and 257 + 27 in p["len_codes"] and p["max_dist"] == 32768
    c = by_name("mszip_bytes_before_the_ck_signature")
    assert [c.stream[t - 1:t] for t in c.tab[1:]] == [b"K", b"Q"]
    p = by_name("mszip_hlit_288_hdist_32").props
    assert p["max_hlit"] == 288 and p["max_hdist"] == 32
    assert by_name("mszip_repeat_code_16_at_position_0").props["repeat_at_0"]
    assert by_name("mszip_zero_run_18_across_the_literal_distance_boundary").props["runs_across"] == {18}
    assert by_name("mszip_zero_run_17_across_the_literal_distance_boundary").props["runs_across"] == {17}
    assert by_name("mszip_repeat_run_overruns_the_tables").props["run_overruns"]
    p = by_name("mszip_stored_blocks_zero_and_after_huffman_blocks").props
    assert p["stored_after_huffman"] >= 2 and 0 in p["stored_lens"]
    p = by_name("mszip_several_blocks_per_frame_distance_32768_code_284").props
    assert 257 + 27 in p["len_codes"] and p["max_dist"] == 32768


# what the coder-extremes search reaches (crafted_streams.qtm_search_extremes), frozen: the case must not quietly degrade.
# (k = n + mu >= 17, two 16-bit refills in one symbol, is not reached: an interval is never narrower than range / total - 1
# >= 2^14 / 3808 - 1 = 3, which leaves at most 14 leading bits in common, and an underflow run behind n shifts needs an interval
# narrower still.)
QTM_MAX_N, QTM_MAX_MU, QTM_MAX_K = 14, 13, 14


def test_quantum_cases_have_the_property_they_name(built):
    """measured on what the writer wrote (props), not declared"""
    Q = {c.name: c for c in CASES if c.codec == "qtm"}
    P = lambda name: Q[name].props
    # sources before the start: the offset is beyond P; zeros first, then real bytes; a period walked back more than once
    for p0 in (0, 1, 3):
        assert P("qtm_offset_beyond_the_start_at_P%d" % p0)["before_start"] == [p0]
    p = P("qtm_offset_of_the_whole_window_at_P0")
    assert p["before_start"][0] == 0 and max(p["slots"][6]) == 19 and 255 in p["slots"][6][19]
    assert P("qtm_match_reads_zeros_then_real_bytes")["before_start"] == [5, 13]
    assert P("qtm_periodic_match_from_before_the_start")["before_start"] == [2, 44, 303] and Q["qtm_periodic_match_from_before_the_start"].plain[2:9] == b"\0\0\0ab\0\0"
    p = P("qtm_w21_every_slot_of_models_4_5_6_from_before_the_start")
    assert [sorted(p["slots"][k]) for k in (4, 5, 6)] == [list(range(24)), list(range(36)), list(range(42))]
    assert p["max_raw"] == 19 and len(p["before_start"]) >= 72 and Q["qtm_w21_every_slot_of_models_4_5_6_from_before_the_start"].out_len < 4096
    # every slot with a real source: no match reads before the start; both ends of every slot's extra bits
    for wb in (10, 12, 17, 18, 21):
        p = P("qtm_every_slot_w%d" % wb)
        assert not p["before_start"], wb
        for sel, n in ((4, min(24, 2 * wb)), (5, min(36, 2 * wb)), (6, 2 * wb)):
            assert sorted(p["slots"][sel]) == list(range(n)), (wb, sel)
            assert all(p["slots"][sel][sl] >= {0, (1 << CS.QPE[sl]) - 1} for sl in range(n)), (wb, sel)
    assert all(P("qtm_every_slot_w12")["len_slots"][sl] >= {0, (1 << CS.QLE[sl]) - 1} for sl in range(27))
    assert 259 in P("qtm_every_slot_w12")["lengths"]
    c = Q["qtm_every_slot_w21"]
    assert c.out_len > (1 << 21) and (1 << 19) - 1 in c.props["slots"][6][41] and len(c.props["slots"][6][41]) >= 2
    # short periods; the literal buffer; the queue
    assert P("qtm_short_periods_1_to_64")["lengths"] >= {64, 65, 128, 259}
    assert set(range(6)) <= set(P("qtm_short_periods_1_to_64")["slots"][6])
    assert Q["qtm_queue_overflows_and_a_match_beyond_its_ring"].out_len > CS.SPQ_RING + 3 * CS.SPQ_CAP
    # window ends: a crossing match with its source before the start; one ending at the end; one starting on the last byte
    for wb in range(10, 15):
        c = Q["qtm_window_ends_w%d" % wb]
        w = 1 << wb
        assert len(c.props["crossing"]) == 3 and c.props["crossing"][0] == w - 10 == c.props["before_start"][0], wb
        assert (c.props["crossing"][1] + 1) % w == 0 and (c.props["crossing"][2] + 100) % w == 0, wb
    assert P("qtm_w15_frame_end_and_window_end_on_one_byte")["junk"] == [b"", b""]
    # frame ends: the trailers' junk, the eight alignments of the payload's end
    for n in (1, 4, 300):
        assert P("qtm_trailer_behind_%d_zero_bytes" % n)["junk"] == [bytes(n)] * 2
        j = P("qtm_trailer_behind_%d_nonzero_bytes" % n)["junk"]
        assert len(j[0]) == n and 0 not in j[0] and 255 not in j[0]
    for r_ in range(8):
        assert P("qtm_frame_payload_ends_at_bit_%d" % r_)["align"][0] == r_
    for nf in (1, 2):
        assert not Q["qtm_%d_whole_frames_without_the_last_trailer" % nf].stream.endswith(b"\xff")
        assert Q["qtm_%d_whole_frames_with_the_last_trailer" % nf].stream.endswith(b"\xff")
        assert Q["qtm_%d_whole_frames_with_the_last_trailer" % nf].out_len == nf * CS.FRAME
    # the models: at least two re-sorts, one of them with tied frequencies, of every model the case is about
    for kind in CS.QTM_PATTERNS:
        m = P("qtm_selector_model_%s" % kind)["model_sel"]
        assert m["resorts"] >= 2 and m["tied_resorts"] >= 1, (kind, m)
        for wb, sizes in ((10, (20, 20, 20)), (17, (24, 34, 34)), (21, (24, 36, 42))):
            p = P("qtm_literal_length_position_models_%s_w%d" % (kind, wb))
            assert tuple(p["model_" + k]["n"] for k in ("4", "5", "6")) == sizes
            for k in ("lit2", "6len", "4", "5", "6"):
                m = p["model_" + k]
                assert m["resorts"] >= 2 and m["tied_resorts"] >= 1, (kind, wb, k, m)
                if kind == "round_robin":
                    assert len(m["used"]) == m["n"], (wb, k)
    assert any(P("qtm_literal_length_position_models_%s_w21" % k)["model_6"]["moving_resorts"] for k in CS.QTM_PATTERNS)
    # the coder's extremes, against what one stream of the project's own encoder takes (tests/test_gpu_qtm.py)
    p = P("qtm_renormalisation_extremes")
    assert (p["max_n"], p["max_mu"], p["max_k"]) == (QTM_MAX_N, QTM_MAX_MU, QTM_MAX_K) and p["double_refills"] == 0
    import libmspack_amd as M
    d = M.gen_plaintext(9, M.TEXT_MIX, 120000)
    n, mu, k, plain = CS.qtm_read_maxima(M.qtm_encode(d, 16)[0], d.size, 16)
    assert plain == d.tobytes()
    print("the encoder's stream: n %d mu %d k %d" % (n, mu, k))
    assert QTM_MAX_N > n and QTM_MAX_MU > mu and QTM_MAX_K > k, (n, mu, k)
    # small requests
    assert [Q["qtm_request_of_%d_bytes" % n].out_len for n in (0, 1, 2)] == [0, 1, 2]
    assert [len(Q["qtm_input_of_%d_bytes" % n].stream) for n in range(4)] == [0, 1, 2, 3]
    c = Q["qtm_request_ends_inside_a_window_crossing_match"]
    assert c.props["crossing"] == [1014] and 1014 < c.out_len < 1024


def test_lzss_lzh_cases_have_the_property_they_name():
    """measured on what the writers wrote (props), not declared"""
    Z = {c.name: c for c in CASES if c.codec in ("lzss", "lzh")}
    P = lambda name: Z[name].props
    # ---- LZSS ----
    for m in (0, 1, 2):
        for n, wraps in ((3, 3), (18, 18)):
            c = Z["lzss_every_distance_at_length_%d_mode%d" % (n, m)]
            assert c.props["distances"][n] == set(range(1, 4097)) and not c.props["before_start"] and c.out_len >= wraps * 4096
            assert 0 not in c.plain[:4200] and 0x20 not in c.plain
        assert P("lzss_every_control_byte_mode%d" % m)["ctrl"] == set(range(256))
        p = P("lzss_every_control_byte_mode%d" % m)
        assert p["d1_behind_literal"] >= 50 and p["reads_previous_match"] >= 50
        assert P("lzss_source_from_the_prefill_into_data_mode%d" % m)["straddle"][0] == 2
        d = P("lzss_overlapping_matches_mode%d" % m)["distances"]
        assert d[18] >= {1, 2, 3, 7, 17, 18} and all(n in d[n] for n in range(3, 19))
        for groups in (1, 40):
            c = Z["lzss_maximum_expansion_%d_bytes_in_mode%d" % (17 * groups, m)]
            assert c.props["ratio"] == (144 * groups, 17 * groups) and c.props["ctrl"] == {0}
    a, b = Z["lzss_same_raw_items_mode0"], Z["lzss_same_raw_items_mode2"]
    assert a.stream == b.stream and a.plain != b.plain and len(a.plain) == len(b.plain)
    c = Z["lzss_same_raw_items_mode1"]                     # (mode 1: mode 0 with its control bytes inverted)
    assert c.plain == a.plain and c.stream != a.stream and c.stream[0] == a.stream[0] ^ 0xFF and c.stream[1:9] == a.stream[1:9]
    for d in (1, 16, 18, 4096):
        for m in (0, 2):
            p = P("lzss_first_item_is_a_match_at_distance_%d_mode%d" % (d, m))
            assert p["before_start"][0] == 0 and d in p["distances"][18]
    cuts = [Z["lzss_every_control_byte_first_%03d_bytes" % n] for n in range(301)]
    assert [len(c.stream) for c in cuts] == list(range(301)) and sorted(c.out_len for c in cuts) == [c.out_len for c in cuts]
    assert len({c.out_len for c in cuts}) > 100 and cuts[0].out_len == cuts[1].out_len == 0
    for m in (0, 1, 2):
        assert [len(Z["lzss_input_of_%d_bytes_mode%d" % (n, m)].stream) for n in range(4)] == [0, 1, 2, 3]
        assert [Z["lzss_input_of_%d_bytes_mode%d" % (n, m)].out_len for n in range(4)] == [0, 0, 0, 9]
    assert Z["lzss_mode_3_is_refused"].err == CS.ERR_ARGS
    # ---- KWAJ LZH ----
    for k in range(5):
        for typ in range(4):
            p = P("lzh_type_%d_on_tree_%d" % (typ, k))
            assert p["types"][k] == typ and all(p["used"]), (k, typ)
            assert typ != 0 or len(set(p["lens"][k])) == 1
    assert P("lzh_type_0_on_every_tree")["types"][:5] == [0] * 5
    # a 16-bit code, which only type 1's ++c from 15 can give, is used by a token; every code length 1..16 is
    for name in ("lzh_literal_codes_of_every_length_1_to_16", "lzh_type_1_runs_on_to_17_and_18"):
        p = P(name)
        assert p["types"][4] == 1 and max(l for l in p["lens"][4] if l <= 16) == 16 and p["used"][4] == set(range(1, 17)), name
    p = P("lzh_type_1_runs_on_to_17_and_18")
    assert sorted(l for l in p["lens"][4] if l > 16) == [17, 18, 18]
    assert all(CS.canon(p["lens"][4], 9)[s] is None for s, l in enumerate(p["lens"][4]) if l > 16)
    assert 16 in P("lzh_offset_codes_of_16_bits")["used"][3] and P("lzh_offset_codes_of_16_bits")["used"][1] >= set(range(2, 16))
    for k in (0, 2, 4):
        p = P("lzh_type_2_steps_to_255_and_back_tree_%d" % k)
        assert p["types"][k] == 2 and p["lens"][k].count(255) == 3
    p = P("lzh_type_3_with_15s")
    assert p["types"][:2] == [3, 3] and p["lens"][0].count(15) == 2 and 15 in p["used"][0] and 15 in p["used"][1]
    for k in range(5):
        lens = P("lzh_short_codes_fill_the_table_tree_%d" % k)["lens"][k]
        codes = CS.canon(lens, 9)
        assert sum(1 << (16 - l) for l in lens if 1 <= l <= 9) == 65536 and sorted(l for l in lens if l > 9) == list(range(10, 16))
        assert all((codes[s] is None) == (l > 9 or l == 0) for s, l in enumerate(lens))
    for k in range(5):
        K = lambda kind: P("lzh_tree_%d_%s" % (k, kind))["lens"][k]
        short = lambda lens: sum(1 << (16 - l) for l in lens if 1 <= l <= 9)
        assert short(K("oversubscribed_short_codes")) > 65536
        assert short(K("oversubscribed_long_codes_only")) < 65536 < CS.kraft(K("oversubscribed_long_codes_only"))
        assert short(K("incomplete")) < CS.kraft(K("incomplete")) < 65536
        assert not any(K("all_lengths_zero"))
        for kind in CS.LZH_BAD:
            c = Z["lzh_tree_%d_%s" % (k, kind)]
            assert c.err == CS.ERR_DATAFORMAT and len(c.props["lens"]) == k + 1 and all(CS.lzh_accepts(l) for l in c.props["lens"][:k])
    for typ in range(4, 16):
        c = Z["lzh_unknown_length_encoding_%d" % typ]
        assert c.props["types"][typ % 5] == typ and c.props["ref_undefined"]
    p = P("lzh_every_match_length_in_both_tables")
    assert p["match_syms"] == [set(range(1, 16))] * 2 and p["lens"][0] != p["lens"][1]
    assert P("lzh_offsets_0_1_63_64_65_4095")["offsets"] >= {0, 1, 63, 64, 65, 4095} and not P("lzh_offsets_0_1_63_64_65_4095")["before_start"]
    assert P("lzh_every_offset_symbol_low_bits_0_and_63")["offsets"] == {(s << 6) | low for s in range(64) for low in (0, 63)}
    for off in (0, 1, 63, 64, 4095):
        p = P("lzh_first_token_is_a_match_at_offset_%d" % off)
        assert p["before_start"][0] == 0 and off in p["offsets"]
    p = P("lzh_overlaps_at_distance_1_2_3_and_from_the_prefill_into_data")
    assert p["offsets"] >= {1, 2, 3, 5} and p["before_start"][0] == 2
    # both match-length tables, for a run and for a match, behind every predecessor they can have
    p = P("lzh_literal_runs_of_every_length_1_to_32")
    assert p["run_lens"] == set(range(1, 33)) and p["lens"][0] != p["lens"][1]
    assert p["tables"] >= {(0, "run32", "match"), (0, "run32", "run"), (0, "match", "run"), (0, "match", "match"),
                           (1, "run", "match"), (1, "run", "run"), (0, "start", "run")}
    assert not any(t == 1 and prev != "run" for t, prev, _ in p["tables"])
    # the expansion the drivers' rooms are sized for: 17 bytes a byte (LZH), 144 bytes per 17 (LZSS, above)
    p = P("lzh_one_bit_trees_17_bytes_a_byte")
    assert p["match_bytes"] * 8 == 17 * p["match_bits"] and p["match_bytes"] >= 6800 and all(u == {1} for u in p["used"])
    # the eight alignments of the last real token's end; a further token out of three or more spare zero bits
    for spare in range(8):
        p = P("lzh_end_with_%d_spare_bits_no_token_in_the_padding" % spare)
        assert p["spare_bits"] == spare and not p["pad_token"] and not p["left_out"]
        if spare >= 3:                 # (the shortest token there is takes three bits)
            p = P("lzh_end_with_%d_spare_bits_a_token_in_the_padding" % spare)
            assert p["spare_bits"] == spare and p["pad_token"] and not p["left_out"]
    assert P("lzh_one_bit_trees_17_bytes_a_byte")["left_out"] > 0       # tokens in the last two bytes that the reference leaves out
    # one stream cut at every byte behind its tree header, the whole stream last
    cuts = [c for c in CASES if c.name.startswith("lzh_stream_cut_after_")]
    hdr, whole = cuts[0].props["header_bytes"], cuts[0].props["whole"]
    assert [len(c.stream) for c in cuts] == list(range(hdr, whole + 1)) and whole - hdr >= 100
    assert all(c.stream == cuts[-1].stream[:len(c.stream)] for c in cuts) and len({c.out_len for c in cuts}) > 10
    assert [c.props.get("ref_undefined", False) for c in CASES if c.name.startswith("lzh_header_cut_after_")][:4] == [False] * 3 + [True]
    # rooms: ample, exact, one less, inside a match, none
    for c in Z.values():
        if c.err == 0 and c.out_len:
            assert c.rooms[0] > c.out_len and {c.out_len, c.out_len - 1, 0} <= set(c.rooms), c.name
    # every valid case whose output holds a match has a room that ends inside one, and no other case can
    n_in = 0
    for c in Z.values():
        inside = {x for x in c.props.get("in_match", ()) if 0 < x < c.out_len}
        assert (c.err == 0 and bool(inside)) == any(r in inside for r in c.rooms), c.name
        n_in += bool(inside)
    assert n_in >= 400


# ---- the hand-built folders at the fold tasks' limits (CS.fold_cases(): not part of all_cases()) ----
FOLD = CS.fold_cases()
FRAME = CS.FRAME


@pytest.mark.parametrize("c", FOLD, ids=[c.name for c in FOLD])
def test_fold_cases_through_the_oracle_and_the_reference(built, c):
    """err and out_len of oracle and reference are equal and the bytes are the case's own plaintext: a case is only worth anything
    if the reference accepts it (or rejects it with the code the case states)"""
    e, o, r = run_oracle(c)
    assert e == c.err, (e, c.err)
    if c.plain is not None:
        assert e == 0 and r.out_len == c.out_len == len(c.plain)
        assert o == c.plain, "differs at byte %d" % next(k for k in range(len(o)) if o[k] != c.plain[k])
    if have_ref():
        re, ro, rw = ref_lzx(c.stream, c.out_len, c.wb, c.reset) if c.codec == "lzx" else ref_mszip(c.stream, c.out_len)
        assert re == e and rw == r.out_len and ro == o[:rw], (re, e, rw, r.out_len)


def fold_frame_matches(c):
    """per frame / block: [(position in it, length, offset)]"""
    if c.codec == "mszip":
        return dict(enumerate(c.props["matches"]))
    per = {}
    for p, n, off in c.props["matches"]:
        per.setdefault(p // FRAME, []).append((p % FRAME, n, off))
    return per


def fold_chain_depth(ms, size=FRAME):
    """the longest chain of copies inside one frame: links from a byte to the literal, or the byte below the frame, it comes from"""
    depth = [0] * size
    for p, n, off in ms:
        for b in range(p, p + n):
            depth[b] = depth[b - off] + 1 if b - off >= 0 else 0
    return max(depth)


def test_fold_cases_have_the_property_they_name():
    """measured on what the builders wrote, not declared: record counts, the deepest chain, the classes of source distance"""
    assert len({c.name for c in FOLD}) == len(FOLD) >= 28
    assert not {c.name for c in FOLD} & {c.name for c in CASES}
    assert all((c.folds is None) == c.name.startswith("fold_lzx_pool_runs_dry_") for c in FOLD)
    assert all(c.out_len <= 8 * FRAME + 1000 for c in FOLD)
    F = {c.name: c for c in FOLD}
    for c in FOLD:
        per, x = fold_frame_matches(c), c.props["expect"]
        for f, n in x.get("records", {}).items():
            assert len(per.get(f, [])) == n, (c.name, f, len(per.get(f, [])), n)
        for f, n in x.get("depth_min", {}).items():
            assert fold_chain_depth(per[f]) >= n, (c.name, f, fold_chain_depth(per[f]), n)
        for f, classes in x.get("below", {}).items():
            got = {off - p for p, n, off in per[f] if off > p}              # how far below the frame's base a match begins
            assert set(classes) <= got, (c.name, f, sorted(set(classes) - got))
            lens = {(off - p, n) for p, n, off in per[f]}
            assert all((d, n) in lens for d in classes for n in ((2, 3, 258) if f < 7 else (2, 3))), (c.name, f)
    g = F["fold_lzx_gather_step_boundaries"]
    for f in range(3, 7):
        assert {1, 2, 32767, 32768, 32769, 65535, 65536, 65537, 98304, f * FRAME} <= set(g.props["expect"]["below"][f])
        ms = fold_frame_matches(g)[f]
        assert ms[0][:2] == (0, 258) and ms[0][2] in (1, 2)                 # root below the frame, the rest an in-frame chain
        assert {p for p, _n, _o in ms} & {4095, 4096, 4097} and max(p + n for p, n, _o in ms) == FRAME
        # one match whose source bytes lie in two frames: f-3 / f-2 and f-2 / f-1
        assert any(off - p > 65536 > off - p - n for p, n, off in ms) and any(off - p > 32768 > off - p - n for p, n, off in ms)
    assert fold_chain_depth(fold_frame_matches(F["fold_lzx_pointer_chains"])[1]) == 32767
    # every hop of frame 5's chain crosses a wave share; frame 6 copies the frame's first 128 bytes from its last share
    pc = fold_frame_matches(F["fold_lzx_pointer_chains"])
    assert all(off == 4097 for _p, _n, off in pc[5]) and all(p >= 7 * 4096 and p - off + n <= 128 for p, n, off in pc[6])
    for name in ("fold_lzx_placeholders", "fold_lzx_placeholders_reset_2"):
        c = F[name]
        reps = {p for p, _k, _v in c.props["reps"]}
        first_is_rep = [f for f, ms in sorted(fold_frame_matches(c).items()) if f * FRAME + ms[0][0] in reps]
        firsts = [f for f in range(8) if f == 0 or (c.reset and f % c.reset == 0)]
        assert [f for f in first_is_rep if f not in firsts] == c.props["expect"]["placeholder_frames"], (name, first_is_rep)
        orders = {tuple(k for p, k, _v in c.props["reps"] if p // FRAME == f)[:3] for f in c.props["expect"]["placeholder_frames"]}
        assert len(orders) == (6 if not c.reset else 4), (name, orders)
        if c.reset:
            assert all(f * FRAME in reps for f in firsts[1:])               # a repeat right behind every reset: it reaches below it
        else:
            assert 1 not in fold_frame_matches(c)                           # a frame without a match
            assert all(f * FRAME + p in reps for f in range(2, 7) for p, _n, _o in fold_frame_matches(c)[f])   # repeats only
    for name in ("fold_lzx_pool_runs_dry_offset_32768", "fold_lzx_pool_runs_dry_rep0"):
        per = fold_frame_matches(F[name])
        need = sum((len(ms) + CS.REC_CHUNK - 1) // CS.REC_CHUNK for ms in per.values())
        assert need == 113 > CS.REC_POOL_PER_SLOT * 9 and all(n == 2 for ms in per.values() if len(ms) > 100 for _p, n, _o in ms)
    for wb in (15, 16):
        offs = {off for _p, _n, off in F["fold_lzx_window_wrap_w%d" % wb].props["matches"]}
        assert {(1 << wb) - 3, (1 << wb) - 4} <= offs and max(offs) == (1 << wb) - 3
    for t in (1, 2, 255, 256, 257, 2049):
        c = F["fold_lzx_short_last_frame_%d" % t]
        ms = fold_frame_matches(c).get(4, [])
        assert c.out_len == 4 * FRAME + t and sum(n for _p, n, _o in ms) >= t - 1
        assert t == 1 or ({(off - p + FRAME - 1) // FRAME for p, _n, off in ms} == ({1, 3} if t > 2 else {1}))
    z = F["fold_mszip_distances_at_the_block_edges"]
    assert z.props["max_dist"] == 32768
    per = fold_frame_matches(z)
    assert all(any(d == q + 1 for q, _n, d in per[b]) for b in (1, 2, 3)) and per[2][0] == (0, 258, 1)
    assert {q for b in (1, 2, 3) for q, _n, d in per[b] if d == 32768} >= {0, 1, 4096, FRAME - 3, FRAME - 258}
    sizes = F["fold_mszip_short_block_in_the_middle"].props["expect"]["sizes"]
    assert sizes[2] == 20000 and len(F["fold_mszip_short_block_in_the_middle"].plain) == sum(sizes)
    assert F["fold_mszip_stored_block_in_the_middle"].props["stored_lens"] == [FRAME]


# the emulator run leaves out (at most two, by name): minutes each there, milliseconds on the GPU, which leaves out none
EMU_LEAVES_OUT = ("qtm_literal_length_position_models_alternating_w10", "qtm_literal_length_position_models_alternating_w17")

EMU_WORKER = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
import libmspack_amd as M
import test_gpu_crafted as G
assert "emu" in M.HIP_SO
G.check_all([c for c in G.CS.all_cases() if c.name not in %r])
print("EMU_CRAFTED_OK")
'''


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"), reason="the emulator build needs ROCm's clang++")
def test_crafted_streams_on_the_wavefront_emulator(built, tmp_path):
    """(wall time of the call: 283 s with the LZSS and LZH cases, which take some 110 s when they run alone; the time before them was not
    measured on its own -- about 170 s by that difference)"""
    so = emu_so()                  # (rebuilt when a kernel source is newer: the run must see the kernels as they are)
    script = tmp_path / "w.py"
    script.write_text(EMU_WORKER % (ROOT, ROOT, EMU_LEAVES_OUT))
    env = dict(os.environ, MSPACK_HIP_SO=so)
    p = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=3000)
    assert p.returncode == 0 and b"EMU_CRAFTED_OK" in p.stdout, p.stdout.decode()[-3000:]


# ---- MSZIP window history at any depth, KWAJ framing (CS.mszip_history_cases, CS.kwaj_mszip_cases) ----------------------
HISTORY = CS.mszip_history_cases()
KWAJ_MSZIP = CS.kwaj_mszip_cases()


def run_history_oracle(c):
    """-> (err, bytes, result) of the oracle for a history / KWAJ case as the unit is given to the kernels"""
    from helpers import oracle_mszip_kwaj, oracle_set_hard_eof
    if c.codec == "kwaj_mszip":
        oracle_set_hard_eof(bool(c.props["uflags"] & CS.UF_HARD_EOF))
        try:
            return oracle_mszip_kwaj(c.stream, c.out_len)
        finally:
            oracle_set_hard_eof(0)
    repair = (c.props["in_chunk"] or 1) if c.props["uflags"] & CS.UF_MSZIP_REPAIR else 0
    return oracle_mszip(c.stream, c.out_len, repair)[:3]


def test_history_case_lists():
    names = [c.name for c in HISTORY + KWAJ_MSZIP]
    assert len(set(names)) == len(names) and not set(names) & {c.name for c in CASES}
    for c in HISTORY + KWAJ_MSZIP:
        assert len(c.props["blocks"]) <= 45 and sum(c.props["blocks"]) <= 1536 * 1024, c.name
        # window bytes no frame wrote (the reference reads uninitialised memory there): the two named streams only
        assert bool(c.props.get("never_written_reads")) == c.props["never"] == any(n in c.name for n in CS.NEVER_WRITTEN), c.name
    for depth in (2, 7, 8, 9, 12, 40):
        for head in ("mszip_history_", "kwaj_mszip_history_"):
            c = next(c for c in HISTORY + KWAJ_MSZIP if c.name == head + "shrinking_chain_depth_%d" % depth)
            chain = c.props["blocks"][:-1]
            assert len(chain) == depth and all(a > b for a, b in zip(chain, chain[1:])), c.name
    assert sum("deep" in c.name or "depth" in c.name for c in HISTORY) >= 20 and CS.ZIP_HIST == 8


@pytest.mark.parametrize("c", HISTORY + KWAJ_MSZIP, ids=[c.name for c in HISTORY + KWAJ_MSZIP])
def test_history_model_equals_the_oracle(built, c):
    """error, flags, bytes written, in_next and every byte: the generator's own ring against the oracle's"""
    e, o, r = run_history_oracle(c)
    assert e == c.err and r.out_len == c.props["written"] == len(c.plain), (e, c.err, r.out_len, c.props["written"])
    assert r.in_next == c.props["in_next"] and r.flags == c.props.get("rflags", 0), (r.in_next, r.flags)
    assert o == c.plain, "differs at byte %d" % next(k for k in range(len(o)) if o[k] != c.plain[k])
