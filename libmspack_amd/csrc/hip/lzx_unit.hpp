// lzx_unit.hpp -- LZX unit decoder: one wavefront per CAB folder / CHM reset interval / OAB block, and the E8 pass.
// Compiled into lzxn and lzxd; LZX_DELTA marks the lines where the two differ (the plain build also adopts the frames the
// frame-parallel path finished).  Replaces, for one unit, lzxd_init + lzxd_decompress(out_len) of the reference
// (lzxd.c:274-346, 388-771) with bit-exact output and error code:
//   frame logic ....... lzxd.c:419-466, 677-697, 749-754
//   main decode loop .. lzxd.c:538-651 -> the speculative runs (lzx_run_*.hpp); the loop here is the EOF-exact scalar
//                       version (last bytes of the input, DELTA's extended lengths): it gathers literals 64 at a time into
//                       one coalesced store
//   E8 translation .... lzxd.c:706-736 -> NOT done while decoding: the window must keep untranslated bytes
//                       and our window IS the output, so the decode kernel only records, per frame,
//                       the intel_filesize to apply; a second, frame-parallel kernel translates (lzx_e8_frame).
// decode one LZX unit.  frame_meta[frame_base + f] receives the intel_filesize to apply to frame f
// (0 = none).  Returns via *res.
#ifdef LZX_DELTA
__device__ __forceinline__ void lzx_decode_unit(const mspack_hip_unit &u, const u8 *in_arena, u8 *out_arena,
                                int32_t *frame_meta, mspack_hip_result *res, LzxShared *sh)
#else
// recs: the pipe's frame records for this launch (NULL: none), indexed by frame slot; toks: its record pool (not read here)
// resume: the launch ran mspack_lzx_pipe first -- the unit's first record says how far its commit task got (rs_*: so many
// complete frames, possibly part of the next one).  Those frames are not decoded again: only their bookkeeping (interval
// header, E8 decision, offsets, in_next) is replayed from their records, and decoding goes on serially where the pipe stopped
__device__ __forceinline__ void lzx_decode_unit(const mspack_hip_unit &u, const u8 *in_arena, u8 *out_arena,
                                int32_t *frame_meta, mspack_hip_result *res, LzxShared *sh,
                                const LzxFrameRec *recs, const uint2 *toks, const bool resume = false)
#endif
{
  const u32 lane = threadIdx.x;
  LzxDec d;
  LzxState s;
  u32 flags = 0;
  const u32 out_bytes = u.out_len;
  u32 remaining = out_bytes;
  u32 in_next = 0;

  d.lane = lane; d.sh = sh; d.err = 0;
  d.w.unit = in_arena + u.in_off; d.w.in_len = u.in_len;
  d.w.eofs = (u.flags & MSPACK_HIP_UF_HARD_EOF) ? 0u : 2u;
  d.w.seek(0, lane);
  d.bb = 0; d.bl = 0; d.rbl = 0;
  d.near_end = (u.in_len <= 64u); d.careful = d.near_end;
#ifdef LZX_DELTA
  // reference data lies right below the unit's output; positions are biased by its size
  d.out = out_arena + u.out_off - u.ref_len; d.P = u.ref_len;
#else
  d.out = out_arena + u.out_off; d.P = 0;
#endif
  d.lit_buf = 0; d.lit_n = 0;
  d.st_rounds = 0;
  // (only trace builds of the parse task read st_t, but this loop shapes the shipped kernels: without it mspack_decode_lzx comes
  // out 619 lines of assembly longer and mspack_decode_lzxd 473 -- tools/isa_diff.sh)
  for (int k_ = 0; k_ < 10; k_++) d.st_t[k_] = 0;

  s.wsize = 1u << u.window_bits;
  s.wpos = 0; s.frame_posn = 0; s.frame = 0; s.reset_frames = u.reset_frames;
  s.offset = 0; s.length = out_bytes;
  s.intel_filesize = 0; s.intel_started = false; s.length_empty = false;
  s.raw_mode = false; s.raw_pos = 0;
  {
    static const u16 slots[11] = { 30, 32, 34, 36, 38, 42, 50, 66, 98, 162, 290 };
    u32 wb = u.window_bits;
#ifdef LZX_DELTA
    s.ref_size = u.ref_len;
    s.num_offsets = (wb >= 17u && wb <= 25u && u.ref_len <= (1u << wb)) ? ((u32) slots[wb - 15u] << 3) : 0u;
#else
    s.ref_size = 0;
    s.num_offsets = (wb >= 15u && wb <= 21u) ? ((u32) slots[wb - 15u] << 3) : 0u;
#endif
  }
  if (s.num_offsets == 0u) {
    if (lane == 0) {
      res->err = ERR_ARGS; res->flags = 0; res->out_len = 0; res->in_used = 0; res->good_len = 0; res->in_next = 0;
#ifndef LZX_DELTA
      if (u.flags & MSPACK_HIP_UF_LZX_LOG) *(u32 *)(out_arena + u.out_off + (((size_t) u.out_len + LZX_FRAME + 15u) & ~(size_t) 15u)) = 0u;
#endif
    }
    return;
  }
  lzx_reset_state(d, s);

#ifndef LZX_DELTA
  const bool use_recs = recs != nullptr && (u.flags & MSPACK_HIP_UF_FRAME_TABLE) != 0u;
  const LzxFrameRec *stale = nullptr;       // adopted record whose code lengths / tables are not in LDS (yet)
  bool stale_tables = false;
  // where mspack_lzx_pipe's commit task stopped (resume): rs_frame complete frames, then possibly part of frame rs_frame
  bool rs_on = false, rs_partial = false, rs_inject = false, positioned = true;
  u32 rs_frame = 0, rs_P = 0, rs_next = 0, rs_R0 = 1, rs_R1 = 1, rs_R2 = 1, ff_end = 0;
  if (resume && use_recs) {
    const LzxFrameRec *r0 = &recs[u.frame_base];
    if (rfl(r0->rs_valid) == 1u) {
      rs_on = true; positioned = false;
      rs_frame = rfl(r0->rs_frame); rs_partial = rfl(r0->rs_partial) != 0u; rs_P = rfl(r0->rs_P); rs_next = rfl(r0->rs_next_bit);
      rs_R0 = rfl(r0->rs_R0); rs_R1 = rfl(r0->rs_R1); rs_R2 = rfl(r0->rs_R2);
    }
  }
#endif
#ifndef LZX_DELTA
  u32 *const olog = (u32 *)(out_arena + u.out_off + (((size_t) u.out_len + LZX_FRAME + 15u) & ~(size_t) 15u));
  u32 n_open_resets = 0;
#endif
  if (out_bytes != 0u) {
    const u32 end_frame = out_bytes / LZX_FRAME + 1u;                      // lzxd.c:419
    while (s.frame < end_frame) {
      if (s.reset_frames && (s.frame % s.reset_frames) == 0u) {
#ifndef LZX_DELTA
        // a block that is still open at a reset point: a format error the reference warns about and decodes through
        // (lzxd.c:423-431); MSPACK_HIP_UF_LZX_LOG: the frame goes into the unit's log for the driver's sys->message
        if (s.block_remaining != 0u && (u.flags & MSPACK_HIP_UF_LZX_LOG) != 0u) {
          if (d.lane == 0 && n_open_resets < u.ref_len) olog[1u + n_open_resets] = s.frame;
          n_open_resets++;
        }
#endif
        // a reset in raw mode keeps reading bits from raw_pos (no pad byte: block_type is cleared)
        lzx_reset_state(d, s);
#ifndef LZX_DELTA
        stale = nullptr; stale_tables = false;
#endif
      }
#ifndef LZX_DELTA
      const bool ff = rs_on && s.frame < rs_frame;                   // done by the pipe: bookkeeping only
      const bool pf = rs_on && s.frame == rs_frame && rs_partial;    // partly done: go on behind its last record
      const LzxFrameRec *frec = (ff || pf) ? &recs[u.frame_base + s.frame] : nullptr;
      if (rs_on && s.frame == rs_frame && !rs_partial) {
        // serial decoding starts with this frame: the state the pipe left at its first bit
        lzx_seek_bit(d, rs_next);
        d.P = rs_P; s.R0 = rs_R0; s.R1 = rs_R1; s.R2 = rs_R2;
        if (rs_frame != 0u && !(s.reset_frames && (s.frame % s.reset_frames) == 0u)) {
          stale = &recs[u.frame_base + rs_frame - 1u];
          stale_tables = s.block_remaining != 0u;                  // inside a block the pipe's frames left open: its tables too
        }
        rs_on = false; positioned = true;
      }
#endif
#ifdef LZX_DELTA
      {                                                               // chunk size (lzxd.c:440-444)
        u32 cs;
        if (s.raw_mode) {
          // inside a stored block the bit buffer is empty: ENSURE_BITS(16) reads two bytes, REMOVE drops them
          if (s.raw_pos + 2u > d.w.in_len + d.w.eofs) { d.err = ERR_READ; break; }
          s.raw_pos += 2u;
        }
        else if (!d.read_bits(16, cs)) break;
      }
#endif
      if (!s.header_read) {
        u32 v, hi = 0, lo = 0;
#ifndef LZX_DELTA
        if (frec) { const u32 iv = rfl(frec->intel_filesize); hi = iv >> 16; lo = iv & 0xFFFFu; }   // (its parse wave read the bits)
        else
#endif
        {
          lzx_leave_raw(d, s);
          if (!d.read_bits(1, v)) break;
          if (v) { if (!d.read_bits(16, hi) || !d.read_bits(16, lo)) break; }
        }
        s.intel_filesize = (int32_t)((hi << 16) | lo);
        if (s.intel_filesize) flags |= MSPACK_HIP_F_INTEL_HEADER;
        s.header_read = true;
      }
      u32 frame_size = LZX_FRAME;
      if (s.length && (s.length - s.offset) < frame_size) frame_size = s.length - s.offset;

      int todo = (int)(s.frame_posn + frame_size - s.wpos);
      bool fail = false;
#ifndef LZX_DELTA
      if (ff) {
        // a frame the pipe finished, decoded and in place: the block it ends in and what is left of that block
        s.block_type = rfl(frec->block_type); s.block_length = rfl(frec->block_length); s.block_remaining = rfl(frec->rem_out);
        const u32 rfl_ = rfl(frec->flags);
        s.length_empty = (rfl_ & 1u) != 0u;
        if (rfl_ & 2u) s.intel_started = true;
        flags |= MSPACK_HIP_F_FRAMES_ADOPTED;
        d.P += frame_size; s.wpos += frame_size;
        ff_end = (rfl(frec->end_bit) + 15u) & ~15u;                  // behind the 16-bit realignment (lzxd.c:695-697)
        todo = 0;
      }
      if (pf) {
        // (the block the record ends in, counted as if it had begun with the frame: the loop below takes the frame's bytes off it)
        s.block_type = rfl(frec->block_type);
        s.block_length = rfl(frec->block_length); s.block_remaining = rfl(frec->run_rem);
        const u32 rfl_ = rfl(frec->flags);
        s.length_empty = (rfl_ & 1u) != 0u;
        if (rfl_ & 2u) s.intel_started = true;
        stale = frec; stale_tables = true;
        flags |= MSPACK_HIP_F_FRAMES_ADOPTED;
        rs_inject = true; rs_on = false;
      }
#endif
      while (todo > 0) {
#ifndef LZX_DELTA
        if (s.block_remaining == 0u && stale) { lzx_restore_lens(d, stale); stale = nullptr; stale_tables = false; }
#endif
        if (s.block_remaining == 0u) { if (!lzx_block_header(d, s)) { fail = true; break; } }
        int run = (int) s.block_remaining;
        if (run > todo) run = todo;
        todo -= run; s.block_remaining -= (u32) run;

        if (s.block_type == 1u || s.block_type == 2u) {
          // ---------------- the hot loop (lzxd.c:538-651) ----------------
          const bool aligned = (s.block_type == 2u);
          const u32 run_end = d.P + (u32) run;
          const u32 wbase = d.P - s.wpos;          // linear position of window index 0
          bool respec = true;                      // try the speculative path (again)
#ifndef LZX_DELTA
          if (rs_inject) {
            // the pipe committed this frame's records up to rs_P: go on from the bit behind the last of them
            rs_inject = false; positioned = true;
            d.flush_lits();
            d.P = rs_P; s.R0 = rs_R0; s.R1 = rs_R1; s.R2 = rs_R2;
            lzx_seek_bit(d, rs_next);
          }
          if (!fail && d.P < run_end && stale_tables) {      // the record did not reach the end of the run
            if (stale) { lzx_restore_lens(d, stale); stale = nullptr; }
            lzx_restore_tables(d, s); stale_tables = false;
          }
          if (fail) break;
#endif
          while (d.P < run_end) {
            if (respec && !d.careful && !d.near_end) {
#ifndef LZX_DELTA
              int rc = aligned ? lzx_run_spec2<true>(d, s, run_end, wbase) : lzx_run_spec2<false>(d, s, run_end, wbase);
#else
              int rc = aligned ? lzx_run_spec<true>(d, s, run_end, wbase) : lzx_run_spec<false>(d, s, run_end, wbase);
#endif
              if (rc == LZX_RUN_FAIL) { fail = true; break; }
              if (d.P >= run_end) break;
            }
#ifdef LZX_DELTA
            respec = true;                           // it hands single tokens over (extended match lengths)
#else
            respec = false;
#endif
            if (d.bl <= 32) d.refill();
            int sym = d.decode_sym<LZX_MAIN_P, LZX_MSH, LZX_MTAB_T>(sh->main_tab, sh->main_sorted, d.hr_main);
            if (sym < 0) { fail = true; break; }
            if (sym < 256) {
              d.lit_buf = wrl(d.lit_buf, (u32) sym, d.lit_n);
              d.lit_n++; d.P++;
              if (d.lit_n == WAVE) d.flush_lits();
              continue;
            }
            u32 m = (u32) sym - 256u, slot = m >> 3, len = m & 7u, off;
            if (len == 7u) {
              if (s.length_empty) { d.err = ERR_DECRUNCH; fail = true; break; }
              int foot = d.decode_sym<LZX_LEN_P>(sh->len_tab, sh->len_sorted, d.hr_len);
              if (foot < 0) { fail = true; break; }
              len += (u32) foot;
            }
            len += 2u;
            if (slot == 0u) off = s.R0;
            else if (slot == 1u) { off = s.R1; s.R1 = s.R0; s.R0 = off; }
            else if (slot == 2u) { off = s.R2; s.R2 = s.R0; s.R0 = off; }
            else {
              // position_base / extra_bits from their closed form (lzxd.c:202-207)
              u32 extra = slot < 4u ? 0u : (slot < 36u ? (slot >> 1) - 1u : 17u);
              u32 base = slot < 4u ? slot : (slot < 36u ? ((2u + (slot & 1u)) << extra) : ((slot - 34u) << 17));
              off = base - 2u;
              if (d.bl <= 32) d.refill();
              if (extra >= 3u && aligned) {
                if (extra > 3u) { u32 vb; if (!d.read_bits((int) extra - 3, vb)) { fail = true; break; } off += vb << 3; }
                int a = d.decode_sym<LZX_ALI_P>(sh->ali_tab, sh->ali_sorted, d.hr_ali);
                if (a < 0) { fail = true; break; }
                off += (u32) a;
              }
              else if (extra) { u32 vb; if (!d.read_bits((int) extra, vb)) { fail = true; break; } off += vb; }
              s.R2 = s.R1; s.R1 = s.R0; s.R0 = off;
            }
#ifdef LZX_DELTA
            if (len == 257u) {                                          // lzxd.c:588-611
              u32 p3, x;
              if (d.bl <= 32) d.refill();
              if (d.careful && !d.ref_ensure(3)) { fail = true; break; }
              p3 = (u32)(d.bb >> 61);
              if ((p3 & 4u) == 0u)      { d.drop(1); if (!d.read_bits(8, x)) { fail = true; break; } }
              else if ((p3 >> 1) == 2u) { d.drop(2); if (!d.read_bits(10, x)) { fail = true; break; } x += 0x100u; }
              else if (p3 == 6u)        { d.drop(3); if (!d.read_bits(12, x)) { fail = true; break; } x += 0x500u; }
              else                      { d.drop(3); if (!d.read_bits(15, x)) { fail = true; break; } }
              len += x;
            }
#endif
            u32 wp = d.P - wbase;
            // a match running past the run is an error in every case (lzxd.c:678-693); test it
            // before copying so that nothing is ever written past the unit's output
            if (d.P + len > run_end) { d.err = ERR_DECRUNCH; fail = true; break; }
            if (wp + len > s.wsize) { d.err = ERR_DECRUNCH; fail = true; break; }       // lzxd.c:613
            if (LZX_BAD_SOURCE(off, wp, s.offset, s.ref_size, s.wsize)) { d.err = ERR_DECRUNCH; fail = true; break; }
            d.flush_lits();
            if (off != 0u && off <= s.wsize) lzx_copy_match(d.out, d.P, off, len, lane);
            else { if (lane == 0) lzx_copy_match_odd(d.out, d.P, wp, s.wsize, off, len); }
            d.P += len;
          }
          d.flush_lits();
          if (fail) break;
          s.wpos = d.P - wbase;
          run = (int)(run_end - d.P);              // <= 0: overrun of the last match
        }
        else if (s.block_type == 3u) {
          // stored bytes: coalesced copy input -> output (lzxd.c:654-671)
          u32 n = (u32) run;
          if (s.raw_pos + n > d.w.in_len + d.w.eofs || s.raw_pos + n < s.raw_pos) { d.err = ERR_READ; fail = true; break; }
          for (u32 i = lane; i < n; i += WAVE) d.out[d.P + i] = (u8) d.w.byte_at(s.raw_pos + i);
          s.raw_pos += n; d.P += n; s.wpos += n;
          run = 0;
        }
        else { d.err = ERR_DECRUNCH; fail = true; break; }

        if (run < 0) {                                                          // lzxd.c:678-685
          if ((u32)(-run) > s.block_remaining) { d.err = ERR_DECRUNCH; fail = true; break; }
          s.block_remaining -= (u32)(-run);
        }
      }
      if (fail) break;
      if ((s.wpos - s.frame_posn) != frame_size) { d.err = ERR_DECRUNCH; break; }  // lzxd.c:689

      // re-align the bitstream to 16 bits (lzxd.c:695-697)
#ifndef LZX_DELTA
      if (ff) {                    // (a frame the pipe finished: its record says where the stream goes on)
        in_next = ff_end >> 3;
        flags = s.block_remaining ? (flags | MSPACK_HIP_F_BLOCK_OPEN) : (flags & ~MSPACK_HIP_F_BLOCK_OPEN);
      }
      else
#endif
      {
        if (!s.raw_mode) {
          if (d.careful) { if (d.rbl > 0 && !d.ref_ensure(16)) break; }
          int n = d.bl & 15;
          if (d.bl < n) d.refill();
          if (n) d.drop(n);
        }
        if (frame_size) {            // for callers that chain units (CHM reset intervals): where the next frame starts
          in_next = s.raw_mode ? s.raw_pos : d.w.origin + (d.cons_bits() >> 3);
          flags = s.block_remaining ? (flags | MSPACK_HIP_F_BLOCK_OPEN) : (flags & ~MSPACK_HIP_F_BLOCK_OPEN);
        }
      }

      // E8: record what the translation pass must do for this frame (lzxd.c:707-708)
      {
        int32_t fs = 0;
        if (s.intel_started && s.intel_filesize && s.frame < 32768u && frame_size > 10u) {
          fs = s.intel_filesize; flags |= MSPACK_HIP_F_E8_APPLIED;
        }
        if (lane == 0 && frame_meta) frame_meta[u.frame_base + s.frame] = fs;
      }
      {
        u32 n = remaining < frame_size ? remaining : frame_size;
        s.offset += n; remaining -= n;
      }
      s.frame_posn += frame_size; s.frame++;
      if (s.wpos == s.wsize) s.wpos = 0;
      if (s.frame_posn == s.wsize) s.frame_posn = 0;
    }
  }
#ifndef LZX_DELTA
  if (!positioned && d.err == 0) lzx_seek_bit(d, ff_end);          // every frame came from the pipe: the reader stands behind the last one
#endif
  int err = d.err;
  if (err == 0 && remaining) err = ERR_DECRUNCH;                                  // lzxd.c:758-761
  if (err == ERR_READ && remaining == 0u) flags |= MSPACK_HIP_F_LOOKAHEAD_READ;
  if (lane == 0) {
#ifndef LZX_DELTA
    if (u.flags & MSPACK_HIP_UF_LZX_LOG) olog[0] = n_open_resets;
#endif
    res->err = err; res->flags = flags; res->out_len = s.offset; res->good_len = s.offset; res->in_next = in_next;
    res->in_used = s.raw_mode ? s.raw_pos : d.iptr();
  }
}

// E8 translation of one 32 KiB frame (lzxd.c:706-736), in place; one wavefront per frame.
// The scan is sequential in the reference (an E8 consumes the 4 following bytes, which are then not
// examined); here 64 bytes are examined at a time, candidates are found with a ballot and the
// skip rule is resolved on the 64-bit mask.
__device__ void lzx_e8_frame(u8 *frame, u32 frame_size, int32_t curpos0, int32_t filesize, u32 lane)
{
  if (frame_size <= 10u) return;
  const u32 end = frame_size - 10u;
  u32 skip_until = 0;                      // bytes below this index belong to an earlier operand
  for (u32 base = 0; base < end; base += WAVE) {
    u32 i = base + lane;
    bool cand = (i < end) && (i >= skip_until) && (frame[i] == 0xE8);
    u64 m = ballot(cand);
    u64 keep = 0;
    while (m) {
      u32 l = (u32) __ffsll((long long) m) - 1u;
      keep |= 1ull << l;
      u64 clr = (l + 5u >= 64u) ? ~0ull << l : (((1ull << 5) - 1ull) << l);
      m &= ~clr;
      skip_until = base + l + 5u;
    }
    // curpos at an accepted E8 at index i equals curpos0 + i (every byte advances it by one:
    // a skipped operand advances it by 5 for 5 bytes, lzxd.c:721,731)
    if ((keep >> lane) & 1ull) {
      int32_t curpos = curpos0 + (int32_t) i;
      int32_t abs_off = (int32_t)((u32) frame[i + 1] | ((u32) frame[i + 2] << 8) | ((u32) frame[i + 3] << 16) |
                                  ((u32) frame[i + 4] << 24));
      if (abs_off >= -curpos && abs_off < filesize) {
        int32_t rel = (abs_off >= 0) ? abs_off - curpos : abs_off + filesize;
        frame[i + 1] = (u8) rel; frame[i + 2] = (u8)(rel >> 8);
        frame[i + 3] = (u8)(rel >> 16); frame[i + 4] = (u8)(rel >> 24);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
}
