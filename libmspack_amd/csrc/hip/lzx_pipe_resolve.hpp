// lzx_pipe_resolve.hpp -- the RESOLVE task of the frame-parallel path: a frame's match records in stream order -- R0-R2
// (lzxd.c:565-586), the reference's checks (lzxd.c:613-634, 678-693), the copies (lzxd.c:636-646) through the match queue --
// and the restore of an adopted frame's code lengths and tables for the unit decoder.  Compiled into lzxn only, in front of
// lzx_unit.hpp (lzx_decode_unit calls lzx_restore_lens / lzx_restore_tables); ends with the fold tasks' half, lzx_fold.hpp.
// an adopted record's code lengths back into LDS (a later block header works on them, lzxd.c:138-183) ...
__device__ __forceinline__ void lzx_restore_lens(LzxDec &d, const LzxFrameRec *rec)
{
  LzxShared *sh = d.sh;
  for (u32 i = d.lane; i < LZX_MAIN_SYMS + 16; i += WAVE) sh->main_len[i] = rec->main_len[i];
  for (u32 i = d.lane; i < LZX_LEN_SYMS + 70; i += WAVE) sh->len_len[i] = rec->len_len[i];
  if (d.lane < 8u) sh->ali_len[d.lane] = rec->ali_len[d.lane];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}
// ... and its decode tables, when the serial path has to finish the block itself
__device__ __forceinline__ void lzx_restore_tables(LzxDec &d, LzxState &s)
{
  LzxShared *sh = d.sh;
  huff_build<LZX_MAIN_P, LZX_MSH, LZX_MTAB_T>(sh->main_len, lzx_main_build_syms(s.num_offsets), 12, sh->main_tab, sh->main_sorted,
                                               sh->cnt, d.hr_main, d.lane, false);
  const int r = huff_build<LZX_LEN_P>(sh->len_len, LZX_LEN_SYMS, 12, sh->len_tab, sh->len_sorted, sh->cnt, d.hr_len, d.lane, false);
  s.length_empty = (r == 2);
  if (s.block_type == 2u) huff_build<LZX_ALI_P>(sh->ali_len, 8, 7, sh->ali_tab, sh->ali_sorted, sh->cnt, d.hr_ali, d.lane, false);
}

// ---------------------------------------------------------------------------------------------------
// lzx_pipe_resolve -- second half of a frame's task in mspack_lzx_pipe (round 4; round 3 had one COMMIT task per unit that
// walked the unit's frames one after the other: a serial chain per unit at the end of every launch).  The wave that parsed
// frame f (lzx_pipe_parse: literals stored, one record per match) waits until frame f - 1 is complete -- its task has an
// earlier ticket, so a live wave holds it --, checks that the frame continues the unit exactly where that frame ended
// (bit position, one block of the frame's size), stores the few literals the parse left in the record, and runs down
// the match records 64 at a time: R0-R2 resolved along the list (lzxd.c:565-586; the same prefix scan as
// lzx_commit_batch), the reference's source checks (lzxd.c:613-634), the copies through the position-space resolver
// (spec_queue.hpp).  Then it publishes the frame as complete (`chain` word; R0-R2 behind its last match for the next
// frame).  The first frame that is not a complete regular one ends the unit's chain: its task leaves, in the unit's first
// record, where serial decoding has to resume (frame, output position, bit position, R0-R2) and mspack_decode_lzx
// (launched behind the pipe) skips what is done, finishes the rest -- at least the last bytes of the input, which always
// belong to the EOF-exact reader -- and reports.  A failed check discards the frame: the serial path decodes it again
// from its first bit and reports the error with the reference's code and byte count.
// All frame tasks are alike (parse + resolve, ~1 ms): a launch's waves finish together instead of waiting for the last
// units' commit chains, and in a unit of many frames the parse of frame f + k runs beside the copies of frame f.
// ---------------------------------------------------------------------------------------------------
#define LZX_CH_OPEN 0u
#define LZX_CH_DONE 1u
#define LZX_CH_ENDED 2u

// one batch of match records: every match's offset through the R0-R2 LRU (lzxd.c:565-586; cf. lzx_commit_batch) and the
// reference's checks (lzxd.c:613-634) -- offsets no linear copy serves (0, beyond the window) end the fast path too.
// Returns false when a check fails.
// the LRU half on its own: the offsets only MOVE (no arithmetic on them), so symbolic values pass through it unchanged
// (lzx_fold.hpp runs it with "R0 / R1 / R2 as they are at the frame's first byte" as placeholders)
__device__ __forceinline__ u32 lzx_lru_batch(const bool ism, const u32 lane, const u32 which, const u32 c1, u32 &R0, u32 &R1, u32 &R2)
{
  const u32 sR0 = R0, sR1 = R1, sR2 = R2;
  u32 vmoff = c1;
  const u64 k1 = ballot(ism && which == 0u);
  if (!ballot(ism && which >= 2u)) {
    const u64 below = k1 & ((1ull << lane) - 1ull);
    const u32 src = below ? 63u - (u32) __clzll((long long) below) : 0u;
    const u32 pv = (u32) __builtin_amdgcn_ds_bpermute((int)(src << 2), (int) c1);
    if (which == 1u) vmoff = below ? pv : sR0;
    if (k1) {
      u64 m = k1;
      const u32 j0 = 63u - (u32) __clzll((long long) m);
      u32 nbv = sR0, ncv = sR1;
      m &= ~(1ull << j0);
      if (m) {
        const u32 j1 = 63u - (u32) __clzll((long long) m);
        nbv = rdl(c1, j1); ncv = sR0;
        m &= ~(1ull << j1);
        if (m) ncv = rdl(c1, 63u - (u32) __clzll((long long) m));
      }
      R0 = rdl(c1, j0); R1 = nbv; R2 = ncv;
    }
  }
  else {
    u32 x = LRU_ID;
    if (ism) x = which == 0u ? (0x010080u | lane) : (which == 2u ? 0x020001u : (which == 3u ? 0x000102u : LRU_ID));
    const u32 Cm = lru_scan(x);
    const u32 e0 = Cm & 0xFFu;
    const u32 pv = (u32) __builtin_amdgcn_ds_bpermute((int)((e0 & 63u) << 2), (int) c1);
    vmoff = (e0 & 0x80u) ? pv : (e0 == 0u ? sR0 : (e0 == 1u ? sR1 : sR2));
    const u32 Cl = rdl(Cm, 63u);
    const u32 f0 = Cl & 0xFFu, f1 = (Cl >> 8) & 0xFFu, f2 = (Cl >> 16) & 0xFFu;
    R0 = (f0 & 0x80u) ? rdl(c1, f0 & 63u) : (f0 == 0u ? sR0 : (f0 == 1u ? sR1 : sR2));
    R1 = (f1 & 0x80u) ? rdl(c1, f1 & 63u) : (f1 == 0u ? sR0 : (f1 == 1u ? sR1 : sR2));
    R2 = (f2 & 0x80u) ? rdl(c1, f2 & 63u) : (f2 == 0u ? sR0 : (f2 == 1u ? sR1 : sR2));
  }
  return vmoff;
}
__device__ __forceinline__ bool lzx_front_batch(const bool ism, const u32 lane, const u32 opos, const u32 olen, const u32 which, const u32 c1,
                                                u32 &R0, u32 &R1, u32 &R2, const u32 frame_pos, const u32 wbase, const u32 wsize, u32 &vmoff_out)
{
  const u32 vmoff = lzx_lru_batch(ism, lane, which, c1, R0, R1, R2);
  vmoff_out = vmoff;
  const u32 wp = opos - wbase;
  const bool b = ism && (wp + olen > wsize || LZX_BAD_SOURCE(vmoff, wp, frame_pos, 0u, wsize) ||
                         vmoff == 0u || vmoff > wsize || vmoff > opos);
  return !ballot(b);
}

// wait until the chain word of the frame below is one of the states a caller can act on
__device__ __forceinline__ u32 lzx_chain_wait(const u32 *p, const bool)
{
  u32 ch = lzx_status_load(p);
  LZX_PIPE_WAIT_BEGIN();
  for (u32 tries = 0; ch == LZX_CH_OPEN && tries < (1u << 24); tries++) {
    __builtin_amdgcn_s_sleep(4);
    ch = lzx_status_load(p);
  }
  LZX_PIPE_WAIT_END();
  return ch;
}

union LzxResolveLds { SpecQueueLds q; };
__device__ void lzx_pipe_resolve(const mspack_hip_unit &u, const u32 f, u8 *out_arena, LzxFrameRec *urecs, const uint2 *pool_base, LzxResolveLds *rl,
                                 const bool merged)
{
  // record j of this frame (wave_common.hpp: RecPool); a batch of 64 that starts at a multiple of 64 lies in one chunk
#define MREC(j_) rec_at(pool_base, rec->chunk, (j_))
  SpecQueueLds *const spq = &rl->q;
  const u32 lane = threadIdx.x;
  u8 *const out = out_arena + u.out_off;
  const u32 rf = u.reset_frames;
  const u32 nreal = (u.out_len + LZX_FRAME - 1u) / LZX_FRAME;
  const u32 wsize = 1u << u.window_bits;
  LzxFrameRec *rec = &urecs[f];
  LzxFrameRec *pr = rec - 1;
  const bool first = rf ? (f % rf) == 0u : f == 0u;
  PHDECL();
  // ---- the frame below: complete?  (Tried in round 4: R0-R2 published as soon as a first pass over the records has
  // resolved them, so that only the copies wait for the frame below -- no gain: a 512-frame folder's chain stayed at 242 us
  // per frame, which is the copies; the first pass is 10 % of a frame's resolve.) ----
  u32 R0 = 1, R1 = 1, R2 = 1, prev_end = 0;
  u32 pch = LZX_CH_DONE;
  if (f != 0u) {
    pch = lzx_chain_wait(&pr->chain, false);
    // (the chain ended below: whoever ended it has said where the serial path resumes.  Still open after the bound: nobody
    // says anything -- no rs_valid, the unit kernel decodes the unit from its first byte)
    if (pch != LZX_CH_DONE) { lzx_status_publish(&rec->chain, LZX_CH_ENDED, lane); return; }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    prev_end = (rfl(pr->end_bit) + 15u) & ~15u;
    if (!first) { R0 = rfl(pr->cR0); R1 = rfl(pr->cR1); R2 = rfl(pr->cR2); }       // (a reset frame: lzxd.c:257-270)
  }
  // ---- this frame's record: written by this wave (`merged`: parse and resolve are one task), else by the wave that holds
  // the frame's parse task -- an earlier ticket ----
  u32 st = lzx_status_load(&rec->status);
  if (!merged) {
    LZX_PIPE_WAIT_BEGIN();
    for (u32 tries = 0; (st == LZX_ST_NONE || st == LZX_ST_CLAIMED || st == LZX_ST_HEADER) && tries < (1u << 24); tries++) {
      __builtin_amdgcn_s_sleep(8);
      st = lzx_status_load(&rec->status);
    }
    LZX_PIPE_WAIT_END();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  PH0();
  u32 fsz = u.out_len - f * LZX_FRAME; if (fsz > LZX_FRAME) fsz = LZX_FRAME;
  const u32 frame_pos = f * LZX_FRAME;
  const u32 wbase = frame_pos & ~(wsize - 1u);                 // linear position of window index 0 in this pass
  const u32 eR0 = R0, eR1 = R1, eR2 = R2;
  u32 n_rec = 0, bytes = 0, end_bit = 0;
  bool bad = st != LZX_ST_EMITTED;
  if (!bad) {
    n_rec = rfl(rec->n_tokens); bytes = rfl(rec->bytes_done); end_bit = rfl(rec->end_bit);
    // (which blocks the frame lies in is the parse tasks' chain: code lengths and what is left of the open block travel from
    // frame to frame with the records, and a record only counts when every frame below it was complete)
    bad = rfl(rec->frame_start_bit) != prev_end || bytes > fsz || n_rec > REC_CHUNK * REC_CHUNKS;
  }
  if (!bad) {
    // ---- the literals of the frame's first cache line ----
    const u32 ne = rfl(rec->n_edge);
    for (u32 i = lane; i < ne; i += WAVE)
      if ((gld(&rec->edge_mask[i >> 5]) >> (i & 31u)) & 1u) gst(out + frame_pos + i, gld(&rec->edge_lit[i]));
    // ---- the match records ----
    SpecQueue Q;
    spq_init(*spq, Q, frame_pos, lane);
    u32 th = 0;
    uint2 cur0 = make_uint2(0u, 0u), cur1 = cur0, cur2 = cur0, cur3 = cur0;
    {
      const uint2 *g0 = rec_group(pool_base, rec->chunk, 0u);     // (groups of four batches: one chunk lookup per 256 records)
      if (th + lane < n_rec) cur0 = gld(g0 + lane);
      if (th + 64u + lane < n_rec) cur1 = gld(g0 + 64u + lane);
      if (th + 128u + lane < n_rec) cur2 = gld(g0 + 128u + lane);
      if (th + 192u + lane < n_rec) cur3 = gld(g0 + 192u + lane);
    }
    for (; th < n_rec && !bad; ) {
      uint2 nx0 = make_uint2(0u, 0u), nx1 = nx0, nx2 = nx0, nx3 = nx0;
      const u32 tb = th + 256u + lane;
      if (th + 256u < n_rec) {
        const uint2 *g1 = rec_group(pool_base, rec->chunk, th + 256u);
        if (tb < n_rec) nx0 = gld(g1 + lane);
        if (tb + 64u < n_rec) nx1 = gld(g1 + 64u + lane);
        if (tb + 128u < n_rec) nx2 = gld(g1 + 128u + lane);
        if (tb + 192u < n_rec) nx3 = gld(g1 + 192u + lane);
      }
#pragma unroll 1
      for (u32 k = 0; k < 4u && th < n_rec && !bad; k++) {
        u32 n = n_rec - th; if (n > 64u) n = 64u;
        const uint2 cur = k == 0u ? cur0 : (k == 1u ? cur1 : (k == 2u ? cur2 : cur3));
        const bool ism = lane < n;
        const u32 opos = cur.x, olen = (cur.y >> 2) & 511u, which = cur.y & 3u, c1 = cur.y >> 11;
        const u64 mm = ballot(ism);
        u32 vmoff = c1;
        // (1) offsets through the R0-R2 LRU, (2) the reference's checks
        if (!lzx_front_batch(ism, lane, opos, olen, which, c1, R0, R1, R2, frame_pos, wbase, wsize, vmoff)) { bad = true; break; }
        PH(9);
        // (3) queue the copies (cf. lzx_commit_batch)
        // (runs -- matches in a row at one offset -- are written as periodic fills, the rest goes through the queue: spec_queue.hpp)
        const u32 newP = rdl(opos + olen, n - 1u);
        spq_push_runs(*spq, Q, out, ism, n, opos, olen, vmoff, lane);
        PH(10);
        if (spq_due(Q, newP)) spq_resolve(*spq, Q, out, newP, false, lane);
        PH(11);
        th += n;
      }
      cur0 = nx0; cur1 = nx1; cur2 = nx2; cur3 = nx3;
    }
    if (!bad) spq_resolve(*spq, Q, out, frame_pos + bytes, true, lane);
    PH(11);
  }
  // ---- the frame is complete: the next frame's task may go on.  Anything else ends the unit's chain here: the serial path
  // (mspack_decode_lzx) resumes at this frame's first bit, or behind its last record when only its end is missing ----
  const bool whole = !bad && bytes == fsz;
  if (lane == 0) {
    if (whole) { rec->cR0 = R0; rec->cR1 = R1; rec->cR2 = R2; }
    if (!whole || f + 1u == nreal) {
      LzxFrameRec *r0 = &urecs[0];
      const bool partial = !bad && !whole;
      r0->rs_frame = whole ? f + 1u : f; r0->rs_partial = partial ? 1u : 0u;
      r0->rs_P = whole ? (f + 1u) * LZX_FRAME : (partial ? frame_pos + bytes : frame_pos);
      r0->rs_next_bit = whole ? ((end_bit + 15u) & ~15u) : (partial ? end_bit : prev_end);
      r0->rs_R0 = bad ? eR0 : R0; r0->rs_R1 = bad ? eR1 : R1; r0->rs_R2 = bad ? eR2 : R2;
      r0->rs_valid = 1u;
    }
  }
  lzx_status_publish(&rec->chain, whole ? LZX_CH_DONE : LZX_CH_ENDED, lane);
  PHFLUSH();
#undef MREC
}
// ---------------------------------------------------------------------------------------------------
// lzx_pipe_resolve_stream -- the resolve task of a launch that has wave slots to spare (round 6; round 3's commit task had this,
// round 4's restructure dropped it, and BASELINE config 3's launch shape -- 1024 intervals: 4096 tickets for 4096 waves -- got slower
// every round since: 1.44 -> 1.58 -> 1.60 ms).  In such a launch every ticket is pulled at once, and a unit's chain is
// P(f0) -> R(f0) -> R(f1): the resolve task of a frame sat idle until the frame's parse task had stored its last record.  Here it
// takes the records up WHILE the frame is parsed: lzx_parse_emit publishes, behind every pass but the last, how many match records
// and output bytes are in memory (`prog`, with the same release recipe as a status word), and this task works through what has
// arrived -- whole groups of 256 records -- one acquire per event.  The frame's chain is then the longer of its parse and its
// resolve, not their sum.  Only where waves are spare (launch.hpp: control word 3): a resolve wave that has started on a frame
// holds its slot until the frame's parse task is through.  Same records, same checks, same hand-over as lzx_pipe_resolve.
// ---------------------------------------------------------------------------------------------------
__device__ void lzx_pipe_resolve_stream(const mspack_hip_unit &u, const u32 f, u8 *out_arena, LzxFrameRec *urecs, const uint2 *pool_base, LzxResolveLds *rl)
{
  SpecQueueLds *const spq = &rl->q;
  const u32 lane = threadIdx.x;
  u8 *const out = out_arena + u.out_off;
  const u32 rf = u.reset_frames;
  const u32 nreal = (u.out_len + LZX_FRAME - 1u) / LZX_FRAME;
  const u32 wsize = 1u << u.window_bits;
  LzxFrameRec *rec = &urecs[f];
  LzxFrameRec *pr = rec - 1;
  const bool first = rf ? (f % rf) == 0u : f == 0u;
  u32 R0 = 1, R1 = 1, R2 = 1, prev_end = 0;
  if (f != 0u) {
    const u32 pch = lzx_chain_wait(&pr->chain, false);
    if (pch != LZX_CH_DONE) { lzx_status_publish(&rec->chain, LZX_CH_ENDED, lane); return; }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    prev_end = (rfl(pr->end_bit) + 15u) & ~15u;
    if (!first) { R0 = rfl(pr->cR0); R1 = rfl(pr->cR1); R2 = rfl(pr->cR2); }
  }
  // the frame's parse task: an earlier ticket.  Its header (status HEADER: the record's first fields stand) or its end
  u32 st = lzx_status_load(&rec->status);
  for (u32 tries = 0; (st == LZX_ST_NONE || st == LZX_ST_CLAIMED) && tries < (1u << 24); tries++) {
    __builtin_amdgcn_s_sleep(8);
    st = lzx_status_load(&rec->status);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  u32 fsz = u.out_len - f * LZX_FRAME; if (fsz > LZX_FRAME) fsz = LZX_FRAME;
  const u32 frame_pos = f * LZX_FRAME;
  const u32 wbase = frame_pos & ~(wsize - 1u);
  const u32 eR0 = R0, eR1 = R1, eR2 = R2;
  u32 n_rec = 0, bytes = 0, end_bit = 0;
  bool bad = !(st == LZX_ST_EMITTED || st == LZX_ST_HEADER);
  if (!bad) bad = rfl(gld(&rec->frame_start_bit)) != prev_end;
  bool fin = false;                                          // the parse task has said its last word
  u32 avail = 0, th = 0;
  bool edge_done = false;
  SpecQueue Q;
  spq_init(*spq, Q, frame_pos, lane);
  while (!bad) {
    if (!fin) {
      st = lzx_status_load(&rec->status);
      if (st != LZX_ST_HEADER) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        fin = true;
        if (st != LZX_ST_EMITTED) { bad = true; break; }
        n_rec = rfl(gld(&rec->n_tokens)); bytes = rfl(gld(&rec->bytes_done)); end_bit = rfl(gld(&rec->end_bit));
        if (bytes > fsz || n_rec > REC_CHUNK * REC_CHUNKS || n_rec < avail) { bad = true; break; }
        avail = n_rec;
      }
      else {
        const u32 pg = lzx_status_load(&rec->prog) & 0x7FFFu;
        if (pg > avail) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); avail = pg;
#if defined(MSPACK_WAVE_EMU)
          if (lane == 0 && getenv("MSPACK_EMU_STREAM_TRACE")) fprintf(stderr, "lzx_pipe_resolve_stream: frame %u: %u records in while the frame is parsed\n", f, avail);
#endif
        }
        else if (th + 256u > avail) { __builtin_amdgcn_s_sleep(8); continue; }
      }
    }
    if (!edge_done && (fin || avail != 0u)) {
      // the literals of the frame's first cache line (their mask is complete once a pass has been published: lzx_parse_emit)
      const u32 ne = rfl(gld(&rec->n_edge));
      for (u32 i = lane; i < ne; i += WAVE)
        if ((gld(&rec->edge_mask[i >> 5]) >> (i & 31u)) & 1u) gst(out + frame_pos + i, gld(&rec->edge_lit[i]));
      edge_done = true;
    }
    // whole groups of 256 records (all that is left once the parse is through)
    while (th < avail && (fin || th + 256u <= avail) && !bad) {
      const uint2 *g0 = rec_group(pool_base, rec->chunk, th);
      uint2 c4[4];
#pragma unroll
      for (u32 k = 0; k < 4u; k++) { c4[k] = make_uint2(0u, 0u); if (th + 64u * k + lane < avail) c4[k] = gld(g0 + 64u * k + lane); }
#pragma unroll 1
      for (u32 k = 0; k < 4u && th < avail && !bad; k++) {
        u32 n = avail - th; if (n > 64u) n = 64u;
        const uint2 cur = k == 0u ? c4[0] : (k == 1u ? c4[1] : (k == 2u ? c4[2] : c4[3]));
        const bool ism = lane < n;
        const u32 opos = cur.x, olen = (cur.y >> 2) & 511u, which = cur.y & 3u, c1 = cur.y >> 11;
        u32 vmoff = c1;
        if (!lzx_front_batch(ism, lane, opos, olen, which, c1, R0, R1, R2, frame_pos, wbase, wsize, vmoff)) { bad = true; break; }
        const u32 newP = rdl(opos + olen, n - 1u);
        spq_push_runs(*spq, Q, out, ism, n, opos, olen, vmoff, lane);
        if (spq_due(Q, newP)) spq_resolve(*spq, Q, out, newP, false, lane);
        th += n;
      }
    }
    if (fin && th >= avail) break;
  }
  if (!bad) {
    if (!edge_done) {
      const u32 ne = rfl(gld(&rec->n_edge));
      for (u32 i = lane; i < ne; i += WAVE)
        if ((gld(&rec->edge_mask[i >> 5]) >> (i & 31u)) & 1u) gst(out + frame_pos + i, gld(&rec->edge_lit[i]));
    }
    spq_resolve(*spq, Q, out, frame_pos + bytes, true, lane);
  }
  const bool whole = !bad && bytes == fsz;
  if (lane == 0) {
    if (whole) { rec->cR0 = R0; rec->cR1 = R1; rec->cR2 = R2; }
    if (!whole || f + 1u == nreal) {
      LzxFrameRec *r0 = &urecs[0];
      const bool partial = !bad && !whole;
      r0->rs_frame = whole ? f + 1u : f; r0->rs_partial = partial ? 1u : 0u;
      r0->rs_P = whole ? (f + 1u) * LZX_FRAME : (partial ? frame_pos + bytes : frame_pos);
      r0->rs_next_bit = whole ? ((end_bit + 15u) & ~15u) : (partial ? end_bit : prev_end);
      r0->rs_R0 = bad ? eR0 : R0; r0->rs_R1 = bad ? eR1 : R1; r0->rs_R2 = bad ? eR2 : R2;
      r0->rs_valid = 1u;
    }
  }
  lzx_status_publish(&rec->chain, whole ? LZX_CH_DONE : LZX_CH_ENDED, lane);
}

#include "lzx_fold.hpp"
