// lzx_pipe_parse.hpp -- the PARSE task of the frame-parallel path: a frame's block headers (a chain of code lengths from frame
// to frame) and its tokens by the lane parser; literals go to the output, matches become records.  Compiled into lzxp only
// (LDS layout and 8-bit main table of LZX_PARSE_ONLY: lzx_kernel.hpp; LZX_STAGE_WORDS and LZX_LIT_RING are set in shim.hip).
// Replaces, per frame, the header reads lzxd.c:467-523 and the token decode of lzxd.c:538-611 -- without the window and R0-R2.

// ---------------------------------------------------------------------------------------------------
// The lane parser -- a frame's tokens, every lane walking its own stretch of the bit stream.
//
// The 64-positions-per-round parser (lzx_run_delta.hpp, lzx_run_plain.hpp) spends its vector instructions on 64 lanes of which
// the ~5 on the chain matter.  Here the frame's bits [B, E) -- E is what the frame table says, a hint -- are cut into 64 stretches and
// lane l walks the tokens of stretch l one after the other: length of the token at p, p += length, until p leaves
// the stretch.  Lane 0 starts at B, a real token start; the others start at their stretch's first bit, which is
// almost never one.  But a walk that starts in the middle of a token falls into step with the real chain after a
// few tokens (each landing is a real token start with probability ~1/mean token length), so its EXIT -- the first
// position beyond the stretch -- is almost always the real chain's.  Round 2: every lane starts again from its
// left neighbour's exit.  Lane l's walk is the real chain if lane l-1's was and its entry is lane l-1's exit: an
// induction from lane 0, checked after every round (entry == left exit for all lanes: done, usually after round
// 2; otherwise only the lanes whose entry moved walk again).  A last walk decodes the token VALUES and stores
// them: lane l's i-th token at (tokens of lanes < l) + i.  Nothing here depends on E being right: a wrong table
// only makes the stretches unequal.  What a lane cannot decode (a code the tables do not hold) ends the record
// there; the unit's own wave judges that token.  The input sits in LDS (LZX_STAGE_WORDS dwords per pass, halves of every dword
// swapped: a plain MSB-first bit string); all walks are LDS lookups, one token per lane per step.
// ---------------------------------------------------------------------------------------------------
#define LZX_LANE_ROUNDS 5u          /* walks before the consistent prefix is taken as it is */
#define LZX_LANE_TAIL 384u
#define LZX_SEG 8u                  /* lzx_parse_emit: tokens per segment of the balanced last walk (a power of two): a round's 64 segments
                                       cover ~1.1 KiB of output -- what the literal ring holds */

// ---------------------------------------------------------------------------------------------------
// lzx_parse_emit -- the lane parser taken one step further (mspack_lzx_pipe): the parse wave does not leave TOKENS
// for the unit's wave, it leaves the frame's LITERALS IN PLACE and a list of MATCH RECORDS.
//
// A frame starts at a known output position (f * 32 KiB), so once the lanes' stretches are consistent every lane
// knows, by a prefix sum over the stretches' output lengths, where its first token's bytes go: in its last walk it
// stores its literals straight into the output and writes one record per match (position, length, explicit offset or
// which of R0-R2 it repeats).  What is left for the unit's wave -- the part LZ77 makes serial -- is resolving R0-R2
// along the record list and copying the matches (lzx_pipe_commit): no token ever travels through memory, and the
// positions / literal stores of all frames of a unit run in parallel.
// The frame's first bytes may share a cache line with bytes another wave is writing at that moment (the end of the
// previous frame, of the previous unit): literals there (`edge_n` positions) are kept in the record and stored by the
// commit wave.  The walk stops where the frame is full (frame_size bytes), at a token that would cross its end, at a
// token the tables do not hold and 56 bytes before the end of the input (the EOF-exact reader's): bytes_done / end_bit
// say how far it got; the rest is decoded serially (mspack_decode_lzx resumes there).
// ---------------------------------------------------------------------------------------------------
template <bool ALIGNED>
__device__ __forceinline__ u32 lzx_adv_olen(const LzxShared *sh, const bool length_empty, const u32 e, const u32 e2,
                                            const u32 w0, const u32 w1, bool &unk, u32 &olen)
{
  const u32 mlen = e >> LZX_MSH, sym = e & LZX_MMASK;
  const bool is_match = sym >= 256u;
  const u32 m = sym - 256u, slot = m >> 3;
  const bool need_len = is_match && (m & 7u) == 7u;
  u32 tot = mlen;
  unk = false;
  olen = is_match ? (m & 7u) + 2u : 1u;
  if (need_len) { unk = (e2 == 0u) || length_empty; tot += e2 >> 10; olen += e2 & 1023u; }
  const int ex_ = (int)(slot >> 1) - 1;
  const u32 extra = (u32)(ex_ < 0 ? 0 : (ex_ > 17 ? 17 : ex_));
  const bool expl = is_match && slot >= 3u;
  if (ALIGNED) {
    const bool ali = extra >= 3u;
    const u32 nb = ali ? extra - 3u : extra;
    const u64 r = ((u64) w0 << 32) | w1;
    const u32 e3 = sh->ali_tab[(u32)((r << (tot + nb)) >> (64 - LZX_ALI_P))];
    if (expl) { tot += nb; if (ali) { tot += e3 >> 10; unk = unk || e3 == 0u; } }
  }
  else if (expl) tot += extra;
  return tot;
}


// ---------------------------------------------------------------------------------------------------
// lzx_build_sub -- second level of the parse waves' main-tree table.
// The direct table has 2^8 entries (LDS), and a main tree of 656 symbols has many codes of 9..16 bits: in nearly every
// step of a walk SOME lane meets one, and the lane-parallel resolve of codes beyond the table (eight limit compares, a
// ds_bpermute, a sorted-symbol lookup: ~35 instructions) ran for the whole wave.  With a second level -- per 8-bit
// prefix that starts longer codes, a sub-table indexed by the next Lmax(prefix) - 8 bits -- a long code costs one more
// LDS read and no branch.  Canonical codes: symbol i of the sorted list (length L, i-th of its length) has the code
// first(L) + (i - offs(L)); hr.fov holds first | offs << 16 per length.  Returns false (tables untouched) when the
// sub-tables do not fit LZX_SUB_CAP entries: the walks then resolve long codes the old way.
// Level-1 entry of such a prefix: 0x8000 | (sub-table bits - 1) << 11 | sub-table base.
// ---------------------------------------------------------------------------------------------------
#define LZX_SUB_CAP ((528u + LZX_MAIN_SYMS + 16u + LZX_LEN_SYMS + 70u + 8u) / 2u)
__device__ __forceinline__ bool lzx_build_sub(LzxShared *sh, const HuffRegs &hr, const u32 nsorted, const u32 lane)
{
  static_assert(LZX_MAIN_P == 8, "lzx_build_sub: 8 direct bits");
  u32 *const lmax = sh->stage;                                  // 256 words of scratch (the stage is filled later)
  for (u32 x = lane; x < 256u; x += WAVE) lmax[x] = 0u;
  u32 first[8], offs[9];                                        // lengths 9..16
#pragma unroll
  for (int l = 9; l <= 16; l++) { const u32 fo = rdl(hr.fov, (u32) l); first[l - 9] = fo & 0xFFFFu; offs[l - 9] = fo >> 16; }
  offs[8] = nsorted;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const u32 lo = offs[0];
  if (lo >= nsorted) return true;                               // no code is longer than the direct table
  // ---- the longest code under every prefix ----
  for (u32 i = lo + lane; i < nsorted; i += WAVE) {
    u32 L = 9u;
#pragma unroll
    for (int l = 10; l <= 16; l++) L += (i >= offs[l - 9]) ? 1u : 0u;
    u32 fc = first[0], of = offs[0];
#pragma unroll
    for (int l = 10; l <= 16; l++) if (L == (u32) l) { fc = first[l - 9]; of = offs[l - 9]; }
    const u32 code16 = (fc + (i - of)) << (16u - L);
    atomicMax(&lmax[(code16 >> 8) & 255u], L);
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  // ---- sub-table sizes -> bases; level-1 entries ----
  u32 total = 0;
  u32 bases[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const u32 x = (u32) r * 64u + lane;
    const u32 lm = lmax[x];
    const u32 sz = lm ? 1u << (lm - 8u) : 0u;
    const u32 inc = wave_incl_scan(sz);
    bases[r] = total + inc - sz;
    total += rdl(inc, 63u);
  }
  if (total > LZX_SUB_CAP) return false;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const u32 x = (u32) r * 64u + lane;
    const u32 lm = lmax[x];
    if (lm) { sh->main_tab[x] = (LZX_MTAB_T)(0x8000u | ((lm - 9u) << 11) | bases[r]); lmax[x] = lm | (bases[r] << 8); }
  }
  for (u32 q = lane; q < total; q += WAVE) sh->sub_tab[q] = 0;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  // ---- every long symbol fills its share of its prefix's sub-table ----
  for (u32 i = lo + lane; i < nsorted; i += WAVE) {
    u32 L = 9u;
#pragma unroll
    for (int l = 10; l <= 16; l++) L += (i >= offs[l - 9]) ? 1u : 0u;
    u32 fc = first[0], of = offs[0];
#pragma unroll
    for (int l = 10; l <= 16; l++) if (L == (u32) l) { fc = first[l - 9]; of = offs[l - 9]; }
    const u32 code16 = (fc + (i - of)) << (16u - L);
    const u32 lb = lmax[(code16 >> 8) & 255u];
    const u32 lm = lb & 255u, base = lb >> 8, sb = lm - 8u;
    const u32 start = (code16 & 255u) >> (8u - sb), cnt = 1u << (lm - L);
    const u32 ent = (u32) sh->main_sorted[i] | (L << 10);
    for (u32 r = 0; r < cnt; r++) sh->sub_tab[base + start + r] = (u16) ent;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  return true;
}

// 32 bits of the staged input (sh->stage: dwords of an MSB-first bit string) from bit p on, and the 32 behind them.
// The window is taken one bit early -- dwords ((p + 31) >> 5) - 1 and the next, shifted right by 31 - ((p + 31) & 31)
// -- so that the shift is always 0..31: one v_alignbit_b32 per word, no 64-bit shift and no special case for p % 32 == 0
// (for p == 0 the dword in front of the stage is read and shifted out entirely).
#define STAGE_BITS(p_, w0_, w1_, WANT1)                                                        \
  u32 w0_, w1_ = 0u;                                                                           \
  {                                                                                            \
    const u32 t_ = (p_) + 31u, a_ = ~t_ & 31u;                                                 \
    const u32 *q_ = sh->stage + (t_ >> 5);                                                     \
    const u32 x0_ = q_[-1], x1_ = q_[0];                                                       \
    w0_ = (u32) __builtin_amdgcn_alignbit(x0_, x1_, a_);                                       \
    if (WANT1) { const u32 x2_ = q_[1]; w1_ = (u32) __builtin_amdgcn_alignbit(x1_, x2_, a_); } \
  }


// One token at the bits (w0, w1), every lane its own: main-tree entry (codes beyond the direct table resolved for all
// lanes at once when any lane has one), length footer, offset bits, aligned-offset symbol.  Everything is computed for
// every lane and selected -- no divergent branches in the walks' loop bodies.  unk: the tables do not hold this token.
struct EmitTok { u32 tot, olen, sym, slot, off; bool is_match, expl, unk; };
template <bool ALIGNED, bool VALUES>
__device__ __forceinline__ EmitTok lzx_emit_token(const LzxShared *sh, const bool act, const bool length_empty,
                                                  const u32 *mlim, const u32 *llim, const u32 main_fov, const u32 len_fov,
                                                  const u32 w0, const u32 w1, const bool two_level)
{
  EmitTok t;
  u32 e = sh->main_tab[w0 >> (32 - LZX_MAIN_P)];
  if (two_level) {
    // (second level: always read, selected -- no branch; a direct entry's fields index some harmless slot)
    const u32 sb = ((e >> 11) & 7u) + 1u;
    u32 ix = (e & 0x7FFu) + (((w0 >> 16) & 255u) >> (8u - sb));
    ix = ix < LZX_SUB_CAP ? ix : 0u;
    const u32 e2_ = sh->sub_tab[ix];
    e = (e & 0x8000u) ? e2_ : e;
  }
  else if (ballot(act && e == 0u)) {
    const u32 pk = w0 >> 16;
    u32 ln = LZX_MAIN_P + 1u;
#pragma unroll
    for (int l = LZX_MAIN_P + 1; l <= 16; l++) ln += (pk >= mlim[l - LZX_MAIN_P - 1]) ? 1u : 0u;
    const u32 lq = ln <= 16u ? ln : 0u;
    const u32 fo = (u32) __builtin_amdgcn_ds_bpermute((int)(lq << 2), (int) main_fov);
    u32 ix = (fo >> 16) + ((pk >> (16u - lq)) - (fo & 0xFFFFu));
    ix = ix < LZX_MAIN_SYMS ? ix : 0u;
    const u32 el = (u32) sh->main_sorted[ix] | (lq << LZX_MSH);
    e = (e == 0u && lq != 0u) ? el : e;
  }
  const u32 ml = e >> LZX_MSH, sy = e & LZX_MMASK;
  const bool is_match = sy >= 256u;
  const u32 mq = sy - 256u, slot = mq >> 3, lh = mq & 7u;
  const bool foot = is_match && lh == 7u;
  const u32 wl = w0 << ml;
  u32 e2 = sh->len_tab[wl >> (32 - LZX_LEN_P)];
  if (ballot(act && foot && e2 == 0u)) {
    const u32 pk = wl >> 16;
    u32 ln = LZX_LEN_P + 1u;
#pragma unroll
    for (int l = LZX_LEN_P + 1; l <= 16; l++) ln += (pk >= llim[l - LZX_LEN_P - 1]) ? 1u : 0u;
    const u32 lq = ln <= 16u ? ln : 0u;
    const u32 fo = (u32) __builtin_amdgcn_ds_bpermute((int)(lq << 2), (int) len_fov);
    u32 ix = (fo >> 16) + ((pk >> (16u - lq)) - (fo & 0xFFFFu));
    ix = ix < 256u ? ix : 0u;
    const u32 el = (u32) sh->len_sorted[ix] | (lq << 10);
    e2 = (e2 == 0u && lq != 0u) ? el : e2;
  }
  u32 tot = ml + (foot ? e2 >> 10 : 0u);
  t.olen = is_match ? lh + 2u + (foot ? e2 & 1023u : 0u) : 1u;
  bool unk = e == 0u || (foot && (e2 == 0u || length_empty));
  const int ex_ = (int)(slot >> 1) - 1;
  const u32 extra = (u32)(ex_ < 0 ? 0 : (ex_ > 17 ? 17 : ex_));
  const bool expl = is_match && slot >= 3u;
  u32 off = 0;
  if (VALUES) off = (((slot < 36u) ? 2u + (slot & 1u) : slot - 34u) << extra) - 2u;
  // the 32 bits behind the codes read so far (tot <= 32; a shift of 32 - tot == 0 hands back w1: right for tot == 32)
  const u32 v = (u32) __builtin_amdgcn_alignbit(w0, w1, 32u - tot);
  if (ALIGNED) {
    const bool ali = extra >= 3u;
    const u32 nb = ali ? extra - 3u : extra;
    const u32 vb = nb ? v >> (32u - nb) : 0u;
    const u32 e3 = sh->ali_tab[(v << nb) >> (32 - LZX_ALI_P)];
    tot += expl ? nb + (ali ? e3 >> 10 : 0u) : 0u;
    unk = unk || (expl && ali && e3 == 0u);
    if (VALUES) off += ali ? (vb << 3) + (e3 & 1023u) : vb;
  }
  else {
    if (VALUES) off += extra ? v >> (32u - extra) : 0u;
    tot += expl ? extra : 0u;
  }
  t.tot = tot; t.sym = sy; t.slot = slot; t.off = off; t.is_match = is_match; t.expl = expl; t.unk = unk;
  return t;
}

template <bool ALIGNED>
__device__ __forceinline__ void lzx_parse_emit(LzxDec &d, const bool length_empty, const u32 start_bit, const u32 frame_end_bit,
                                               u8 *const fout, const u32 frame_pos, const u32 frame_size, const u32 edge_n,
                                               LzxFrameRec *rec, RecWriter &W, u32 &n_rec, u32 &end_bit, u32 &bytes_done,
                                               const bool two_level, const bool stream, const u32 plimit, const bool first_seg)
{
  // (between two calls for one frame the edge literals' position mask -- its LDS words are the table builder's counters -- and
  // the record writer's chunk list -- the pretree's table -- wait in the stage's last 64 words, which only a pass's look-ahead
  // uses: nothing between the calls touches them)
  // n_rec / bytes_done: in and out -- a frame that holds the end of one block and the beginning of the next is parsed in two
  // calls (lzx_pipe_parse), each with its own tables, the second one going on where the first one stopped; plimit: the frame
  // position the call may not pass (the end of its block or of the frame: a match that crosses either is the serial path's to
  // report, lzxd.c:678-693)
  LzxShared *sh = d.sh;
  const u32 lane = d.lane;
  const u32 in_limit = d.w.in_len > 56u ? (d.w.in_len - 56u) * 8u : 0u;
  const u32 Eall = frame_end_bit < in_limit ? frame_end_bit : in_limit;
  u32 mlim[16 - LZX_MAIN_P], llim[16 - LZX_LEN_P];
#pragma unroll
  for (int l = LZX_MAIN_P + 1; l <= 16; l++) mlim[l - LZX_MAIN_P - 1] = rdl(d.hr_main.limv, (u32) l);
#pragma unroll
  for (int l = LZX_LEN_P + 1; l <= 16; l++) llim[l - LZX_LEN_P - 1] = rdl(d.hr_len.limv, (u32) l);
  const u32 main_fov = d.hr_main.fov, len_fov = d.hr_len.fov;
  u32 tt = rfl(n_rec), B = rfl(start_bit), P = rfl(bytes_done);   // records written, next bit, bytes of the frame done
  bool stop = false;
  if (first_seg) { if (lane < 4u) sh->cnt[lane] = 0u; }        // the edge literals' positions (128 bits)
  else {
    if (lane < 4u) sh->cnt[lane] = sh->stage[LZX_STAGE_WORDS + REC_CHUNKS + lane];
    W.restore(sh->stage + LZX_STAGE_WORDS, lane);
  }
  // literals below this position have left the ring (a multiple of 16).  (A second call starts with the first whole row at or
  // above P: the literals in front of it are stored on their own -- the row they lie in holds the first call's bytes)
  u32 lit_flushed = first_seg ? edge_n : (((P + 15u) & ~15u) > edge_n ? ((P + 15u) & ~15u) : edge_n);

  while (!stop && B < Eall && P < plimit) {
    PHE0();
    PHCNT(3, 1u);
    // ---- stage the input from the dword that holds bit B ----
    const u32 sb_byte = (B >> 5) << 2, sb_bit = sb_byte * 8u;
    u32 E = sb_bit + LZX_STAGE_WORDS * 32u; if (E > Eall) E = Eall;
    const u32 b0 = B - sb_bit, e0 = E - sb_bit;
    d.w.origin = sb_byte;
    {
      // every chunk of the pass is requested before the first one is waited for: one memory round trip per pass
      const u32 nck = (e0 + 128u + 2047u) >> 11;               // a token that starts below e0 ends below e0 + 53
      constexpr int NCH = (int)(LZX_STAGE_WORDS / 64u) + 1;
      u32 sv[NCH];
      if ((((size_t) d.w.unit) & 3u) == 0u) {
        // dword-aligned input (sb_byte is a multiple of 4): plain loads from clamped addresses, nothing between them
        // that waits -- the chunks' loads are all in flight before the first LDS store
#pragma unroll
        for (int c = 0; c < NCH; c++) {
          const u32 o = sb_byte + (u32) c * 256u + lane * 4u;
          sv[c] = gld((const u32 *)(d.w.unit + (((u32) c < nck && o < d.w.in_len) ? o : 0u)));
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) {
          const u32 o = sb_byte + (u32) c * 256u + lane * 4u;
          u32 v = o < d.w.in_len ? sv[c] : 0u;
          const u32 rem = d.w.in_len - o;
          v = (o < d.w.in_len && rem < 4u) ? v & ((1u << (8u * rem)) - 1u) : v;
          if ((u32) c < nck) sh->stage[(u32) c * 64u + lane] = SWAP16(v);
        }
      }
      else {
#pragma unroll
        for (int c = 0; c < NCH; c++) sv[c] = (u32) c < nck ? d.w.load_chunk((u32) c, lane) : 0u;
#pragma unroll
        for (int c = 0; c < NCH; c++) if ((u32) c < nck) sh->stage[(u32) c * 64u + lane] = SWAP16(sv[c]);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    PHE(6);
    // Stretches: equal in bits, but lane 0's is only as long as the others' FIRST walk (their last LZX_LANE_TAIL bits):
    // lane 0 starts at a real token and walks its whole stretch in the first round, while the others find their exits --
    // with equal stretches that round lasted as long as a full walk.
    const u32 Lb = e0 - b0;
    u32 S = (Lb + 63u) >> 6; if (S < 64u) S = 64u;
    u32 S0 = S;
    if (S > LZX_LANE_TAIL + 64u) { S0 = LZX_LANE_TAIL; S = (Lb - S0 + 62u) / 63u; }
    const u32 nl = Lb <= S0 ? 1u : 1u + (Lb - S0 + S - 1u) / S;
    const u32 rstart = lane == 0u ? b0 : b0 + S0 + (lane - 1u) * S;
    u32 rend = rstart + (lane == 0u ? S0 : S); if (rend > e0) rend = e0;
    u32 entry = lane == 0u ? b0 : (rend > rstart + LZX_LANE_TAIL ? rend - LZX_LANE_TAIL : rstart);
    u32 n = 0, nb = 0, nmr = 0, exitp = entry, stop_at = 0;      // tokens / output bytes / matches of the stretch
    bool dead = false, changed = lane < nl;
    // checkpoints of the lane's walk, one per LZX_SEG tokens: bit position | output bytes so far << 16, and matches so far
    // (a byte each).  All walking lanes take a token per step, so the capture is a wave-uniform branch every LZX_SEG steps.
    u32 ckA1 = 0, ckA2 = 0, ckA3 = 0, ckA4 = 0, ckA5 = 0, ckA6 = 0, ckA7 = 0, ckM0 = 0, ckM1 = 0;
    for (u32 round = 0; ; ) {
      // ---- the lanes whose entry moved walk their stretch: token lengths, output lengths ----
      u32 p = entry, cnt = 0, cb = 0, cm = 0, sa = 0;
      bool dd = false;
      for (u32 it = 0; ; it++) {
        const bool act = changed && p < rend;
        if (!ballot(act)) break;
        if ((it & (LZX_SEG - 1u)) == 0u && it != 0u && it < 8u * LZX_SEG) {
          // (a lane that has stopped keeps cnt < it: its checkpoints beyond its last token are never used)
          const u32 a = p | (cb << 16), k = it / LZX_SEG;
          if (changed) {
            if (k == 1u) ckA1 = a; else if (k == 2u) ckA2 = a; else if (k == 3u) ckA3 = a; else if (k == 4u) ckA4 = a;
            else if (k == 5u) ckA5 = a; else if (k == 6u) ckA6 = a; else ckA7 = a;
            if (k <= 4u) ckM0 = (ckM0 & ~(0xFFu << (8u * (k - 1u)))) | (cm << (8u * (k - 1u)));
            else ckM1 = (ckM1 & ~(0xFFu << (8u * (k - 5u)))) | (cm << (8u * (k - 5u)));
          }
        }
        PHCNT(0, 1u);
        PHCNT(4, round >= 2u ? 1u : 0u);                   /* (steps of the walks behind the second) */
        LZX_MARK("emit_count_step_begin");
        STAGE_BITS(act ? p : 0u, w0, w1, ALIGNED)
        const EmitTok t = lzx_emit_token<ALIGNED, false>(sh, act, length_empty, mlim, llim, main_fov, len_fov, w0, w1, two_level);
        const bool ok = act && !t.unk, die = act && t.unk;
        dd = dd || die; sa = die ? p : sa;
        cnt += ok ? 1u : 0u; cb += ok ? t.olen : 0u; cm += (ok && t.is_match) ? 1u : 0u;
        p = die ? rend : p + (ok ? t.tot : 0u);
        LZX_MARK("emit_count_step_end");
      }
      if (changed) { n = cnt; nb = cb; nmr = cm; exitp = p; dead = dd; stop_at = sa; }
      round++;
      PHCNT(1, 1u);
      const u32 pe = (u32) __builtin_amdgcn_ds_bpermute((int)(((lane - 1u) & 63u) << 2), (int) exitp);
      const u32 ne = lane == 0u ? b0 : pe;
      changed = lane < nl && ne != entry;
      entry = ne;
      PHCNT(5, round >= 2u ? (u32) __popcll(ballot(changed)) : 0u);      /* (lanes that walk again behind the second walk) */
      if (!ballot(changed) || round >= LZX_LANE_ROUNDS) break;
    }
    // ---- the consistent prefix: lanes < mm ----
    u32 m = nl;
    { const u64 chm = ballot(changed); if (chm) m = (u32) __ffsll((long long) chm) - 1u; }
    u32 mm = m, dl = 0;
    bool hit = false;
    { const u64 dm = ballot(dead && lane < m); if (dm) { dl = (u32) __ffsll((long long) dm) - 1u; mm = dl + 1u; hit = true; } }
    const u32 cvb = lane < mm ? nb : 0u, cvm = lane < mm ? nmr : 0u;
    const u32 inclb = wave_incl_scan(cvb), inclm = wave_incl_scan(cvm);
    PHE(7);
    // room for this pass's match records (taken from the launch's pool, a chunk at a time): without it the frame ends here
    if (!W.ensure(tt + (mm ? rdl(inclm, mm - 1u) : 0u), lane)) { stop = true; break; }
    // ---- last walk, BALANCED: the pass's tokens are cut into segments of LZX_SEG tokens (the lanes' checkpoints) and
    // segment r * 64 + l goes to lane l in round r.  Every lane then decodes the same number of tokens per round (the
    // stretches are equal in bits, not in tokens: the longest one used to set the pace), and the 64 segments of a round
    // are NEIGHBOURS in the output and in the record list: a round writes ~2 KiB of adjacent literals and ~3 KiB of
    // adjacent records whose cache lines are complete when the round ends, instead of 64 lines per store that the
    // XCD's L2 has dropped again before the lane's next store to them arrives (traffic).
    u32 segc = lane < mm ? (n + LZX_SEG - 1u) / LZX_SEG : 0u;
    if (segc > 8u) segc = 8u;                                     // (a stretch of more than 8 segments: the last one is long)
    const u32 seginc = wave_incl_scan(segc);
    const u32 T = rdl(seginc, 63u);
    // (512 bytes of scratch: the sorted symbols are not needed once the second-level table stands
    // -- or, without one, the block header's input window: NOT the code lengths, a later header of this frame works on them)
    u8 *const owner = two_level ? (u8 *) sh->main_sorted : (u8 *) sh->inbuf;
    for (u32 q = 0; q < segc; q++) owner[seginc - segc + q] = (u8) lane;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const u32 info0 = entry | (n << 16), info1 = P + inclb - cvb, info2 = tt + inclm - cvm, info3 = (seginc - segc) | (segc << 16);
    bool have_bad = false;
    u32 bad_s = 0xFFFFu, bad_pos = 0, bad_j = 0, bad_p = 0;
    for (u32 r = 0; r * 64u < T; r++) {
      const u32 sg = r * 64u + lane;
      const bool sact = sg < T;
      const u32 o = sact ? (u32) owner[sg] : 0u, oa = o << 2;
      const u32 i0_ = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) info0), i1_ = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) info1);
      const u32 i2_ = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) info2), i3_ = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) info3);
      const u32 k = sg - (i3_ & 0xFFFFu), osegc = i3_ >> 16, on_ = i0_ >> 16;
      const u32 a1 = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckA1), a2 = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckA2);
      const u32 a3 = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckA3), a4 = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckA4);
      const u32 a5 = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckA5), a6 = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckA6);
      const u32 a7 = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckA7);
      const u32 m0_ = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckM0), m1_ = (u32) __builtin_amdgcn_ds_bpermute((int) oa, (int) ckM1);
      const u32 ca = k == 0u ? (i0_ & 0xFFFFu) : (k == 1u ? a1 : (k == 2u ? a2 : (k == 3u ? a3 : (k == 4u ? a4 : (k == 5u ? a5 : (k == 6u ? a6 : a7))))));
      const u32 cmk = k == 0u ? 0u : (k <= 4u ? (m0_ >> (8u * (k - 1u))) & 0xFFu : (m1_ >> (8u * (k - 5u))) & 0xFFu);
      const u32 ntok = sact ? (k + 1u == osegc ? on_ - k * LZX_SEG : LZX_SEG) : 0u;
      u32 p = ca & 0xFFFFu, i = 0, pos = i1_ + (k == 0u ? 0u : ca >> 16), j = i2_ + cmk;
      bool cross = false;
      for (;;) {
        const bool on = i < ntok && pos < plimit && !cross;
        if (!ballot(on)) break;
        PHCNT(2, 1u);
        LZX_MARK("emit_last_step_begin");
        STAGE_BITS(on ? p : 0u, w0, w1, true)
        const EmitTok t = lzx_emit_token<ALIGNED, true>(sh, on, length_empty, mlim, llim, main_fov, len_fov, w0, w1, two_level);
        const bool lit = on && !t.is_match;
        const bool crs = on && t.is_match && pos + t.olen > plimit;   // lzxd.c:678-693: the serial path reports it
        const bool mt = on && t.is_match && !crs;
        if (lit) {
          // (inside the ring's window: into LDS, written out row by row behind the round; a literal beyond it -- long matches
          // between the segments -- goes out on its own)
          if (pos >= edge_n) { if (pos - lit_flushed < LZX_LIT_RING) ((u8 *) sh->litring)[pos & (LZX_LIT_RING - 1u)] = (u8) t.sym; else gst_stream(fout + pos, (u8) t.sym); }
          else { gst(&rec->edge_lit[pos], (u8) t.sym); atomicOr(&sh->cnt[pos >> 5], 1u << (pos & 31u)); }
        }
        // (an offset beyond the field -- only garbage decodes to one -- is recorded as 0: never valid, lzx_pipe_commit stops there)
        if (mt) gst_record(W.at(j), make_uint2(frame_pos + pos, (t.expl ? ((t.off < (1u << 21) ? t.off : 0u) << 11) : 0u) | (t.olen << 2) |
                                                         (t.expl ? 0u : t.slot + 1u)));
        cross = cross || crs;
        const bool adv = lit || mt;
        pos += lit ? 1u : (mt ? t.olen : 0u); j += mt ? 1u : 0u;
        p += adv ? t.tot : 0u; i += adv ? 1u : 0u;
        LZX_MARK("emit_last_step_end");
      }
      if (sact && !have_bad && (i < ntok || cross)) { have_bad = true; bad_s = sg; bad_pos = pos; bad_j = j; bad_p = p; }
      {
        // The round's 64 segments are neighbours in the output: what they left in the ring goes out as whole 16-byte rows (the
        // bytes of the matches in between are whatever the ring held -- they are not final before the frame's matches are
        // copied, lzx_pipe_resolve).  Rows up to the last complete one; the rest waits for the next round.  A round that
        // outran the ring stored its far literals itself: the rows behind the window are skipped for good.
        u32 rmax = rdl(wave_incl_max(sact ? pos : 0u), 63u);
        if (rmax > frame_size) rmax = frame_size;
        if (rmax > lit_flushed) {
          const bool outran = rmax - lit_flushed > LZX_LIT_RING;
          const u32 upto = outran ? (rmax + 15u) & ~15u : rmax & ~15u;
          u32 lim = upto; if (outran) lim = lit_flushed + LZX_LIT_RING;
          if (lim > (frame_size & ~15u)) lim = frame_size & ~15u;
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          for (u32 row = lit_flushed + 16u * lane; row < lim; row += 16u * WAVE)
            gst_row((uint4 *)(fout + row), *(const uint4 *)((const u8 *) sh->litring + (row & (LZX_LIT_RING - 1u))));
          if (upto > lit_flushed) lit_flushed = upto;
        }
      }
    }
    PHE(8);
    // ---- where did this pass get to?  the first segment that was not emitted completely ends the frame ----
    u32 smin = have_bad ? bad_s : 0xFFFFu;
#pragma unroll
    for (u32 dlt = 1; dlt < WAVE; dlt <<= 1) {
      const u32 ot = (u32) __builtin_amdgcn_ds_bpermute((int)((lane ^ dlt) << 2), (int) smin);
      smin = ot < smin ? ot : smin;
    }
    smin = rfl(smin);
    if (smin != 0xFFFFu) {
      const u32 kq = smin & 63u;
      P = rdl(bad_pos, kq); tt = rdl(bad_j, kq); B = sb_bit + rdl(bad_p, kq); stop = true;
    }
    else {
      if (mm) { P += rdl(inclb, mm - 1u); tt += rdl(inclm, mm - 1u); }
      if (hit) { B = sb_bit + rdl(stop_at, dl); stop = true; }
      else if (mm == 0u) stop = true;
      else B = sb_bit + rdl(exitp, mm - 1u);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");        // the stage is rewritten by the next pass
    // Another pass follows (and the launch has wave slots to spare, `stream`): what this one stored -- literals below P,
    // match records below tt -- is published now, so that the unit's commit task works on this frame while its later passes
    // are still being parsed (lzx_pipe_commit).  The edge literals all lie in the first 128 bytes: their mask is complete
    // once P has passed them.
    if (stream && !stop && B < Eall && P < plimit && P >= 128u && tt <= 0x7FFFu) {
      if (lane < 4u) rec->edge_mask[lane] = sh->cnt[lane];
      lzx_status_publish(&rec->prog, tt | (P << 15), lane);
#ifdef MSPACK_WAVE_EMU
      if (lane == 0) emu_test_delay();                             // (emulator test hook: lets the commit task see partial progress)
#endif
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  if (P > lit_flushed && P - lit_flushed <= LZX_LIT_RING) {
    // the last rows (the frame's end, or where the parse stopped): byte by byte behind the last complete row
    const u32 full = P & ~15u;
    for (u32 row = lit_flushed + 16u * lane; row < full; row += 16u * WAVE)
      gst_row((uint4 *)(fout + row), *(const uint4 *)((const u8 *) sh->litring + (row & (LZX_LIT_RING - 1u))));
    const u32 b0 = full > lit_flushed ? full : lit_flushed;
    if (b0 + lane < P) gst(fout + b0 + lane, ((const u8 *) sh->litring)[(b0 + lane) & (LZX_LIT_RING - 1u)]);
  }
  if (lane < 4u) { const u32 em = sh->cnt[lane]; rec->edge_mask[lane] = em; sh->stage[LZX_STAGE_WORDS + REC_CHUNKS + lane] = em; }
  W.save(sh->stage + LZX_STAGE_WORDS, lane);
  n_rec = tt; end_bit = B; bytes_done = P;
}

// ---------------------------------------------------------------------------------------------------
// mspack_lzx_pipe's PARSE task: header + tokens of frame f of unit u, by one wave.
// The block headers of a reset interval are a chain (code lengths are deltas on the previous block's,
// lzxd.c:138-183): the wave takes the previous frame's lengths from that frame's record as soon as its parse wave
// has published them (status HEADER or later), reads its own header at the position the frame table states, publishes
// its lengths, and only then parses its tokens (lzx_parse_emit) -- so the chain costs one header per link, not one
// frame.  It works on guesses (one block per frame, at the table's position) and gives up silently; the serial path stays the judge.
// Waiting is safe: the task it waits for has an earlier ticket (entry_kernels.hpp), i.e. a live wave is working on it.
// ---------------------------------------------------------------------------------------------------
// the rest of a frame whose first block ended inside it: header, tables, tokens -- block by block to the frame's end.  A real
// call: frames like this are one in a few hundred, and inlined the general case's registers counted against every frame's
// parse (scratch accesses of the task 26 -> 104).  The code lengths of the block that ended are still in LDS (no second-level
// table was built over them), the record's first fields are written, `bytes_done` bytes / `n_rec` records are out.
__device__ __attribute__((noinline)) void lzx_pipe_parse_tail(const mspack_hip_unit *up, const u32 f, const u8 *in_arena, u8 *out_arena,
                                                              LzxFrameRec *urecs, const RecPool pool, LzxShared *sh)
{
  // (where lzx_pipe_parse stopped: LZX_TAIL_ARGS)
  u32 bytes_done = rfl(sh->stage[LZX_STAGE_WORDS + 32u]), n_rec = rfl(sh->stage[LZX_STAGE_WORDS + 33u]), cur_bit = rfl(sh->stage[LZX_STAGE_WORDS + 34u]);
  const u32 n_chunks = rfl(sh->stage[LZX_STAGE_WORDS + 35u]);
  const mspack_hip_unit u = *up;
  const u32 lane = threadIdx.x;
  LzxFrameRec *rec = &urecs[f];
  LzxDec d;
  LzxState s;
  lzx_side_setup(d, s, u, in_arena, sh);
  const u32 *ftab = (const u32 *)(in_arena + (size_t) u.in_chunk * 4u);
  const u32 nreal = (u.out_len + LZX_FRAME - 1u) / LZX_FRAME;
  const u32 fo = rfl(ftab[f]);
  u32 fsz = u.out_len - f * LZX_FRAME; if (fsz > LZX_FRAME) fsz = LZX_FRAME;
  u32 fe = (f + 1u < nreal) ? rfl(ftab[f + 1u]) : u.in_len;
  if (fe > u.in_len || fe <= fo) fe = u.in_len;
  u8 *const fout = out_arena + u.out_off + (size_t) f * LZX_FRAME;
  // (rounded up to a multiple of 16 FRAME positions: the literal ring leaves as 16-byte rows of position space, and a first row
  // at any other position wrapped past the ring's end -- out_off need not be a multiple of 16)
  const u32 edge_n = (((128u - (u32)((size_t) fout & 127u)) & 127u) + 15u) & ~15u;
  RecWriter W;
  W.begin(pool, (u32 *) sh->pre_tab, rec->chunk);
  W.n_chunks = n_chunks;
  bool published = false, failed = false;
  u32 rem = 0, btype = 0, end_bit = cur_bit, pub_p0 = 0, e8flag = 0;
  while (bytes_done < fsz) {
    const u32 seg_p0 = bytes_done;
    if (rem == 0u) {
      lzx_seek_bit(d, cur_bit);
      d.err = 0; s.block_type = 0;
      const bool hok = lzx_block_header(d, s, false) && !d.careful && !d.near_end;
      if (!hok || (s.block_type != 1u && s.block_type != 2u) || s.block_length == 0u) { failed = true; break; }
      rem = s.block_length; btype = s.block_type;
      if (rfl((u32) sh->main_len[0xE8]) != 0u) e8flag = 2u;       // lzxd.c:497
      cur_bit = rfl(d.w.origin) * 8u + rfl(d.cons_bits());
    }
    const u32 need = fsz - seg_p0;
    if (!published && rem >= need) {
      for (u32 i = lane; i < (LZX_MAIN_SYMS + 16) / 4u; i += WAVE) gst((u32 *) rec->main_len + i, ((const u32 *) sh->main_len)[i]);
      for (u32 i = lane; i < (LZX_LEN_SYMS + 70) / 4u; i += WAVE) gst((u32 *) rec->len_len + i, ((const u32 *) sh->len_len)[i]);
      if (lane < 8u) rec->ali_len[lane] = sh->ali_len[lane];
      pub_p0 = seg_p0;
      if (lane == 0) {
        rec->end_bit = cur_bit; rec->block_type = btype; rec->block_length = rem; rec->rem_out = rem - need;
        rec->run_rem = seg_p0 + rem;      // (the block the record may end in, counted from the frame's first byte: lzx_decode_unit)
      }
      lzx_status_publish(&rec->status, LZX_ST_HEADER, lane);
      published = true;
    }
    bool tables = true, two_level = false;
    {
      const int r = huff_build<LZX_LEN_P>(sh->len_len, LZX_LEN_SYMS, 12, sh->len_tab, sh->len_sorted, sh->cnt, d.hr_len, lane, false);
      tables = r != 1;
      s.length_empty = (r == 2);
    }
    if (tables && btype == 2u) tables = !huff_build<LZX_ALI_P>(sh->ali_len, 8, 7, sh->ali_tab, sh->ali_sorted, sh->cnt, d.hr_ali, lane, false);
    if (tables) {
      u32 nsorted = 0;
      tables = !huff_build<LZX_MAIN_P, LZX_MSH, LZX_MTAB_T>(sh->main_len, lzx_main_build_syms(s.num_offsets), 12, sh->main_tab, sh->main_sorted,
                                                            sh->cnt, d.hr_main, lane, false, &nsorted);
      if (tables && published) two_level = rfl(lzx_build_sub(sh, d.hr_main, nsorted, lane) ? 1u : 0u) != 0u;
    }
    if (!tables) { failed = !published; break; }
    const u32 plimit = seg_p0 + (rem < need ? rem : need);
    if (btype == 2u) lzx_parse_emit<true>(d, s.length_empty, cur_bit, fe * 8u, fout, f * LZX_FRAME, fsz, edge_n, rec, W, n_rec, end_bit, bytes_done, two_level, false, plimit, false);
    else lzx_parse_emit<false>(d, s.length_empty, cur_bit, fe * 8u, fout, f * LZX_FRAME, fsz, edge_n, rec, W, n_rec, end_bit, bytes_done, two_level, false, plimit, false);
    if (bytes_done < plimit) break;                               // the record ends early: the serial path goes on behind it
    rem -= plimit - seg_p0;
    cur_bit = end_bit;
  }
  // nothing to hand on (a header that is no verbatim / aligned block, tables that do not build, a record that ends in front of
  // the frame's last header): nothing of this frame is used, the chain of code lengths ends here
  if (failed || !published) { lzx_status_publish(&rec->status, LZX_ST_FAILED, lane); return; }
  // a record that ends early must end INSIDE the frame's last block, behind at least one of its tokens
  if (bytes_done < fsz && bytes_done <= pub_p0) { lzx_status_publish(&rec->status, LZX_ST_HDRONLY, lane); return; }
  if (lane == 0) {
    rec->n_tokens = n_rec; rec->end_bit = end_bit; rec->bytes_done = bytes_done;
    rec->flags = rec->flags | e8flag | (s.length_empty ? 1u : 0u);
  }
  lzx_status_publish(&rec->status, LZX_ST_EMITTED, lane);
}

// ---------------------------------------------------------------------------------------------------
// The header chain without the headers on it (round 6).  A block header's code lengths are DELTAS on the previous block's
// (lzxd.c:138-183), so a folder written one block per frame -- this build's encoder, and others' -- chains its frames' parse
// tasks: wait for the frame below, read the own header (~60 us), publish; 512 frames: 32 ms, however many waves there are
// (measured: the whole fold path behind it takes 12).  But WHERE a header's bits end and WHAT it does to the lengths do not
// depend on the lengths it is applied to: every entry comes out as (old[x] + a) mod 17, as (old[x - i] + a) mod 17 for the
// i-th follower (i <= 4) of a run of equal lengths (pretree symbol 19: the run takes its value from ITS FIRST entry's old
// length), or as a value that depends on nothing old (zero runs, and whatever is written over an earlier run's overshoot --
// lzxd.c:159: runs are not clipped).  So a task whose predecessor is not ready reads its header at once, TWICE, against two
// probe vectors -- all zeros, and 1 + (x mod 5): five neighbours all different, none zero -- and keeps, per entry, a and what
// it is relative to (the difference of the two results names it: 0 = nothing, else the probe value of the entry it came
// from); when the frame below publishes, its lengths go through that program (~2 us) instead of through a header decode.
// Whether the frame STARTS with a header is the frame below's to say (rem_out): a frame inside a block throws the
// speculation away, as does a header that does not read the same way twice.  lzx_read_lens itself is untouched -- this is
// its own function applied to two inputs.  The program lives in the input stage's room (nothing is staged before the
// frame's first parse pass): LZX_SPEC_LENS bytes a | rel << 5 (rel 7: absolute), the aligned tree's 8 lengths, then the
// block's type, its length and the bit position behind the header.
// ---------------------------------------------------------------------------------------------------
#define LZX_SPEC_LENS (LZX_MAIN_SYMS + 16u + LZX_LEN_SYMS + 70u)     /* main_len and len_len lie back to back in LDS */
static_assert(LZX_SPEC_LENS + 8u + 16u <= LZX_STAGE_WORDS * 4u, "the header program fits the input stage");
static_assert(offsetof(LzxShared, len_len) == offsetof(LzxShared, main_len) + LZX_MAIN_SYMS + 16u, "main_len and len_len are contiguous");
__device__ __attribute__((noinline)) bool lzx_pipe_spec_header(const mspack_hip_unit *up, const u32 fo, const u8 *in_arena, LzxShared *sh)
{
  const mspack_hip_unit u = *up;
  const u32 lane = threadIdx.x;
  LzxDec d;
  LzxState s;
  if (!lzx_side_setup(d, s, u, in_arena, sh)) return false;
  u8 *const lens = sh->main_len;
  u8 *const prog = (u8 *) sh->stage;
  u32 bt = 0, bl = 0, cb = 0;
  for (u32 run = 0; run < 2u; run++) {
    for (u32 x = lane; x < LZX_SPEC_LENS; x += WAVE) lens[x] = run ? (u8)(1u + x % 5u) : (u8) 0u;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    d.w.seek(fo, lane);
    d.bb = 0; d.bl = 0; d.rbl = 0; d.near_end = false; d.careful = false; d.err = 0;
    s.block_type = 0; s.raw_mode = false;
    const bool hok = lzx_block_header(d, s, false) && !d.careful && !d.near_end;
    if (!hok || (s.block_type != 1u && s.block_type != 2u) || s.block_length == 0u) return false;
    const u32 c = rfl(d.w.origin) * 8u + rfl(d.cons_bits());
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (run == 0u) {
      bt = s.block_type; bl = s.block_length; cb = c;
      for (u32 x = lane; x < LZX_SPEC_LENS; x += WAVE) prog[x] = lens[x];
      if (lane < 8u) prog[LZX_SPEC_LENS + lane] = sh->ali_len[lane];
    }
    else {
      bool bad = s.block_type != bt || s.block_length != bl || c != cb;
      for (u32 x = lane; x < LZX_SPEC_LENS; x += WAVE) {
        const u32 a = prog[x], b = lens[x];
        const u32 diff = (b + 17u - a) % 17u;                  // 0: nothing old went into it; else the probe value of the entry that did
        const u32 rel = diff == 0u ? 7u : (x % 5u + 5u - (diff - 1u)) % 5u;
        bad = bad || a > 16u || b > 16u || diff > 5u || (diff != 0u && rel > x);
        prog[x] = (u8)(a | (rel << 5));
      }
      if (ballot(bad)) return false;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  if (lane == 0) {
    u32 *w = (u32 *)(prog + ((LZX_SPEC_LENS + 8u + 3u) & ~3u));
    w[0] = bt; w[1] = bl; w[2] = cb;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  return true;
}
// the previous block's code lengths (in LDS) through the program
__device__ __forceinline__ void lzx_pipe_apply_header(LzxShared *sh, const u32 lane)
{
  u8 *const lens = sh->main_len;
  const u8 *const prog = (const u8 *) sh->stage;
  u32 nv[(LZX_SPEC_LENS + 63u) / 64u];
#pragma unroll
  for (u32 k = 0; k < (LZX_SPEC_LENS + 63u) / 64u; k++) {
    const u32 x = k * 64u + lane;
    u32 v = 0;
    if (x < LZX_SPEC_LENS) {
      const u32 p = prog[x], a = p & 31u, rel = p >> 5;
      v = rel == 7u ? a : ((u32) lens[x - rel] + a) % 17u;
    }
    nv[k] = v;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
  for (u32 k = 0; k < (LZX_SPEC_LENS + 63u) / 64u; k++) {
    const u32 x = k * 64u + lane;
    if (x < LZX_SPEC_LENS) lens[x] = (u8) nv[k];
  }
  if (lane < 8u) sh->ali_len[lane] = prog[LZX_SPEC_LENS + lane];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// Returns 1 when the frame's first block ended inside it and lzx_pipe_parse_tail has to go on (its arguments wait in the stage's
// spare words); 0 otherwise.  `spec`: the caller has read the frame's header ahead of the chain (lzx_pipe_spec_header: the
// program is in the stage).  Both are calls of the ticket loop (entry_kernels.hpp), not of this function: nested, their frames -- and the
// registers this function had to save around them -- added up in every wave's scratch allocation (324 B per lane in round 5).
#define LZX_TAIL_ARGS (LZX_STAGE_WORDS + 32u)                  /* stage words: bytes done, records, bit position, record chunks */
__device__ u32 lzx_pipe_parse(const mspack_hip_unit &u, const mspack_hip_unit *up, const u32 f, const u8 *in_arena, u8 *out_arena,
                              LzxFrameRec *urecs, const RecPool &pool, LzxShared *sh, const bool stream, const bool spec)
{
  const u32 lane = threadIdx.x;
  LzxFrameRec *rec = &urecs[f];
  {
    u32 st = 0;
    if (lane == 0) st = atomicCAS(&rec->status, LZX_ST_NONE, LZX_ST_CLAIMED);
    if (rfl(st) != LZX_ST_NONE) return 0u;                        // the unit's wave was faster: it decodes this frame itself
  }
  LzxDec d;
  LzxState s;
  if (!lzx_side_setup(d, s, u, in_arena, sh) || u.in_len >= (1u << 28)) { lzx_status_publish(&rec->status, LZX_ST_FAILED, lane); return 0u; }
  const u32 *ftab = (const u32 *)(in_arena + (size_t) u.in_chunk * 4u);
  const u32 rf = u.reset_frames;
  const u32 nreal = (u.out_len + LZX_FRAME - 1u) / LZX_FRAME;
  const bool first = rf ? (f % rf) == 0u : f == 0u;
  PHDECL();
  PH0();
  // ---- the state in front of the frame: the code lengths of the last block header and what is left of that block ----
  u32 rem = 0, btype = 0;
  if (first) lzx_reset_state(d, s);
  else {
    const LzxFrameRec *pr = rec - 1;
    u32 ps;
    // (the previous frame's task has an earlier ticket: a live wave holds it.  The bound is a safety net -- giving up means
    // this frame and the ones behind it go to the serial path, never a hang)
    for (u32 tries = 0; ; tries++) {
      ps = lzx_status_load(&pr->status);
      if (ps != LZX_ST_NONE && ps != LZX_ST_CLAIMED) break;
      if (tries >= (1u << 24)) { ps = LZX_ST_FAILED; break; }
      __builtin_amdgcn_s_sleep(8);
    }
    if (ps == LZX_ST_FAILED || ps == LZX_ST_TAKEN) { lzx_status_publish(&rec->status, LZX_ST_FAILED, lane); return 0u; }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // (1056 bytes, a dword per lane and step)
    for (u32 i = lane; i < (LZX_MAIN_SYMS + 16) / 4u; i += WAVE) ((u32 *) sh->main_len)[i] = gld((const u32 *) pr->main_len + i);
    for (u32 i = lane; i < (LZX_LEN_SYMS + 70) / 4u; i += WAVE) ((u32 *) sh->len_len)[i] = gld((const u32 *) pr->len_len + i);
    if (lane < 8u) sh->ali_len[lane] = gld(&pr->ali_len[lane]);
    rem = rfl(gld(&pr->rem_out)); btype = rfl(gld(&pr->block_type));
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  PH(0);
  // ---- where the frame table says the frame begins ----
  const u32 fo = rfl(ftab[f]);
  bool ok = !(fo >= u.in_len || u.in_len - fo <= 64u);         // the last bytes of the input belong to the EOF-exact reader
  u32 intel = 0;
  if (ok) {
    d.w.seek(fo, lane);
    d.bb = 0; d.bl = 0; d.rbl = 0; d.near_end = false; d.careful = false; d.err = 0;
    if (first) {                                                // the interval's (stream's) 1 + 32 header bits, lzxd.c:447-453
      u32 v, hi = 0, lo = 0;
      ok = d.read_bits(1, v);
      if (ok && v) ok = d.read_bits(16, hi) && d.read_bits(16, lo);
      intel = (hi << 16) | lo;
    }
  }
  if (!ok || (rem != 0u && btype != 1u && btype != 2u)) { lzx_status_publish(&rec->status, LZX_ST_FAILED, lane); return 0u; }
  u32 fsz = u.out_len - f * LZX_FRAME; if (fsz > LZX_FRAME) fsz = LZX_FRAME;
  u32 fe = (f + 1u < nreal) ? rfl(ftab[f + 1u]) : u.in_len;       // where the table says the frame ends (a hint)
  if (fe > u.in_len || fe <= fo) fe = u.in_len;
  u8 *const fout = out_arena + u.out_off + (size_t) f * LZX_FRAME;
  // the frame's first bytes up to the next 128-byte line: another wave may be writing that line (see lzx_parse_emit)
  // (rounded up to a multiple of 16 FRAME positions: the literal ring leaves as 16-byte rows of position space, and a first row
  // at any other position wrapped past the ring's end -- out_off need not be a multiple of 16)
  const u32 edge_n = (((128u - (u32)((size_t) fout & 127u)) & 127u) + 15u) & ~15u;
  // ---- the frame's first block (or what is left of the block it lies in).  Round 5: a frame need not be ONE block that begins
  // where it begins (what this build's own encoder writes, and all rounds 2-4 handled here): Microsoft's encoder writes blocks of
  // megabytes (the reference's large-files cabinets: one aligned block of 8 384 624 bytes, then the next), so a frame usually
  // lies INSIDE a block -- it inherits the previous frame's code lengths and has no header at all -- and now and then holds the
  // end of one block and the header and first tokens of the next (lzx_pipe_parse_tail).  The chain from frame to frame is "code
  // lengths + bytes left of the open block" (rem_out); it is published as soon as the LAST header of the frame has been read,
  // i.e. at once for a frame without one. ----
  u32 cur_bit = rfl(d.w.origin) * 8u + rfl(d.cons_bits());     // the frame's first block header, or its first token
  if (lane == 0) {
    // (what does not change any more goes into the record now: fewer values to carry through the parse)
    rec->hdr_start_bit = cur_bit; rec->frame_start_bit = fo * 8u; rec->intel_filesize = intel;
    rec->n_edge = edge_n < fsz ? edge_n : fsz; rec->n_tokens = 0; rec->bytes_done = 0; rec->prog = 0; rec->flags = 0;
  }
  if (rem == 0u && spec) {
    // the header was read ahead of the chain: the previous block's lengths go through its program
    lzx_pipe_apply_header(sh, lane);
    const u32 *w = (const u32 *)((const u8 *) sh->stage + ((LZX_SPEC_LENS + 8u + 3u) & ~3u));
    btype = rfl(w[0]); rem = rfl(w[1]); cur_bit = rfl(w[2]);
    s.block_type = btype; s.block_length = rem;
#if defined(MSPACK_WAVE_EMU)                                   /* emulator analysis runs: which frames took their header this way */
    if (lane == 0 && getenv("MSPACK_EMU_SPEC_TRACE")) fprintf(stderr, "lzx_pipe_parse: frame %u: header read ahead of the chain (block type %u, %u bytes)\n", f, btype, rem);
#endif
    if (lane == 0 && sh->main_len[0xE8] != 0) rec->flags = 2u;   // lzxd.c:497
  }
  else if (rem == 0u) {
    s.block_type = 0;
    const bool hok = lzx_block_header(d, s, false) && !d.careful && !d.near_end;
    if (!hok || (s.block_type != 1u && s.block_type != 2u) || s.block_length == 0u) { lzx_status_publish(&rec->status, LZX_ST_FAILED, lane); return 0u; }
    rem = s.block_length; btype = s.block_type;
    if (lane == 0 && sh->main_len[0xE8] != 0) rec->flags = 2u;   // lzxd.c:497: a block header with a code for 0xE8
    cur_bit = rfl(d.w.origin) * 8u + rfl(d.cons_bits());         // the block's first token
  }
  else s.block_type = btype;
  const bool published = rem >= fsz;
  if (published) {
    // the state behind this frame is known: the next frame's task may go on
    PH(1);
    for (u32 i = lane; i < (LZX_MAIN_SYMS + 16) / 4u; i += WAVE) gst((u32 *) rec->main_len + i, ((const u32 *) sh->main_len)[i]);
    for (u32 i = lane; i < (LZX_LEN_SYMS + 70) / 4u; i += WAVE) gst((u32 *) rec->len_len + i, ((const u32 *) sh->len_len)[i]);
    if (lane < 8u) rec->ali_len[lane] = sh->ali_len[lane];
    if (lane == 0) { rec->end_bit = cur_bit; rec->block_type = btype; rec->block_length = rem; rec->rem_out = rem - fsz; rec->run_rem = rem; }
    lzx_status_publish(&rec->status, LZX_ST_HEADER, lane);      // the next frame's wave may go on
    PH(2);
  }
  // ---- tables (cf. lzx_parse_frame): length and aligned trees first, the main tree last -- its second level takes the room of
  // the code lengths (which are in the record by then; not while a later header of this frame still works on them) ----
  bool tables = true, two_level = false;
  {
    const int r = huff_build<LZX_LEN_P>(sh->len_len, LZX_LEN_SYMS, 12, sh->len_tab, sh->len_sorted, sh->cnt, d.hr_len, lane, false);
    tables = r != 1;
    s.length_empty = (r == 2);
  }
  if (tables && btype == 2u) tables = !huff_build<LZX_ALI_P>(sh->ali_len, 8, 7, sh->ali_tab, sh->ali_sorted, sh->cnt, d.hr_ali, lane, false);
  if (tables) {
    u32 nsorted = 0;
    tables = !huff_build<LZX_MAIN_P, LZX_MSH, LZX_MTAB_T>(sh->main_len, lzx_main_build_syms(s.num_offsets), 12, sh->main_tab, sh->main_sorted,
                                                          sh->cnt, d.hr_main, lane, false, &nsorted);
    if (tables && published) two_level = rfl(lzx_build_sub(sh, d.hr_main, nsorted, lane) ? 1u : 0u) != 0u;
  }
  if (!tables) { lzx_status_publish(&rec->status, published ? LZX_ST_HDRONLY : LZX_ST_FAILED, lane); return 0u; }
  PH(3);
  u32 n_rec = 0, end_bit = 0, bytes_done = 0;
  u32 n_chunks = 0;
  {
    // (the frame's chunk list in LDS: the room of the pretree's table -- only a block header uses that; a later header of this
    // frame finds the list put aside, lzx_parse_emit)
    RecWriter W;
    W.begin(pool, (u32 *) sh->pre_tab, rec->chunk);
    const u32 plimit = rem < fsz ? rem : fsz;
    if (btype == 2u) lzx_parse_emit<true>(d, s.length_empty, cur_bit, fe * 8u, fout, f * LZX_FRAME, fsz, edge_n, rec, W, n_rec, end_bit, bytes_done, two_level, stream, plimit, true);
    else lzx_parse_emit<false>(d, s.length_empty, cur_bit, fe * 8u, fout, f * LZX_FRAME, fsz, edge_n, rec, W, n_rec, end_bit, bytes_done, two_level, stream, plimit, true);
    n_chunks = W.n_chunks;
  }
  if (!published) {
    // the block ends inside the frame.  Parsed up to its end: the next header is read THERE (a real call: the hot path above
    // does not carry the general case's registers).  Not that far: nothing to hand on -- the chain of code lengths ends here
    if (bytes_done == rem) {
      if (lane == 0) { sh->stage[LZX_TAIL_ARGS] = bytes_done; sh->stage[LZX_TAIL_ARGS + 1u] = n_rec; sh->stage[LZX_TAIL_ARGS + 2u] = end_bit; sh->stage[LZX_TAIL_ARGS + 3u] = n_chunks; }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      PHFLUSH();
      return 1u;
    }
    lzx_status_publish(&rec->status, LZX_ST_FAILED, lane);
    PHFLUSH();
    return 0u;
  }
  // a record that ends early must end behind at least one token of the block: the serial path goes on from its last bit with
  // this block's tables.  Else: code lengths only
  if (bytes_done < fsz && bytes_done == 0u) { lzx_status_publish(&rec->status, LZX_ST_HDRONLY, lane); PHFLUSH(); return 0u; }
  if (lane == 0) {
    rec->n_tokens = n_rec; rec->end_bit = end_bit; rec->bytes_done = bytes_done;
    rec->flags = rec->flags | (s.length_empty ? 1u : 0u);
  }
  PH(4);
  lzx_status_publish(&rec->status, LZX_ST_EMITTED, lane);
  PH(5);
#ifdef LZX_PIPE_TRACE
  pha_[6] = d.st_t[6]; pha_[7] = d.st_t[7]; pha_[8] = d.st_t[8];
  pha_[12] = d.st_t[0]; pha_[13] = d.st_t[1]; pha_[14] = d.st_t[2]; pha_[15] = d.st_t[3];
  pha_[9] = d.st_t[4]; pha_[10] = d.st_t[5];
#endif
  PHFLUSH();
  return 0u;
}
