// lzx_run.hpp -- the commit half of a speculative run: 64 parsed tokens, one per lane, become output positions, literal
// stores, R0-R2 and queued match copies.  Shared by lzx_run_spec (lzx_run_delta.hpp) and lzx_run_spec2 (lzx_run_plain.hpp).
// Compiled into lzxn and lzxd.  Replaces the body of the reference's main decode loop, lzxd.c:538-651 (R0-R2: 565-586,
// the checks: 613-634, 678-693); the match copies are deferred to spec_queue.hpp.

// ---------------------------------------------------------------------------------------------------
// The speculative decode of a run of tokens (lzxd.c:538-651), in two alternating phases.
//
// PARSE (per round of 64 bit positions): every lane decodes the complete token that would start at bit
// (bitpos + lane); the chain of real tokens is followed with v_readlane; the tokens on the chain are
// appended to a token queue in LDS (kind, output length, offset or literal, start bit).  Nothing else
// happens in a round: no output position is needed to find the next token, so the serial chain of the
// whole decoder is just "decode 64 positions, walk".  A token the lane-parallel decoder does not take
// (a code beyond the direct length / aligned tables, an invalid one) is decoded on the scalar side from
// the same 64 bits and queued like the others.
//
// COMMIT (per 64 queued tokens, one token per lane, all lanes busy): prefix sum of the output lengths
// -> positions; literals are stored; R0-R2 are resolved for all matches at once (lru_scan); the
// reference's checks (lzxd.c:613-634, 678-693) run for all matches at once; the matches go to the
// deferred-copy queue of spec_queue.hpp, which is resolved 64 output bytes per pass.
//
// The parser runs ahead of the committed position, so at the end of a run (lzxd.c:538: tokens are read
// only while this_run > 0) it has parsed tokens that do not belong to the run -- bits of the next block
// header read as tokens.  They are dropped and the bit position goes back to the first of them (every
// record carries the low 16 bits of its start).  For the same reason the parser never fails: what it
// cannot decode becomes a FAIL marker that only counts when the commit reaches it.
// ---------------------------------------------------------------------------------------------------

// ---- COMMIT: one batch of parsed tokens, one token per lane ---------------------------------------------
// Used by the speculative runs of the serial path (tokens from the LDS queue).
struct LzxCommit {                  // wave-uniform commit-side state of a run
  u32 P, R0, R1, R2;
  u32 run_end, wbase, wsize, offset_written, ref_size;
  SpecQueue Q;
};
#define LZX_TK_BAIL 6u             /* DELTA: a match length that announces an extension (lzxd.c:588-611) */
#define LZX_TK_FAIL 7u

// c0 = kind | output length << 3 | ..., c1 = literal or explicit offset; lanes >= n are idle.  Returns the number
// of tokens taken: fewer than n at a marker (its kind in `marker`) or where the run ends (lzxd.c:538).
__device__ __forceinline__ u32 lzx_commit_batch(LzxDec &d, LzxCommit &C, const u32 c0, const u32 c1, u32 n,
                                                u32 &marker, bool &fail_after)
{
  LzxShared *sh = d.sh;
  const u32 lane = d.lane;
  u8 *const out = d.out;
  const u32 run_end = C.run_end, wbase = C.wbase, wsize = C.wsize;
  const u32 P = C.P;
  const u32 kind = c0 & 7u;
  marker = 0; fail_after = false;
  {
    const u64 mk = ballot(lane < n && kind >= LZX_TK_BAIL);
    if (mk) { const u32 jm = (u32) __ffsll((long long) mk) - 1u; marker = rdl(kind, jm); n = jm; }
  }
  const u32 olen = lane < n ? ((c0 >> 3) & 511u) : 0u;
  const u32 incl = wave_incl_scan(olen);
  const u32 opos = P + incl - olen;                   // output position of this lane's token
  u32 newP = P + rdl(incl, 63u);
  // tokens are decoded only while the run lasts (lzxd.c:538): the first one that would start at or
  // after run_end, and everything parsed behind it, is not part of this run
  if (newP >= run_end) {
    // (a literal run that would cross the end of the run is not taken either: the serial path goes on there)
    const u64 late = ballot(lane < n && (opos >= run_end || (kind == 0u && opos + olen > run_end)));
    if (late) { const u32 j = (u32) __ffsll((long long) late) - 1u; n = j; newP = rdl(opos, j); marker = 0; }
  }
  const bool valid = lane < n;
  if (valid && kind == 0u) {
    gst(out + opos, (u8) c1);
    if (olen > 1u) {                                        // a literal run: 2..4 bytes, first literal in the low byte
      gst(out + opos + 1u, (u8)(c1 >> 8));
      if (olen > 2u) gst(out + opos + 2u, (u8)(c1 >> 16));
      if (olen > 3u) gst(out + opos + 3u, (u8)(c1 >> 24));
    }
  }
  const bool ism0 = valid && kind != 0u;
  u64 mm = ballot(ism0);
  if (mm) {
    // (1) every match's offset through the R0-R2 LRU (lzxd.c:565-586)
    const u32 sR0 = C.R0, sR1 = C.R1, sR2 = C.R2;
    u32 vmoff = c1;
    const u64 k1 = ballot(ism0 && kind == 1u);
    if (!ballot(ism0 && kind >= 3u)) {
      // only explicit offsets and repeats of R0: a repeat takes the nearest explicit offset before
      // it, and the last three explicit offsets are the new R0-R2
      const u64 below = k1 & ((1ull << lane) - 1ull);
      const u32 src = below ? 63u - (u32) __clzll((long long) below) : 0u;
      const u32 pv = (u32) __builtin_amdgcn_ds_bpermute((int)(src << 2), (int) c1);
      if (kind == 2u) vmoff = below ? pv : sR0;
      if (k1) {
        u64 m = k1;
        const u32 j0 = 63u - (u32) __clzll((long long) m);
        u32 nb = sR0, nc = sR1;
        m &= ~(1ull << j0);
        if (m) {
          const u32 j1 = 63u - (u32) __clzll((long long) m);
          nb = rdl(c1, j1); nc = sR0;
          m &= ~(1ull << j1);
          if (m) nc = rdl(c1, 63u - (u32) __clzll((long long) m));
        }
        C.R0 = rdl(c1, j0); C.R1 = nb; C.R2 = nc;
      }
    }
    else {
      u32 x = LRU_ID;
      if (ism0) x = kind == 1u ? (0x010080u | lane) : (kind == 3u ? 0x020001u : (kind == 4u ? 0x000102u : LRU_ID));
      const u32 Cm = lru_scan(x);
      const u32 e0 = Cm & 0xFFu;
      const u32 pv = (u32) __builtin_amdgcn_ds_bpermute((int)((e0 & 63u) << 2), (int) c1);
      vmoff = (e0 & 0x80u) ? pv : (e0 == 0u ? sR0 : (e0 == 1u ? sR1 : sR2));
      const u32 Cl = rdl(Cm, 63u);
      const u32 f0 = Cl & 0xFFu, f1 = (Cl >> 8) & 0xFFu, f2 = (Cl >> 16) & 0xFFu;
      C.R0 = (f0 & 0x80u) ? rdl(c1, f0 & 63u) : (f0 == 0u ? sR0 : (f0 == 1u ? sR1 : sR2));
      C.R1 = (f1 & 0x80u) ? rdl(c1, f1 & 63u) : (f1 == 0u ? sR0 : (f1 == 1u ? sR1 : sR2));
      C.R2 = (f2 & 0x80u) ? rdl(c1, f2 & 63u) : (f2 == 0u ? sR0 : (f2 == 1u ? sR1 : sR2));
    }
    // (2) the reference's checks (lzxd.c:613-634, 678-693) for all matches at once
    {
      const u32 wp = opos - wbase;
      const bool bad = ism0 && (opos + olen > run_end || wp + olen > wsize ||
                                LZX_BAD_SOURCE(vmoff, wp, C.offset_written, C.ref_size, wsize));
      const u64 badm = ballot(bad);
      if (badm) { mm &= (1ull << ((u32) __ffsll((long long) badm) - 1u)) - 1ull; fail_after = true; }
    }
    // (3) queue the matches
    if (mm) {
      bool ism = lane_in(mm);
      // Offsets no linear copy can serve (0, or beyond the window: only from a stored block's R0-R2;
      // DELTA: beyond the 23 bits the queue holds) take the slow way: resolve the queue, copy this
      // batch's matches one at a time with the reference's ring semantics.
      if (ballot(ism && (vmoff == 0u || vmoff > wsize || (vmoff >> 23) != 0u))) {
        spq_resolve(sh->spq, C.Q, out, P, true, lane);
        for (u64 dm = mm; dm; dm &= dm - 1ull) {
          const u32 l = (u32) __ffsll((long long) dm) - 1u;
          const u32 pos_l = rdl(opos, l), len_l = rdl(olen, l), off_l = rdl(vmoff, l);
          if (off_l != 0u && off_l <= wsize) lzx_copy_match(out, pos_l, off_l, len_l, lane);
          else { if (lane == 0) lzx_copy_match_odd(out, pos_l, pos_l - wbase, wsize, off_l, len_l); }
        }
        C.Q.Pf = newP;
      }
      else {
        if (C.Q.mcount + (u32) __popcll(mm) > SPQ_CAP) spq_resolve(sh->spq, C.Q, out, P, true, lane);
        for (;;) {
          // a push must keep every start flag inside the ring (spec_queue.hpp): take the matches that
          // end inside it, resolve up to the first one that does not, go on
          const u32 limit = (C.Q.Pf & ~63u) + SPQ_RING;
          const u64 fit = newP <= limit ? mm : ballot(ism && opos + olen <= limit);
          if (fit) {
            const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(fit >> 32), __builtin_amdgcn_mbcnt_lo((u32) fit, 0u));
            spq_push(sh->spq, C.Q, lane_in(fit), rank, (u32) __popcll(fit), opos, vmoff, olen);
            mm &= ~fit;
            ism = lane_in(mm);
          }
          if (!mm) break;
          spq_resolve(sh->spq, C.Q, out, rdl(opos, (u32) __ffsll((long long) mm) - 1u), true, lane);
        }
      }
    }
  }
  C.P = newP;
  return n;
}
