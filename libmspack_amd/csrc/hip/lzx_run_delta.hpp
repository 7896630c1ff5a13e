// lzx_run_delta.hpp -- lzx_run_spec: the speculative run of LZX DELTA (parse whole tokens 64 bit positions per round, commit
// 64 tokens at a time); the PARSE / COMMIT scheme is described in lzx_run.hpp.  Compiled into lzxd only.  Replaces
// lzxd.c:538-651; a match length that announces an extension (lzxd.c:588-611) goes back to the scalar loop of lzx_unit.hpp.
#define LZX_TQ 128u                /* token queue entries (two commits' worth) */

template <bool ALIGNED>
__device__ __forceinline__ int lzx_run_spec(LzxDec &d, LzxState &s, const u32 run_end_, const u32 wbase_)
{
  LzxShared *sh = d.sh;
  const u32 lane = d.lane;
  u8 *const out = d.out;
  // everything below is wave-uniform; readfirstlane tells the compiler so (SGPRs, scalar branches)
  LzxCommit C;
  C.run_end = rfl(run_end_); C.wbase = rfl(wbase_);
  C.P = rfl(d.P);
  C.R0 = rfl(s.R0); C.R1 = rfl(s.R1); C.R2 = rfl(s.R2);
  C.wsize = rfl(s.wsize); C.offset_written = rfl(s.offset); C.ref_size = rfl(s.ref_size);
  const bool length_empty = rfl((u32) s.length_empty) != 0u;
  int rc = LZX_RUN_DONE;

  // The parser stops `margin` bytes before the end of the input.  A round (64 starts + a 53-bit
  // token) plus one scalar token consumes at most 22 bytes, a block header read without any symbol
  // decode 17 more and the first symbol after it 7: with 56 the EOF-exact reader
  // (LzxDec::sym_ensure) still takes over at a symbol boundary at least 6 bytes before the
  // reference's read pointer can reach the end of the input.
  const u32 bit_limit = spec_bit_limit(d, 56u);
  if (rfl(d.cons_bits()) >= bit_limit) return LZX_RUN_SWITCH;
  // pending literals of the scalar path go out first: this path stores literals directly
  d.flush_lits();
  u32 bitpos, cb, pf;                                   // next unparsed bit (relative to d.w.origin)
  spec_stage(d, bitpos, cb, pf);
  u32 mlim[16 - LZX_MAIN_P];                            // limits of the code lengths beyond the table
#pragma unroll
  for (int l = LZX_MAIN_P + 1; l <= 16; l++) mlim[l - LZX_MAIN_P - 1] = rdl(d.hr_main.limv, (u32) l);

  spq_init(sh->spq, C.Q, C.P, lane);
  u32 *const tq0 = sh->tq0, *const tq1 = sh->tq1;
  u32 th = 0, tt = 0;                                   // token queue: committed / parsed (counters)
  bool stop = false;                                    // the parser is done (input margin, marker)
  bool bail = false;

  while (rc == LZX_RUN_DONE && C.P < C.run_end && !bail) {
    // =================================== PARSE ===================================
    if (!stop && tt - th < 64u) {
      spec_slide(d, bitpos, cb, pf);
      const u32 rel = bitpos - (cb << 11) + lane;
      const u32 k = rel >> 5, sft = rel & 31u;
      const u32 i0 = sh->inbuf[k], i1 = sh->inbuf[k + 1u], i2 = sh->inbuf[k + 2u];
      const u32 w0 = (u32)(((((u64) i0 << 32) | i1) << sft) >> 32);
      const u32 w1 = (u32)(((((u64) i1 << 32) | i2) << sft) >> 32);
      const SpecTok t = lzx_spec_token<ALIGNED>(sh, d.hr_main.fov, mlim, length_empty, w0, w1);
      // next token start (in bits from bitpos); >= 256 marks "needs the scalar decoder" and ends the walk
      const u32 vn = t.unk ? (256u + lane) : (lane + t.tot);
      // ---- follow the real token boundaries: which positions start a token? ----
      u64 chain = 0, chain2 = 0;
      u32 q = 0;
      do { chain |= 1ull << q; q = rdl(vn, q); } while (q < 64u);
      bool hit_unknown = false;
      if (q >= 256u) {
        q -= 256u; hit_unknown = true;
        if (q < 64u) chain &= ~(1ull << q); else chain2 &= ~(1ull << (q - 64u));
      }
      u32 nA = (u32) __popcll(chain), nB = (u32) __popcll(chain2);
      // ---- queue the tokens on the chain ----
      {
        const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(chain >> 32), __builtin_amdgcn_mbcnt_lo((u32) chain, 0u));
        if ((chain >> lane) & 1ull) {
          const u32 ti = (tt + rank) & (LZX_TQ - 1u);
          tq0[ti] = t.kind | (t.olen << 3) | (((bitpos + lane) & 0xFFFFu) << 12);
          tq1[ti] = t.kind == 0u ? t.sym : t.off;
        }
        tt += nA + nB;
      }
      bitpos += q;
      d.st_rounds++;
      if (hit_unknown) {
        u32 tk_kind = 0, tk_val = 0, tk_off = 0;
        const u64 rq = ((u64) rdl(w0, q) << 32) | rdl(w1, q);
        const u32 tk_tot = lzx_scalar_token<ALIGNED>(d, length_empty, rq, tk_kind, tk_val, tk_off);
        u32 r0, r1 = tk_kind == 0u ? tk_val : tk_off;
        if (tk_tot == 0u) { r0 = LZX_TK_FAIL; stop = true; }
        else if (tk_kind != 0u && tk_val == 257u) { r0 = LZX_TK_BAIL; stop = true; }
        else r0 = tk_kind | ((tk_kind == 0u ? 1u : tk_val) << 3);
        if (lane == 0u) {
          const u32 ti = tt & (LZX_TQ - 1u);
          tq0[ti] = r0 | ((bitpos & 0xFFFFu) << 12);
          tq1[ti] = r1;
        }
        tt++;
        if (!stop) bitpos += tk_tot;
      }
      if (bitpos >= bit_limit) stop = true;
      if (!stop && tt - th < 64u) continue;
    }

    // =================================== COMMIT ===================================
    u32 n = tt - th;
    if (n > 64u) n = 64u;
    if (n == 0u) { rc = LZX_RUN_SWITCH; break; }         // the input margin was reached and all is committed
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const u32 ci = (th + lane) & (LZX_TQ - 1u);
    const u32 c0 = tq0[ci], c1 = tq1[ci];
    u32 marker; bool fail_after;
    th += lzx_commit_batch(d, C, c0, c1, n, marker, fail_after);
    if (spq_due(C.Q, C.P)) spq_resolve(sh->spq, C.Q, out, C.P, false, lane);
    if (fail_after || marker == LZX_TK_FAIL) { d.err = ERR_DECRUNCH; rc = LZX_RUN_FAIL; }
    else if (marker == LZX_TK_BAIL) bail = true;
  }
  spq_resolve(sh->spq, C.Q, out, C.P, true, lane);
  // parsed but not committed: the bit position goes back to the first such token
  if (tt != th) {
    const u32 lo = rfl(tq0[th & (LZX_TQ - 1u)]) >> 12;
    bitpos -= (bitpos - lo) & 0xFFFFu;
  }
  d.P = C.P;
  s.R0 = C.R0; s.R1 = C.R1; s.R2 = C.R2;
  spec_resync(d, bitpos, cb, pf);
  return rc;
}
