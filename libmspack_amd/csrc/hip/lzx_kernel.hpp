// lzx_kernel.hpp -- the core every LZX wave is made of (the file keeps its name, and its history, for this part):
// table widths, the LDS block (LzxShared), the bit reader (LzxDec), the
// decoder state (LzxState), block headers, match copies, the lane-parallel token decoders and the R0-R2 scan.
//
// Compiled by shim.hip into all three namespaces: lzxn (plain LZX of CAB folders and CHM sections), lzxd (LZX_DELTA: LZX
// DELTA of OAB files) and lzxp (LZX_PARSE_ONLY: the parse waves of the frame-parallel path).  The two macros are looked at
// here for the layout of LzxShared and the main-tree table only; the role headers that follow (lzx_run*.hpp, lzx_pipe*.hpp,
// lzx_unit.hpp) are included per namespace.
//
// Replaces of the reference (libmspack/mspack), bit-exact in output and error code:
//   bit reader ........ readbits.h:133-166 + lzxd.c:85-91 -> 64-bit SGPR bit buffer, refilled 32 bits
//                       at a time by v_readlane from the lane-resident input chunk
//   READ_HUFFSYM ...... readhuff.h:39-66 -> one LDS lookup (10/8/7/6 direct bits); long codes by a
//                       wave-wide limit compare + ballot (wave_common.hpp)
//   make_decode_table . readhuff.h:83-176 -> lane-parallel build, same accept/reject set
//   lzxd_read_lens .... lzxd.c:138-183 -> lzx_read_lens_spec: pretree tokens decoded 64 bit positions at a
//                       time, run lengths prefix-summed into indices (each length is a delta on the
//                       previous block's value, so the lengths array itself stays in LDS)
//   reset, block header lzxd.c:257-270, 467-523
//   match copy ........ lzxd.c:613-646 -> one coalesced 64-lane load/store per 64 bytes, the overlapping case
//                       (offset < length) served from the periodic source
// The output buffer doubles as the LZ77 window ("linear window"): src = pos - offset, valid because
// frames never straddle the window wrap (lzxd.c:655-656); positions modulo window_size are kept
// only for the reference's error checks (lzxd.c:613-634).
//
// LZX_DELTA (lzxd.c:288-293, 348-382, 440-444, 588-611): windows 2^17..2^25 (main alphabets of up to 2576
// symbols: the main-tree table entries are 32 bits wide with a 12-bit symbol field), a 16-bit
// chunk size in front of every frame, match lengths extended beyond 257, and reference data that
// sits in the output arena right below the unit's output (positions are then biased by its size,
// so a source inside the reference data is an ordinary linear copy).
#include "wave_common.hpp"
#include "spec_queue.hpp"

#define LZX_FRAME 32768u
#undef LZX_MAIN_P
#ifdef LZX_PARSE_ONLY
/* namespace lzxp (shim.hip): the parse waves of the frame-parallel path.  They need no match
 * queue and no token queue, and a main-tree table of 8 direct bits (codes beyond it are resolved lane-parallel
 * anyway): 5.5 KiB of LDS instead of 9.75, i.e. 7 waves per SIMD instead of 4 -- parse throughput is a matter of
 * how many serial chains a SIMD can interleave */
#define LZX_MAIN_P 8
#else
#define LZX_MAIN_P 10
#endif
#define LZX_LEN_P 9
#define LZX_ALI_P 7
#define LZX_PRE_P 6
#undef LZX_MAIN_SYMS
#undef LZX_MSH
#undef LZX_MTAB_T
#ifdef LZX_DELTA
#define LZX_MAIN_SYMS 2640     /* 256 + 290*8 + 64 (w<=25) */
#define LZX_MSH 12             /* main-tree table entries: symbol | length << 12, in 32 bits */
#define LZX_MTAB_T u32
#else
#define LZX_MAIN_SYMS 720      /* 256 + 50*8 + 64: every index that can ever be non-zero (w<=21) */
#define LZX_MSH 10             /* symbol | length << 10, in 16 bits */
#define LZX_MTAB_T u16
#endif
#define LZX_MMASK ((1u << LZX_MSH) - 1u)
#define LZX_LEN_SYMS 250
#ifdef LZX_MARKS      /* analysis builds: region markers in the assembly (tools/count_isa.py) */
#define LZX_MARK(name) asm volatile("; MARK " name)
#else
#define LZX_MARK(name) do { } while (0)
#endif

struct __align__(16) LzxShared {
  LZX_MTAB_T main_tab[1 << LZX_MAIN_P];
  u16 main_sorted[LZX_MAIN_SYMS];
  u16 len_tab[1 << LZX_LEN_P];
  u16 len_sorted[256];
  u16 ali_tab[1 << LZX_ALI_P];
  u16 ali_sorted[8];
#if defined(LZX_DELTA) || defined(LZX_PARSE_ONLY)
  u16 pre_tab[1 << LZX_PRE_P];
  u16 pre_sorted[24];
  u32 cnt[20];
  u8  pre_len[24];
#ifndef LZX_PARSE_ONLY
  u32 inbuf[128 + 4];            /* speculative path: two 256-byte input chunks, words pre-swapped */
#else
  u32 stage[LZX_STAGE_WORDS + 64]; /* lzx_parse_emit: a stretch of a frame's input, words pre-swapped */
  alignas(16) u32 litring[LZX_LIT_RING / 4u];  /* lzx_parse_emit: the literals of the last walk's rounds on their way out (whole 16-byte rows) */
  /* what only the block header needs -- its input window and the code lengths -- shares its room with the main tree's
   * second-level table (lzx_build_sub), which is built when the header is done and the lengths are in the frame's record */
  union {
    struct {
      u32 inbuf[128 + 4];
      u8  main_len[LZX_MAIN_SYMS + 16];
      u8  len_len[LZX_LEN_SYMS + 70];
      u8  ali_len[8];
    };
    u16 sub_tab[(528 + LZX_MAIN_SYMS + 16 + LZX_LEN_SYMS + 70 + 8) / 2];
  };
#endif
#else
  /* lzx_run_spec2's token queue (start bits of parsed tokens) shares its room with what only block headers
   * use (pretree tables, the table builder's counters): a header is never decoded while tokens are queued */
  union {
    u32 tq0[256];
    struct { u16 pre_tab[1 << LZX_PRE_P]; u16 pre_sorted[24]; u32 cnt[20]; u8 pre_len[24]; };
  };
  u32 inbuf[192 + 4];            /* lzx_run_spec2: three chunks (the one behind the parse position too: queued
                                    tokens are decoded from their start bit at commit time) */
#endif
#ifndef LZX_PARSE_ONLY
  u8  main_len[LZX_MAIN_SYMS + 16];
  u8  len_len[LZX_LEN_SYMS + 70];
  u8  ali_len[8];
  SpecQueueLds spq;              /* speculative path: queued matches + start flags (spec_queue.hpp) */
#ifdef LZX_DELTA
  u32 tq0[128], tq1[128];        /* lzx_run_spec keeps whole tokens (kind/length, value) */
#else
  u32 side0[16], side1[16];      /* lzx_run_spec2 keeps start bits; the few tokens the scalar decoder took are here */
#endif
#endif
};

struct LzxDec {
  // ---- input / bit buffer (wave-uniform unless noted) ----
  InWindow w;
  u64 bb; int bl;
  bool near_end, careful; int rbl;   // reference bits_left is simulated only near end of input
  int err;
  u32 lane;
  // ---- output ----
  u8 *out; u32 P;                    // linear position == bytes decoded since unit start
  u32 lit_buf; u32 lit_n;            // lit_buf is per-lane
  u32 st_rounds;                     // speculative rounds run (lzx_run_*.hpp).  Nothing reads it and no instruction is emitted for it,
                                     // but the register allocator orders 14 / 16 scalar moves of mspack_decode_lzxd / _lzx differently
                                     // without the counter (tools/isa_diff.sh), so it stays while the kernels are to stay as they are
  u32 st_t[10];                      // LZX_PIPE_TRACE builds: the parse task's phase sums (lzx_pipe.hpp: PHE / PHCNT)
  LzxShared *sh;
  HuffRegs hr_main, hr_len, hr_ali, hr_pre;

  __device__ __forceinline__ u32 cons_bits() const { return w.wi * 32u - (u32) bl; }
  __device__ __forceinline__ void refill() {
    u32 d = w.next_dword(lane);
    u32 x = (d << 16) | (d >> 16);               // two LE16 words, first word on top (lzxd.c:85-91)
    bb |= (u64) x << (32 - bl);
    bl += 32;
    u32 fetched = w.origin + w.wi * 4u;
    if (fetched >= w.in_len || w.in_len - fetched <= 64u) near_end = true;
  }
  __device__ __forceinline__ void need(int n) { if (bl < n) refill(); }   // n <= 32
  __device__ __forceinline__ bool ref_ensure(int n) {             // ENSURE_BITS(n) of the reference, EOF-exact
    while (rbl < n) {
      u32 i = w.origin + ((cons_bits() + (u32) rbl) >> 3);   // the reference's i_ptr
      if (i + 2u > w.in_len + w.eofs) { err = ERR_READ; return false; }   // fake bytes, then ERR_READ
      rbl += 16;
    }
    return true;
  }
  __device__ __forceinline__ bool sym_ensure() {  // ENSURE_BITS(16): bits_left becomes a pure
    if (careful) return ref_ensure(16);           // function of the bit position
    if (near_end) { careful = true; rbl = 16 + (int)((0u - cons_bits()) & 15u); }
    return true;
  }
  __device__ __forceinline__ void drop(int n) { bb <<= n; bl -= n; if (careful) rbl -= n; }
  __device__ __forceinline__ bool read_bits(int n, u32 &v) {    // READ_BITS, 1 <= n <= 17
    need(n);
    if (careful && !ref_ensure(n)) return false;
    v = (u32)(bb >> (64 - n));
    drop(n);
    return true;
  }
  template <int TP, int SH = 10, typename TabT = u16>
  __device__ __forceinline__ int decode_sym(const TabT *tab, const u16 *sorted, const HuffRegs &hr) {
    if (!sym_ensure()) return -1;
    u32 e = rfl((u32) tab[(u32)(bb >> (64 - TP))]);
    if (e == 0) {
      e = huff_long<SH>(hr, sorted, (u32)(bb >> 48), lane);
      if (e == 0) { err = ERR_DECRUNCH; return -1; }
    }
    drop((int)(e >> SH));
    return (int)(e & ((1u << SH) - 1u));
  }
  // the reference's i_ptr (bytes) -- exact in careful mode, a lower bound otherwise
  __device__ __forceinline__ u32 iptr() const {
    u32 c = cons_bits();
    return w.origin + (careful ? ((c + (u32) rbl) >> 3) : (((c + 15u) & ~15u) >> 3));
  }

  __device__ __forceinline__ void flush_lits() {
    if (lit_n) {
      if (lane < lit_n) gst(out + P - lit_n + lane, (u8) lit_buf);
      lit_n = 0;
    }
  }
};

__device__ __forceinline__ u32 lzx_read_lens_spec(LzxDec &d, u8 *lens, u32 first, u32 last);

// lzxd_read_lens (lzxd.c:138-183).  Every length is a delta against the previous block's lens[x], but
// the tokens of one call never depend on each other: far from the end of the input they are decoded
// 64 bit positions at a time (lzx_read_lens_spec); the scalar loop below is the EOF-exact version.
__device__ __forceinline__ bool lzx_read_lens(LzxDec &d, u8 *lens, u32 first, u32 last)
{
  LzxShared *sh = d.sh;
  u32 v;
  for (u32 x = 0; x < 20; x++) {
    if (!d.read_bits(4, v)) return false;
    sh->pre_len[x] = (u8) v;
  }
  if (d.lane < 4u) sh->pre_len[20 + d.lane] = 0;
  if (huff_build<LZX_PRE_P>(sh->pre_len, 20, 6, sh->pre_tab, sh->pre_sorted, sh->cnt, d.hr_pre, d.lane, false)) {
    d.err = ERR_DECRUNCH; return false;                       // incl. the all-zero pretree
  }
  if (!d.careful) first = lzx_read_lens_spec(d, lens, first, last);
  for (u32 x = first; x < last; ) {
    d.need(32);
    int z = d.decode_sym<LZX_PRE_P>(sh->pre_tab, sh->pre_sorted, d.hr_pre);
    if (z < 0) return false;
    if (z == 17 || z == 18) {
      u32 y;
      if (!d.read_bits(z == 17 ? 4 : 5, y)) return false;
      y += (z == 17) ? 4u : 20u;
      for (u32 i = d.lane; i < y; i += WAVE) lens[x + i] = 0;  // runs are NOT clipped (lzxd.c:159)
      x += y;
    }
    else if (z == 19) {
      u32 y;
      if (!d.read_bits(1, y)) return false;
      y += 4u;
      d.need(16);
      int z2 = d.decode_sym<LZX_PRE_P>(sh->pre_tab, sh->pre_sorted, d.hr_pre);
      if (z2 < 0) return false;
      int nv = (int) rfl((u32) lens[x]) - z2; if (nv < 0) nv += 17;
      if (d.lane < y) lens[x + d.lane] = (u8) nv;
      x += y;
    }
    else {
      int nv = (int) rfl((u32) lens[x]) - z; if (nv < 0) nv += 17;
      lens[x] = (u8) nv;
      x++;
    }
  }
  return true;
}

struct LzxState {
  u32 R0, R1, R2;
  u32 block_type, block_length, block_remaining;
  u32 wsize, wpos, frame_posn, frame, reset_frames, num_offsets;
  u32 offset;            // bytes written (lzx->offset)
  u32 length;            // lzx->length
  int32_t intel_filesize;
  bool header_read, intel_started, length_empty;
  bool raw_mode; u32 raw_pos;   // inside / right after an uncompressed block: input byte position
  u32 ref_size;          // LZX DELTA: bytes of reference data below position 0 (0 otherwise)
};

// a match source before the window position is legal when the stream has produced that much, or
// (DELTA) when it stays inside the reference data; never beyond the window (lzxd.c:622-634)
#define LZX_BAD_SOURCE(off_, wp_, written_, ref_, wsize_)                                       \
  ((off_) > (wp_) && ((((off_) > (written_)) && (((off_) - (wp_)) > (ref_))) || (((off_) - (wp_)) > (wsize_))))

// symbols the main table is built over: every index a pretree run can make non-zero (up to 4 past 256 + num_offsets,
// lzxd.c:159-166), but never beyond LZX_MAINTREE_MAXSYMBOLS = 2576 (lzx.h:38, lzxd.c:96-104): at 2^25 a run from entry
// 2575 writes 2576..2579, which the reference's table does not count
__device__ __forceinline__ int lzx_main_build_syms(u32 num_offsets)
{
  const int n = 256 + (int) num_offsets + 64;
  return n < 2576 ? n : 2576;
}

__device__ __forceinline__ void lzx_reset_state(LzxDec &d, LzxState &s) {      // lzxd.c:257-270
  s.R0 = s.R1 = s.R2 = 1;
  s.header_read = false; s.block_remaining = 0; s.block_type = 0;
  for (u32 i = d.lane; i < LZX_MAIN_SYMS + 16; i += WAVE) d.sh->main_len[i] = 0;
  // NB the reference clears exactly MAXSYMBOLS entries; the safety area beyond is never cleared
  // but also never read back for the length tree (index 249 is inside MAXSYMBOLS = 250)
  for (u32 i = d.lane; i < LZX_LEN_SYMS; i += WAVE) d.sh->len_len[i] = 0;
}

// leave raw (uncompressed-block) input mode: bit reading restarts at raw_pos with an empty buffer
__device__ __forceinline__ void lzx_leave_raw(LzxDec &d, LzxState &s) {
  if (s.raw_mode) {
    d.w.seek(s.raw_pos, d.lane);
    d.bb = 0; d.bl = 0; d.rbl = 0;
    u32 fetched = s.raw_pos;
    d.near_end = (fetched >= d.w.in_len || d.w.in_len - fetched <= 64u);
    if (d.near_end) d.careful = true;      // bits_left == 0 here: a determined point
    s.raw_mode = false;
  }
}

// block header (lzxd.c:467-523); returns false on error (d.err set)
__device__ __forceinline__ bool lzx_block_header(LzxDec &d, LzxState &s, const bool tables = true)
{
  LzxShared *sh = d.sh;
  u32 v, hi, lo;
  if (s.block_type == 3u && (s.block_length & 1u)) {            // odd-sized stored block: pad byte
    // bit buffer is empty here; the byte is skipped at i_ptr (lzxd.c:469-474)
    if (s.raw_mode) {
      if (s.raw_pos >= d.w.in_len + d.w.eofs) { d.err = ERR_READ; return false; }
      s.raw_pos++;
    }
    else {
      // stored block ended earlier in raw mode and we already re-seeked: cannot happen, raw_mode
      // is only left here or at a reset (where block_type is cleared)
    }
  }
  lzx_leave_raw(d, s);
  if (!d.read_bits(3, v) || !d.read_bits(16, hi) || !d.read_bits(8, lo)) return false;
  s.block_type = v;
  s.block_remaining = s.block_length = (hi << 8) | lo;
  if (v == 2u) {
    for (u32 i = 0; i < 8; i++) { u32 t; if (!d.read_bits(3, t)) return false; sh->ali_len[i] = (u8) t; }
    if (huff_build<LZX_ALI_P>(sh->ali_len, 8, 7, sh->ali_tab, sh->ali_sorted, sh->cnt, d.hr_ali, d.lane, false)) {
      d.err = ERR_DECRUNCH; return false;
    }
  }
  if (v == 1u || v == 2u) {
    // three pretree-coded runs (lzxd.c:491-497); one inlined call site keeps the code small
    int r = 0;
    for (int part = 0; part < 3; part++) {
      u8 *lens = (part == 2) ? sh->len_len : sh->main_len;
      u32 first = (part == 1) ? 256u : 0u;
      u32 last = (part == 0) ? 256u : (part == 1 ? 256u + s.num_offsets : 249u);
      if (!lzx_read_lens(d, lens, first, last)) return false;
      if (part == 1 && tables) {
        if (huff_build<LZX_MAIN_P, LZX_MSH, LZX_MTAB_T>(sh->main_len, lzx_main_build_syms(s.num_offsets), 12, sh->main_tab, sh->main_sorted,
                                   sh->cnt, d.hr_main, d.lane, false)) {
          d.err = ERR_DECRUNCH; return false;
        }
        if (rfl((u32) sh->main_len[0xE8]) != 0u) s.intel_started = true;
      }
    }
    if (!tables) return true;              // a parse wave walking the headers in front of its own frame: lengths only
    r = huff_build<LZX_LEN_P>(sh->len_len, LZX_LEN_SYMS, 12, sh->len_tab, sh->len_sorted, sh->cnt,
                              d.hr_len, d.lane, false);
    if (r == 1) { d.err = ERR_DECRUNCH; return false; }
    s.length_empty = (r == 2);                                   // lzxd.c:111-125
    return true;
  }
  if (v == 3u) {
    s.intel_started = true;
    // discard 1..16 bits up to the next word boundary (a whole word if already aligned),
    // lzxd.c:506-507.  After the 27 header bits the reference holds < 16 bits, so the data starts
    // at the end of the current word, or one word further when exactly aligned.
    u32 c = d.cons_bits();
    u32 data = d.w.origin + (((c + 15u) & ~15u) >> 3) + (((c & 15u) == 0u) ? 2u : 0u);
    if (d.careful) {
      if (d.rbl == 0 && !d.ref_ensure(16)) return false;
    }
    // 12 bytes R0,R1,R2 (LE32), then the raw bytes; bytes up to in_len+1 exist (two fake zeros)
    if (data + 12u > d.w.in_len + d.w.eofs) { d.err = ERR_READ; return false; }
    u32 b = (d.lane < 12u) ? d.w.byte_at(data + d.lane) : 0u;
    u32 r[3];
#pragma unroll
    for (int k = 0; k < 3; k++)
      r[k] = rdl(b, 4 * k) | (rdl(b, 4 * k + 1) << 8) | (rdl(b, 4 * k + 2) << 16) | (rdl(b, 4 * k + 3) << 24);
    s.R0 = r[0]; s.R1 = r[1]; s.R2 = r[2];
    s.raw_mode = true; s.raw_pos = data + 12u;
    d.bb = 0; d.bl = 0; d.rbl = 0;
    return true;
  }
  d.err = ERR_DECRUNCH;
  return false;
}

// copy a match of `len` bytes at distance `off` (1 <= off <= window) to the linear position P
__device__ __forceinline__ void lzx_copy_match(u8 *out, u32 P, u32 off, u32 len, u32 lane)
{
  u8 *dst = out + P;
  const u8 *src = dst - off;
  if (off >= len || off >= WAVE) {
    // every 64-byte step only reads bytes that are already complete (earlier steps/tokens)
    for (u32 i = lane; i < len; i += WAVE) gst(dst + i, gld(src + i));
  }
  else {
    // overlapping copy, period `off` < 64: lane i takes pattern byte (i mod off)
    u32 r = lane, s = off << 5;
#pragma unroll
    for (int k = 0; k < 6; k++) { u32 t = r - s; r = t < r ? t : r; s >>= 1; }     // r = lane mod off
    u32 step = 64u, ss = off << 5;
#pragma unroll
    for (int k = 0; k < 6; k++) { u32 t = step - ss; step = t < step ? t : step; ss >>= 1; }  // 64 mod off
    for (u32 i = lane; i < len; i += WAVE) {
      gst(dst + i, gld(src + r));
      r += step; if (r >= off) r -= off;
    }
  }
}

// reference-exact slow path for offsets no encoder produces (0, or beyond the window: only reachable
// through R0-R2 loaded from a stored-block header).  Byte-serial ring semantics of lzxd.c:618-646.
__device__ void lzx_copy_match_odd(u8 *out, u32 P, u32 wpos, u32 wsize, u32 off, u32 len)
{
  u32 base = P - wpos;                       // linear position of window index 0 in this pass
  for (u32 k = 0; k < len; k++) {
    u32 sidx = (wpos - off + k) & (wsize - 1u);
    if (off > wpos) { u32 j = off - wpos; sidx = (k < j) ? (wsize - j + k) : (k - j); }
    u8 b = 0;
    if (sidx < wpos + k) b = out[base + sidx];
    else if (base + sidx >= wsize) b = out[base + sidx - wsize];
    out[P + k] = b;
  }
}


// what a steady-state run (lzx_run_spec, lzx_run_delta.hpp / lzx_run_spec2, lzx_run_plain.hpp) ends with: the run is through, the generic (EOF-exact) loop of
// lzx_decode_unit takes over -- always at a token boundary, where the reference's bits_left is a pure function of the bit
// position (LzxDec::sym_ensure) --, or the stream is bad
enum { LZX_RUN_DONE = 0, LZX_RUN_SWITCH = 1, LZX_RUN_FAIL = 2 };



// ---------------------------------------------------------------------------------------------------
// Speculative window decode: the steady-state path.
//
// A Huffman/LZ bitstream is serial only because a symbol's start is known once the previous symbol's
// length is.  So all 64 lanes decode a COMPLETE token (main symbol, length footer, offset bits,
// aligned symbol) each starting at a different bit -- lane l at bit (pos + l) -- with gathered LDS
// table lookups, and publish "bits consumed / kind / length / offset" in two registers.  The true
// symbol boundaries are then followed through those registers with v_readlane: a token costs two
// readlanes and a handful of scalar ops instead of a chain of dependent LDS round trips, and the
// lookups of ~6 consecutive tokens (64 bits / ~10 bits per token) overlap.  Tokens with a code
// longer than the direct table are decoded by the scalar routine from the same 64 bits.
// Input: the two current 256-byte chunks live in LDS with each dword's 16-bit halves swapped, so the
// stream is a plain MSB-first bit string; the next chunk is prefetched in a register.
// ---------------------------------------------------------------------------------------------------
template <bool ALIGNED>
__device__ __forceinline__ u32 lzx_scalar_token(const LzxDec &d, bool length_empty, u64 r,
                                                u32 &kind, u32 &val, u32 &off)
{
  const LzxShared *sh = d.sh;
  u32 tot = 0;
  u32 e = rfl((u32) sh->main_tab[(u32)(r >> (64 - LZX_MAIN_P))]);
  if (e == 0) { e = huff_long<LZX_MSH>(d.hr_main, sh->main_sorted, (u32)(r >> 48), d.lane); if (e == 0) return 0; }
  { u32 l = e >> LZX_MSH; r <<= l; tot += l; }
  u32 sym = e & LZX_MMASK;
  if (sym < 256u) { kind = 0; val = sym; off = 0; return tot; }
  u32 m = sym - 256u, slot = m >> 3, len = (m & 7u) + 2u;
  if ((m & 7u) == 7u) {
    if (length_empty) return 0;
    u32 f = rfl((u32) sh->len_tab[(u32)(r >> (64 - LZX_LEN_P))]);
    if (f == 0) { f = huff_long(d.hr_len, sh->len_sorted, (u32)(r >> 48), d.lane); if (f == 0) return 0; }
    { u32 l = f >> 10; r <<= l; tot += l; }
    len += f & 1023u;
  }
  val = len;
  if (slot < 3u) { kind = 2u + slot; off = 0; return tot; }
  u32 extra = slot < 4u ? 0u : (slot < 36u ? (slot >> 1) - 1u : 17u);
  u32 base = slot < 4u ? slot : (slot < 36u ? ((2u + (slot & 1u)) << extra) : ((slot - 34u) << 17));
  off = base - 2u;
  if (ALIGNED && extra >= 3u) {
    u32 nb = extra - 3u;
    if (nb) { off += (u32)(r >> (64 - nb)) << 3; r <<= nb; tot += nb; }
    u32 a = rfl((u32) sh->ali_tab[(u32)(r >> (64 - LZX_ALI_P))]);
    if (a == 0) return 0;
    tot += a >> 10; off += a & 1023u;
  }
  else if (extra) { off += (u32)(r >> (64 - extra)); tot += extra; }
  kind = 1;
  return tot;
}


// one speculative token: everything lane-local, decoded from 64 bits of the stream
struct SpecTok { u32 tot, sym, kind, olen, off; bool unk;
};

template <bool ALIGNED>
__device__ __forceinline__ SpecTok lzx_spec_token(const LzxShared *sh, const u32 main_fov, const u32 *mlim,
                                                  const bool length_empty, const u32 w0, const u32 w1)
{
  SpecTok t;
  u64 r = ((u64) w0 << 32) | w1;
  u32 e = sh->main_tab[w0 >> (32 - LZX_MAIN_P)];
  {
    // codes longer than the direct table, for all lanes at once: canonical length = number of
    // per-length limits the 16-bit peek is not below; symbol via the sorted list (readhuff.h:144-172)
    u32 peek16 = w0 >> 16, ln = LZX_MAIN_P + 1u;
#pragma unroll
    for (int l = LZX_MAIN_P + 1; l <= 16; l++) ln += (peek16 >= mlim[l - LZX_MAIN_P - 1]) ? 1u : 0u;
    u32 lq = ln <= 16u ? ln : 0u;
    u32 fo = (u32) __builtin_amdgcn_ds_bpermute((int)(lq << 2), (int) main_fov);
    u32 idx = (fo >> 16) + ((peek16 >> (16u - lq)) - (fo & 0xFFFFu));
    if (idx >= LZX_MAIN_SYMS) idx = 0;
    u32 ls = sh->main_sorted[idx];
    if (e == 0u && lq != 0u) e = ls | (lq << LZX_MSH);
  }
  bool unk = (e == 0u);
  u32 tot = e >> LZX_MSH, sym = e & LZX_MMASK;
  r <<= tot;
  bool is_match = sym >= 256u;
  u32 m = sym - 256u, slot = m >> 3, lh = m & 7u;
  u32 e2 = sh->len_tab[(u32)(r >> (64 - LZX_LEN_P))];
  bool need_len = is_match && lh == 7u;
  if (need_len) { unk = unk || e2 == 0u || length_empty; u32 l2 = e2 >> 10; r <<= l2; tot += l2; }
  u32 mlen = lh + 2u + (need_len ? (e2 & 1023u) : 0u);
#ifdef LZX_DELTA
  if (is_match && mlen == 257u) unk = true;             // announces an extended length (lzxd.c:588-611)
#endif
  // position_base / extra_bits in closed form (lzxd.c:202-207), branch-free; only slots >= 3 matter here
  // (0..2 are the repeats): extra = clamp(slot/2 - 1, 0, 17), base = (slot < 36 ? 2 + (slot & 1) : slot - 34) << extra
  const int ex_ = (int)(slot >> 1) - 1;
  const u32 extra = (u32)(ex_ < 0 ? 0 : (ex_ > 17 ? 17 : ex_));
  u32 off = (((slot < 36u) ? 2u + (slot & 1u) : slot - 34u) << extra) - 2u;
  bool expl = is_match && slot >= 3u;
  if (ALIGNED) {
    bool ali = extra >= 3u;
    u32 nb = ali ? extra - 3u : extra;
    u32 vb = nb ? (u32)(r >> (64u - nb)) : 0u;
    u64 r2 = r << nb;
    u32 e3 = sh->ali_tab[(u32)(r2 >> (64 - LZX_ALI_P))];
    if (expl) {
      tot += nb;
      if (ali) { off += (vb << 3) + (e3 & 1023u); tot += e3 >> 10; unk = unk || e3 == 0u; }
      else off += vb;
    }
  }
  else {
    u32 vb = extra ? (u32)(r >> (64u - extra)) : 0u;
    if (expl) { off += vb; tot += extra; }
  }
  t.tot = tot; t.sym = sym; t.unk = unk; t.off = off;
  t.kind = !is_match ? 0u : (expl ? 1u : 2u + slot);
  t.olen = is_match ? mlen : 1u;
  return t;
}


// how many bits does the token take whose main-tree entry is e (symbol | code length << LZX_MSH, not 0)?
template <bool ALIGNED>
__device__ __forceinline__ u32 lzx_adv_from_entry(const LzxShared *sh, const bool length_empty, const u32 e,
                                                  const u32 w0, const u32 w1, bool &unk)
{
  const u32 mlen = e >> LZX_MSH, sym = e & LZX_MMASK;
  const bool is_match = sym >= 256u;
  const u32 m = sym - 256u, slot = m >> 3;
  const bool need_len = is_match && (m & 7u) == 7u;
  const u32 e2 = sh->len_tab[(w0 << mlen) >> (32 - LZX_LEN_P)];        // the footer's code starts right behind the main code
  u32 tot = mlen;
  unk = false;
  if (need_len) { unk = (e2 == 0u) || length_empty; tot += e2 >> 10; }
  const int ex_ = (int)(slot >> 1) - 1;
  const u32 extra = (u32)(ex_ < 0 ? 0 : (ex_ > 17 ? 17 : ex_));
  const bool expl = is_match && slot >= 3u;
  if (ALIGNED) {
    const bool ali = extra >= 3u;
    const u32 nb = ali ? extra - 3u : extra;
    const u64 r = ((u64) w0 << 32) | w1;
    const u32 e3 = sh->ali_tab[(u32)((r << (tot + nb)) >> (64 - LZX_ALI_P))];   // behind the verbatim bits (bit <= 46)
    if (expl) { tot += nb; if (ali) { tot += e3 >> 10; unk = unk || e3 == 0u; } }
  }
  else if (expl) tot += extra;
  return tot;
}


// ---- input staging shared by the speculative paths ----------------------------------------------
// The two current 256-byte input chunks live in LDS with each dword's 16-bit halves swapped (the
// stream becomes a plain MSB-first bit string); the next chunk is prefetched in a register.
#define SWAP16(x) (((x) << 16) | ((x) >> 16))
__device__ __forceinline__ void spec_stage(LzxDec &d, u32 &bitpos, u32 &cb, u32 &pf)
{
  LzxShared *sh = d.sh;
  const u32 lane = d.lane;
  bitpos = rfl(d.cons_bits());
  cb = bitpos >> 11;                                    // chunk cb = dwords [64cb, 64cb+64)
  u32 lo = d.w.load_chunk(cb, lane), hi = d.w.load_chunk(cb + 1u, lane);
  sh->inbuf[lane] = SWAP16(lo); sh->inbuf[64u + lane] = SWAP16(hi);
  if (lane < 4u) sh->inbuf[128u + lane] = 0;
  pf = d.w.load_chunk(cb + 2u, lane);
}
__device__ __forceinline__ void spec_slide(LzxDec &d, const u32 bitpos, u32 &cb, u32 &pf)
{
  if ((bitpos >> 11) != cb) {                           // slide the LDS window by one chunk
    LzxShared *sh = d.sh;
    const u32 lane = d.lane;
    u32 up = sh->inbuf[64u + lane];
    sh->inbuf[lane] = up; sh->inbuf[64u + lane] = SWAP16(pf);
    cb++;
    pf = d.w.load_chunk(cb + 2u, lane);
  }
}
// hand the exact bit position back to the scalar reader
__device__ __forceinline__ void spec_resync(LzxDec &d, const u32 bitpos, const u32 cb, const u32 pf)
{
  LzxShared *sh = d.sh;
  const u32 lane = d.lane;
  u32 wi = bitpos >> 5, ch = wi >> 6;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  u32 lo = sh->inbuf[lane], hi = sh->inbuf[64u + lane];
  lo = SWAP16(lo); hi = SWAP16(hi);
  if (ch == cb) { d.w.cur = lo; d.w.nxt = hi; }
  else if (ch == cb + 1u) { d.w.cur = hi; d.w.nxt = pf; }
  else { d.w.cur = d.w.load_chunk(ch, lane); d.w.nxt = d.w.load_chunk(ch + 1u, lane); }   // went back (end of a run)
  d.w.wi = wi; d.bb = 0; d.bl = 0;
  d.refill(); d.refill();
  u32 sk = bitpos & 31u;
  if (sk) { d.bb <<= sk; d.bl -= (int) sk; }
}
// last bit position (relative to the window origin) from which a speculative round may start; see
// the margin discussion in lzx_run_spec
__device__ __forceinline__ u32 spec_bit_limit(const LzxDec &d, const u32 margin)
{
  const u32 room_bytes = (d.w.in_len > d.w.origin + margin) ? (d.w.in_len - d.w.origin - margin) : 0u;
  return rfl(room_bytes * 8u);
}

// lzxd_read_lens, vector form.  Decodes pretree tokens from `first` on and returns the index the
// scalar loop has to continue from (== last when everything was done here).  A token = pretree
// symbol z [+ 4 / 5 / 1 extra bits for z = 17 / 18 / 19] [+ a second symbol for z = 19]; it sets
// y = 1 or a run of y lengths (lzxd.c:150-179).  All 64 lanes decode the token starting at bit
// (bitpos + lane); the chain of real tokens is followed with v_readlane; a prefix sum of the run
// lengths gives every token its index x; then every on-chain lane rewrites its own lens[x .. x+y).
__device__ __forceinline__ u32 lzx_read_lens_spec(LzxDec &d, u8 *lens, u32 first, u32 last_)
{
  LzxShared *sh = d.sh;
  const u32 lane = d.lane;
  const u32 last = rfl(last_);
  u32 X = rfl(first);
  const u32 bit_limit = spec_bit_limit(d, 56u);
  if (rfl(d.cons_bits()) >= bit_limit) return X;
  u32 bitpos, cb, pf;
  spec_stage(d, bitpos, cb, pf);
  u32 plim[16 - LZX_PRE_P];                             // limits of the code lengths beyond the table
#pragma unroll
  for (int l = LZX_PRE_P + 1; l <= 16; l++) plim[l - LZX_PRE_P - 1] = rdl(d.hr_pre.limv, (u32) l);

  while (X < last && bitpos < bit_limit) {
    spec_slide(d, bitpos, cb, pf);
    const u32 rel = bitpos - (cb << 11) + lane;
    const u32 k = rel >> 5, sft = rel & 31u;
    const u32 i0 = sh->inbuf[k], i1 = sh->inbuf[k + 1u], i2 = sh->inbuf[k + 2u];
    const u32 w0 = (u32)(((((u64) i0 << 32) | i1) << sft) >> 32);
    const u32 w1 = (u32)(((((u64) i1 << 32) | i2) << sft) >> 32);
    u64 r = ((u64) w0 << 32) | w1;
    u32 e = sh->pre_tab[w0 >> (32 - LZX_PRE_P)];
    {
      u32 peek16 = w0 >> 16, ln = LZX_PRE_P + 1u;
#pragma unroll
      for (int l = LZX_PRE_P + 1; l <= 16; l++) ln += (peek16 >= plim[l - LZX_PRE_P - 1]) ? 1u : 0u;
      u32 lq = ln <= 16u ? ln : 0u;
      u32 fo = (u32) __builtin_amdgcn_ds_bpermute((int)(lq << 2), (int) d.hr_pre.fov);
      u32 idx = (fo >> 16) + ((peek16 >> (16u - lq)) - (fo & 0xFFFFu));
      if (idx >= 20u) idx = 0;
      u32 ls = sh->pre_sorted[idx];
      if (e == 0u && lq != 0u) e = ls | (lq << 10);
    }
    bool unk = (e == 0u);
    const u32 z = e & 1023u;
    u32 tot = e >> 10;
    r <<= tot;
    const u32 nb = z == 17u ? 4u : (z == 18u ? 5u : (z == 19u ? 1u : 0u));
    const u32 xb = nb ? (u32)(r >> (64u - nb)) : 0u;
    r <<= nb; tot += nb;
    const u32 y = z == 17u ? 4u + xb : (z == 18u ? 20u + xb : (z == 19u ? 4u + xb : 1u));
    const u32 e2 = sh->pre_tab[(u32)(r >> (64 - LZX_PRE_P))];       // second symbol of a "same" run
    if (z == 19u) { unk = unk || e2 == 0u; tot += e2 >> 10; }       // (a long second code: scalar loop)
    const u32 zz = z == 19u ? (e2 & 1023u) : z;
    const bool zero = z == 17u || z == 18u;
    const u32 vnext = unk ? (128u + lane) : (lane + tot);

    u64 chain = 0;
    u32 q = 0;
    do { chain |= 1ull << q; q = rdl(vnext, q); } while (q < WAVE);
    bool hit_unknown = false;
    if (q >= 128u) { q -= 128u; chain &= ~(1ull << q); hit_unknown = true; }
    bool on = (chain >> lane) & 1ull;
    const u32 yy = on ? y : 0u;
    const u32 incl = wave_incl_scan(yy);
    const u32 x = X + incl - yy;
    u32 newX = X + rdl(incl, 63u);
    // lengths are read only while x < last (lzxd.c:148); a run may overshoot (it is not clipped)
    const u64 late = ballot(on && x >= last);
    if (late) {
      u32 j = (u32) __ffsll((long long) late) - 1u;
      chain &= (1ull << j) - 1ull;
      on = (chain >> lane) & 1ull;
      q = j; hit_unknown = false; newX = rdl(x, j);
    }
    if (on) {
      int nv = 0;
      if (!zero) { nv = (int)(u32) lens[x] - (int) zz; if (nv < 0) nv += 17; }
      for (u32 i = 0; i < y; i++) lens[x + i] = (u8) nv;
    }
    X = newX;
    bitpos += q;
    if (hit_unknown) break;                             // the scalar loop takes (and judges) this token
  }
  spec_resync(d, bitpos, cb, pf);
  return X;
}

// ---- R0-R2 as a prefix scan ----------------------------------------------------------------------
// What a token does to the three recent offsets (lzxd.c:565-586) is a map "new slot i <- old slot j or
// this token's own offset": an explicit offset is (own, R0, R1), a repeat of R0 changes nothing, a
// repeat of R1 / R2 swaps it with R0.  Such maps compose associatively, so the state after every token
// of a batch is an inclusive scan.  A map is three bytes, one per new slot: 0..2 = old slot, 0x80 | lane =
// the offset of the token in that lane.  v_perm_b32 composes two maps in one instruction.
#define LRU_ID 0x020100u
__device__ __forceinline__ u32 lru_compose(u32 first, u32 then)
{
  const u32 L = then & 0x808080u;                        // slots `then` fills with a token's own offset
  const u32 full = (L << 1) - (L >> 7);                  // 0xFF in those bytes
  const u32 sel = (then & ~full) | (0x060504u & full) | 0x0C000000u;
  return __builtin_amdgcn_perm(then, first, sel);        // byte i: first[then[i]] or then[i] itself
}
__device__ __forceinline__ u32 lru_scan(u32 x)
{
  u32 v = x, t;
  t = (u32) __builtin_amdgcn_update_dpp((int) LRU_ID, (int) v, 0x111, 0xf, 0xf, false); v = lru_compose(t, v);
  t = (u32) __builtin_amdgcn_update_dpp((int) LRU_ID, (int) v, 0x112, 0xf, 0xf, false); v = lru_compose(t, v);
  t = (u32) __builtin_amdgcn_update_dpp((int) LRU_ID, (int) v, 0x114, 0xf, 0xf, false); v = lru_compose(t, v);
  t = (u32) __builtin_amdgcn_update_dpp((int) LRU_ID, (int) v, 0x118, 0xf, 0xf, false); v = lru_compose(t, v);
  t = (u32) __builtin_amdgcn_update_dpp((int) LRU_ID, (int) v, 0x142, 0xa, 0xf, false); v = lru_compose(t, v);
  t = (u32) __builtin_amdgcn_update_dpp((int) LRU_ID, (int) v, 0x143, 0xc, 0xf, false); v = lru_compose(t, v);
  return v;
}
