// lzx_pipe.hpp -- what the tasks of the frame-parallel path (mspack_lzx_pipe, entry_kernels.hpp) share: the frame record and its
// status word, the hand-off (lzx_status_load / lzx_status_publish), the trace macros of LZX_PIPE_TRACE builds, lzx_seek_bit
// and lzx_side_setup.  Compiled into lzxn (resolve tasks, the unit decoder's resume) and lzxp (parse tasks).  Nothing of the
// reference corresponds to it: lzxd.c decodes a stream front to back; what makes frames independent is lzxd.c:695-697.

// ---------------------------------------------------------------------------------------------------
// Frame-level parse parallelism (plain LZX; units that carry a frame table, MSPACK_HIP_UF_FRAME_TABLE).
//
// Every 32 KiB frame starts on a 16-bit boundary of the compressed stream (lzxd.c:695-697) at an offset the
// container states up front -- one CFDATA block per frame in a cabinet (cabd.c:1362-1479), one reset-table
// entry per frame in a CHM (chmd.c:1146-1149).  The serial chain of a unit is "where does the next token
// start"; it needs the Huffman tables, not the window and not R0-R2.  So mspack_lzx_pipe gives every FRAME a parse
// task (lzx_pipe_parse): it waits for the code lengths of the frame before it (code lengths are deltas on the previous
// block's, lzxd.c:138-183: a chain, but a short one -- one header per link), reads its own block header, publishes
// its code lengths, builds the tables and parses the frame's tokens with every lane walking its own stretch of the bits
// (lzx_parse_emit): literals go straight to the output, matches become 8-byte records in the launch's record pool.
// Rounds 2-4 parsed on the guess that every frame holds exactly ONE verbatim / aligned block that begins where the frame
// begins -- what this build's own encoder writes.  Microsoft's encoder does not: the reference's large-files cabinets hold
// blocks of megabytes (8 384 624 bytes, 7 379 562 ...), so their frames lie INSIDE a block, and the guess failed for every
// frame of every real cabinet tried (they all took the serial path: 180 MB/s).  Round 5: the chain from frame to frame is
// "code lengths + what is left of the open block"; a frame inside a block inherits both and has no header to read, a frame
// that holds a block's end parses up to it, reads the next header there and goes on with the new tables (lzx_pipe_parse).
// Stored blocks, a block that ends where nothing can be parsed, damage: the task gives up silently.  A resolve task per frame (lzx_pipe_resolve) then
// turns the records into copies in stream order: R0-R2, the reference's checks, the match queue.  Whatever the tasks
// do not cover -- the last bytes of the input, a frame with several blocks, stored blocks, a damaged stream, a wrong
// table -- ends the unit's chain there (rs_* in the unit's first record) and is decoded by the serial path
// (mspack_decode_lzx, resume) from that very bit, so error codes and byte counts cannot differ.
// ---------------------------------------------------------------------------------------------------

struct __align__(16) LzxFrameRec {
  u32 status;                       /* LZX_ST_*: 2 = header known (code lengths published), 7 = literals stored, records written */
  u32 n_tokens;
  u32 hdr_start_bit;                /* bit positions count from the unit's first compressed byte */
  u32 end_bit;                      /* first bit that was not parsed */
  u32 block_type, block_length;
  u32 flags;                        /* 1: the length tree is empty, 2: literal 0xE8 has a code */
  u32 prog;                         /* mspack_lzx_pipe, while status is 2: match records | output bytes << 15 that are in memory
                                       already (published after every pass of lzx_parse_emit but the last) */
  u8 ali_len[8];
  u32 rem_out;                      /* lzx_pipe_parse: bytes of the block that is open BEHIND this frame (0: the next frame starts with a
                                       block header).  Published with the code lengths (status 2): the next frame's task inherits both */
  u32 run_rem;                      /* what a decoder that goes on INSIDE this frame (a record that ends early) has as block_remaining
                                       at the frame's first byte, counting the block the record ends in as if it had begun there */
  u8 main_len[LZX_MAIN_SYMS + 16];
  u8 len_len[LZX_LEN_SYMS + 70];
  /* ---- mspack_lzx_pipe (lzx_pipe_parse / lzx_pipe_commit) ---- */
  u32 frame_start_bit;              /* where the frame begins: in front of a reset interval's 1 + 32 header bits */
  u32 intel_filesize;               /* the interval header's value when this frame carries it (else 0) */
  u32 bytes_done;                   /* output bytes the record covers (== the frame's size: a complete frame) */
  u32 n_edge;                       /* literals kept in edge_lit (the frame's first bytes share a cache line with the
                                       bytes below them, which another wave may be writing: the commit wave stores them) */
  u32 edge_mask[4];
  /* what the unit's commit task leaves for mspack_decode_lzx: where serial decoding resumes (in the unit's FIRST record) */
  u32 rs_valid, rs_frame, rs_partial, rs_P, rs_next_bit, rs_R0, rs_R1, rs_R2;
  u8 edge_lit[128];
  /* the unit's chain of frames (lzx_pipe_resolve): 0 = open, 1 = this frame and every frame before it are complete in the
   * output (cR0-cR2: R0-R2 behind its last match), 2 = the chain ended at or before this frame */
  u32 chain, cR0, cR1, cR2;
  /* lzx_fold.hpp: R0-R2 behind the frame's last match, published as soon as they are known -- long before its bytes are
   * final (rst: 0 open, 1 valid, 2 the chain ends at or before this frame) */
  u32 rst, rR0, rR1, rR2;
  u8 pad2[16];
  u32 chunk[REC_CHUNKS];            /* where the frame's match records are: wave_common.hpp, RecPool */
};
static_assert(sizeof(LzxFrameRec) == 1408, "LzxFrameRec layout");
// LzxFrameRec::status.  The separate header / parse launches only use 0, 2, 1.  In the dependency-driven launch
// (mspack_lzx_pipe, entry_kernels.hpp) the word is also the hand-off flag between the frame's parse task and the unit's wave:
//   0 untouched | 5 a parse wave claimed the frame | 2 its code lengths are in the record, tokens still being parsed |
//   1 tokens parsed (final) | 3 code lengths valid, no tokens (final) | 4 nothing usable (final; the chain of code
//   lengths is broken for the rest of the reset interval) | 6 the unit's own wave took the frame (decodes it serially)
#ifdef LZX_PIPE_TRACE      /* analysis builds: time a unit task spends waiting for parse tasks (entry_kernels.hpp: g_pipe_trace) */
__device__ unsigned long long g_pipe_wait[1 << 16];
__device__ unsigned long long g_pipe_phase[16];     /* summed over all waves: s_memrealtime ticks per phase (PH below) */
/* (accumulated in registers, added to the global sums once per task: an atomic per stamp would serialise the waves) */
#define PHDECL() u32 pha_[16] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }
#define PH0() unsigned long long ph_ = __builtin_amdgcn_s_memrealtime()
#define PH(k) do { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); pha_[k] += (u32)(n_ - ph_); ph_ = n_; } while (0)
#define PHE0() unsigned long long phe_ = __builtin_amdgcn_s_memrealtime()
#define PHE(k) do { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); d.st_t[k] += (u32)(n_ - phe_); phe_ = n_; } while (0)
#define PHFLUSH() do { if (threadIdx.x == 0) for (int k_ = 0; k_ < 16; k_++) if (pha_[k_]) atomicAdd(&g_pipe_phase[k_], (unsigned long long) pha_[k_]); } while (0)
#define PHCNT(k, n) do { d.st_t[k] += (n); } while (0)       /* (12..15: counts, not times -- steps of the count walks, rounds, steps of the last walk, passes) */
#else
#define PHDECL() do { } while (0)
#define PHE0() do { } while (0)
#define PHE(k) do { } while (0)
#define PHCNT(k, n) do { } while (0)
#define PH0() do { } while (0)
#define PH(k) do { } while (0)
#define PHFLUSH() do { } while (0)
#endif
#ifdef LZX_PIPE_TRACE
#define LZX_PIPE_WAIT_BEGIN() const unsigned long long pw_ = __builtin_amdgcn_s_memrealtime()
#define LZX_PIPE_WAIT_END() do { if (threadIdx.x == 0) g_pipe_wait[blockIdx.x & 0xFFFFu] += __builtin_amdgcn_s_memrealtime() - pw_; } while (0)
#else
#define LZX_PIPE_WAIT_BEGIN() do { } while (0)
#define LZX_PIPE_WAIT_END() do { } while (0)
#endif
#define LZX_ST_NONE 0u
#define LZX_ST_PARSED 1u
#define LZX_ST_HEADER 2u
#define LZX_ST_HDRONLY 3u
#define LZX_ST_FAILED 4u
#define LZX_ST_CLAIMED 5u
#define LZX_ST_TAKEN 6u
#define LZX_ST_EMITTED 7u         /* lzx_pipe_parse: literals stored, match records written (final) */
/* a match record of lzx_pipe_parse (uint2): x = position in the unit's output, y = offset << 11 | length << 2 | which:
 * 0 explicit offset, 1..3 repeat of R0 / R1 / R2 (lzxd.c:565-586) */
__device__ __forceinline__ u32 lzx_status_load(const u32 *p) {
  return rfl(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// publish what this wave stored (tokens, record fields), then the status word: agent-scope release, a drained
// store queue (the compiler may drop the wait behind the write-back: MI355X guide, hand-off recipe), relaxed flag
__device__ __forceinline__ void lzx_status_publish(u32 *p, const u32 v, const u32 lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#ifndef MSPACK_WAVE_EMU
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  if (lane == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// continue reading at an absolute bit position (from the unit's first byte)
__device__ __forceinline__ void lzx_seek_bit(LzxDec &d, const u32 abs_bit)
{
  const u32 par = d.w.origin & 1u;                       // 16-bit words start at bytes of this parity
  const u32 wbyte = ((((abs_bit >> 3) - par) >> 1) << 1) + par;
  const u32 sk = abs_bit - wbyte * 8u;
  d.w.seek(wbyte, d.lane);
  d.bb = 0; d.bl = 0; d.rbl = 0;
  d.near_end = (wbyte >= d.w.in_len || d.w.in_len - wbyte <= 64u);
  d.refill(); d.refill();
  if (sk) { d.bb <<= sk; d.bl -= (int) sk; }
}


// common set-up of the header wave and the parse waves: a decoder on the unit's input, nothing read yet
__device__ __forceinline__ bool lzx_side_setup(LzxDec &d, LzxState &s, const mspack_hip_unit &u, const u8 *in_arena, LzxShared *sh)
{
  d.lane = threadIdx.x; d.sh = sh; d.err = 0;
  d.w.unit = in_arena + u.in_off; d.w.in_len = u.in_len;
  d.w.eofs = (u.flags & MSPACK_HIP_UF_HARD_EOF) ? 0u : 2u;
  d.out = nullptr; d.P = 0; d.lit_buf = 0; d.lit_n = 0;
  for (int k_ = 0; k_ < 10; k_++) d.st_t[k_] = 0;
  d.bb = 0; d.bl = 0; d.rbl = 0; d.near_end = false; d.careful = false;
  d.w.origin = 0; d.w.wi = 0; d.w.cur = 0; d.w.nxt = 0;
  s.wsize = 1u << u.window_bits;
  s.wpos = 0; s.frame_posn = 0; s.frame = 0; s.reset_frames = u.reset_frames;
  s.offset = 0; s.length = u.out_len;
  s.intel_filesize = 0; s.intel_started = false; s.length_empty = false;
  s.raw_mode = false; s.raw_pos = 0; s.ref_size = 0;
  s.R0 = s.R1 = s.R2 = 1; s.header_read = false; s.block_remaining = 0; s.block_type = 0; s.block_length = 0;
  static const u16 slots[11] = { 30, 32, 34, 36, 38, 42, 50, 66, 98, 162, 290 };
  const u32 wb = u.window_bits;
  s.num_offsets = (wb >= 15u && wb <= 21u) ? ((u32) slots[wb - 15u] << 3) : 0u;
  return s.num_offsets != 0u;
}
