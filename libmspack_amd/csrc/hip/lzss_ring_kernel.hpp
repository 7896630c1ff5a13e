// lzss_ring_kernel.hpp -- LZSS units that carry MSPACK_HIP_UF_LZSS_RING: one wavefront per stream, the 4096-byte window in LDS.
//
// lzss_kernel.hpp decodes into a "linear window": the 4096 bytes below the unit's output are its pre-fill, and every control byte,
// item and match is a dependent access to global memory.  For the batches the SZDD / KWAJ prefetch calls build -- thousands of
// streams of 5 to 30 KiB -- that is 4 KiB of padding per file and a chain of global round trips per group.  Here
//   * the window is the reference's own ring (lzssd.c:36-91): 4096 bytes of LDS filled with spaces, written at the ring positions the
//     stream names (start 4096-16, QBASIC 4096-18), copies byte-serial -- a source that overlaps its destination is periodic;
//   * the input is staged through LDS in blocks of LZR_STAGE bytes, one aligned 16-byte load per lane; a block is refilled when
//     fewer bytes are left than one step can consume (LZR_GROUPS groups of at most 17 bytes) and the stream goes on behind it;
//   * a step takes LZR_GROUPS control groups: lanes 8g..8g+7 own group g, the group starts are a scalar chain over the staged bytes
//     (held in registers, read with v_readlane: no memory latency on the chain);
//   * the output leaves LDS as whole aligned 16-byte rows of the unit's region, before the step that could overwrite them; the
//     ragged head and tail of the region go out as byte stores; bytes beyond the room (unit.out_len) are dropped.
// The unit owns nothing below out_off.  Results are those of lzss_decode_unit.
// LDS: 4096 (ring) + 1024 + 192 (stage and the read-ahead behind its last block) = 5312 bytes per wave.
#pragma once
#include "lzss_kernel.hpp"

#define LZR_GROUPS     8u                          /* control groups per step: 64 items, one per lane */
#define LZR_STEP_IN    (17u * LZR_GROUPS)          /* most input bytes a step consumes */
#define LZR_STEP_OUT   (18u * 8u * LZR_GROUPS)     /* most output bytes a step produces */
#define LZR_STAGE      1024u                       /* staged input: 64 lanes x 16 bytes */
#define LZR_STAGE_MORE 192u                        /* room the chain's window may read behind the stage's last block (never used as data) */

struct __align__(16) LzssRingShared {
  uint4 ring[LZSS_WINDOW / 16u];
  uint4 stage[(LZR_STAGE + LZR_STAGE_MORE) / 16u];
};

// output bytes [F, E) from the ring to the unit's region (E - F <= 4096, all of them still in the ring); F = E afterwards
__device__ __forceinline__ void lzr_flush(const u8 *ring, u8 *out, u32 start, u32 &F, u32 E, u32 cap, u32 lane)
{
  if (F >= cap) { F = E; return; }                       // (beyond the room: dropped)
  const u32 a = (u32)((u64) out & 15u);
  u32 hb = (16u - ((a + F) & 15u)) & 15u;                // ragged head: up to the region's next 16-byte row
  if (hb > E - F) hb = E - F;
  if (lane < hb && F + lane < cap) out[F + lane] = ring[(start + F + lane) & 4095u];
  F += hb;
  const u32 nrows = (E - F) >> 4;
  const u32 *ring32 = (const u32 *) ring;
  const u32 sh = (start + F) & 3u;                       // the rows' misalignment in the ring (wave-uniform)
  for (u32 r = lane; r < nrows; r += WAVE) {
    const u32 k0 = F + 16u * r;
    if (k0 >= cap) continue;
    if (cap - k0 >= 16u) {
      const u32 b = ((start + k0) & 4095u) >> 2;
      const u32 d0 = ring32[b], d1 = ring32[(b + 1u) & 1023u], d2 = ring32[(b + 2u) & 1023u], d3 = ring32[(b + 3u) & 1023u],
                d4 = ring32[(b + 4u) & 1023u];
      gst_row((uint4 *)(out + k0), make_uint4(__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                                               __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)));
    }
    else for (u32 k = k0; k < cap; k++) out[k] = ring[(start + k) & 4095u];      // the row the room ends in
  }
  F += 16u * nrows;
  if (lane < E - F && F + lane < cap) out[F + lane] = ring[(start + F + lane) & 4095u];      // ragged tail
  F = E;
}

__device__ void lzss_ring_decode_unit(const mspack_hip_unit &u, const u8 *in_arena, u8 *out_arena, mspack_hip_result *res,
                                      LzssRingShared *sh)
{
  const u32 lane = threadIdx.x;
  const u32 in_len = u.in_len, mode = u.window_bits, cap = u.out_len;      // 0 EXPAND, 1 MSHELP, 2 QBASIC (lzssd.c:49-51)
  if (mode > 2u) { if (lane == 0) { res->err = ERR_ARGS; res->flags = 0; res->out_len = 0; res->in_used = 0; res->good_len = 0; res->in_next = 0; } return; }
  u8 *const ring = (u8 *) sh->ring;
  const u8 *const stage = (const u8 *) sh->stage;
  const u32 *const stage32 = (const u32 *) sh->stage;
  for (u32 k = lane; k < LZSS_WINDOW / 16u; k += WAVE) sh->ring[k] = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
  const u64 A = (u64)(in_arena + u.in_off);
  u8 *const out = out_arena + u.out_off;
  const u32 start = LZSS_WINDOW - (mode == 2u ? 18u : 16u);   // ring position of the first output byte
  const u32 invert = (mode == 1u) ? 0xFFu : 0u;
  const u32 a = (u32)((u64) out & 15u);
  u32 ip = 0, P = 0, F = 0;                              // input offset, bytes produced, bytes that have left the ring
  long long sofs = 0, shi = 0;                           // the stage holds the input offsets [sofs, shi)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  while (ip < in_len) {
    if ((long long) ip + (long long) LZR_STEP_IN > shi && shi < (long long) in_len) {
      // refill: the 1024 bytes from the 16-byte row that holds `ip` on (what is left of the old block comes again)
      const u64 SA = (A + ip) & ~15ull;
      sofs = (long long)(SA - A);
      shi = sofs + (long long) LZR_STAGE;
      const u64 row = SA + 16u * lane;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row < A + in_len) v = *(const uint4 *) row;
      sh->stage[lane] = v;
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    if (P - F > LZSS_WINDOW - LZR_STEP_OUT) {            // this step could overwrite bytes that have not left: whole rows go
      lzr_flush(ring, out, start, F, P - ((a + P) & 15u), cap, lane);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    // the step's input window in registers: lane l holds the dword at stage offset (si & ~3) + 4 l
    const u32 si = (u32)((long long) ip - sofs);
    const u32 wv = lane < (LZR_STEP_IN + 3u + 3u) / 4u ? stage32[(si >> 2) + lane] : 0u;
    u32 pos = ip, bi = si & 3u, myc = 0, mypos = 0;
#pragma unroll
    for (u32 g = 0; g < LZR_GROUPS; g++) {               // the scalar chain of group starts
      const u32 c = ((rdl(wv, bi >> 2) >> (8u * (bi & 3u))) ^ invert) & 0xFFu;
      if ((lane >> 3) == g) { myc = c; mypos = pos; }
      const u32 adv = 9u + (u32) __popc((~c) & 0xFFu);   // the control byte, a byte per literal, two per match
      pos += adv; bi += adv;
    }
    const u32 i = lane & 7u;
    const u32 ioff = mypos + 1u + i + (u32) __popc((~myc) & ((1u << i) - 1u));
    const bool lit = (myc >> i) & 1u;
    const u32 need = lit ? 1u : 2u;
    const bool have = (u64) ioff + need <= (u64) in_len;      // ENSURE_BYTES before every byte (lzssd.c:15-28)
    u32 b0 = 0, b1 = 0;
    if (have) { const u32 s = (u32)((long long) ioff - sofs); b0 = stage[s]; if (!lit) b1 = stage[s + 1u]; }
    // the first incomplete item ends the stream; items before it are complete
    const u64 okm = ballot(have);
    const u32 nitems = okm == ~0ull ? 64u : (u32) __builtin_ctzll(~okm);
    const u32 olen = lane < nitems ? (lit ? 1u : (b1 & 0x0Fu) + 3u) : 0u;
    const u32 incl = wave_incl_scan(olen);
    const u32 rpos = (start + P + incl - olen) & 4095u;  // ring position of the item's first byte
    // items in stream order: a match may read what an earlier item of this step wrote, and what a LATER item is about to
    // overwrite (a source almost 4096 back) -- so the literals in front of a match are stored before it, the others after it
    bool lit_todo = olen != 0u && lit;
    for (u64 m1 = ballot(olen != 0u && !lit); m1; m1 &= m1 - 1ull) {
      const u32 j = (u32) __ffsll((long long) m1) - 1u;
      if (lit_todo && lane < j) { ring[rpos] = (u8) b0; lit_todo = false; }
      const u32 rj = rdl(rpos, j), lj = rdl(olen, j), mp = rdl(b0, j) | ((rdl(b1, j) & 0xF0u) << 4);
      const u32 d = ((rj - mp - 1u) & 4095u) + 1u;       // 1..4096
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      u32 v = 0;
      if (lane < lj) {
        u32 kk = lane;
        while (kk >= d) kk -= d;                         // periodic source: only bytes that existed before
        v = ring[(mp + kk) & 4095u];
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      if (lane < lj) ring[(rj + lane) & 4095u] = (u8) v;
    }
    if (lit_todo) ring[rpos] = (u8) b0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    P += rdl(incl, 63);
    if (nitems < 64u) { ip = in_len; break; }
    ip = pos;
  }
  lzr_flush(ring, out, start, F, P, cap, lane);
  if (lane == 0) {
    res->err = ERR_OK; res->flags = 0; res->out_len = P; res->good_len = P;
    res->in_used = ip; res->in_next = 0;
  }
}
