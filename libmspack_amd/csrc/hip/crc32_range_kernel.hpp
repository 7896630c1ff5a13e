// crc32_range_kernel.hpp -- MSPACK_HIP_KIND_CRC32: the CRC-32 (zlib's convention) of a byte range of the output arena, at any length.
//
// The arithmetic is crc32_kernel.hpp's, unchanged: a range's bytes as aligned 16-byte rows with a masked head, 64 KiB segments, one
// wavefront per segment (crc_segment), a segment's share = its raw value times x^(8 * bytes behind it in its range).  What is new
// is the WORK SPLIT.  Ranges are files: 0 bytes to gigabytes, a hundred thousand of them in one list, a few of them most of the bytes.
//
//   ticket space   the segments of ALL ranges of the list, range after range in list order, numbered 0 .. T - 1 (64-bit: ranges
//                  may overlap, so T is not bounded by the arena).  Waves take CHUNKS of K consecutive tickets from one counter
//                  (K from T and the grid: about four chunks per wave, so the 4 KiB table build and the search below are paid
//                  once per several segments) until the counter is past the end; then they leave.  A 2 GiB range beside 100 000
//                  short ones is 32 768 tickets among 132 768: it spreads over the chip like everything else.
//   blocks         the list is read 64 positions at a time (a "block": one position per lane).  Within a block the tickets'
//                  owners follow from a wave scan of the lanes' segment counts -- nothing stored.  ACROSS blocks a wave needs the
//                  tickets in front of a block: P[b], 64-bit.  mspack_crc32r_scan, ONE wave in front of the pass, walks the
//                  blocks once and leaves P[b] in the spare result words (good_len, in_next) of block b's first range unit.
//                  A chunk's first ticket is found by a binary search over the blocks (a probe = one block read + P of its first
//                  unit; a block without range units is stepped over downwards); the chunk's other tickets by walking on.
//   control        the FIRST range unit of the list has P = 0 by construction, so its three spare words are free: in_used is
//                  the chunk counter, (good_len, in_next) hold T.  Every wave finds it by reading blocks from the front (the
//                  host path's lists hold range units only: the first block).
//   no waiting     no wave reads anything another wave of the same launch writes, except through the two atomics (the counter,
//                  the XOR into result.out_len).  Launch boundaries order the rest: init (results, the start value's affine
//                  term XOR 0xFFFFFFFF -- zlib's final inversion for free), scan, pass, finish (the spare words back to 0).
//
// A unit whose range leaves out_bytes is no range unit for any of this: init answers MSPACK_ERR_ARGS with zeros, nothing of it is
// read, it owns no ticket and no scratch.  Every read of the arena is bounded by a range that was checked against out_bytes in the
// same wave (a block read re-derives everything from the unit table; the scratch words only say WHERE in the ticket space a block
// stands: wrong ones would give wrong checksums, never a read outside a checked range).
#pragma once
#include "crc32_kernel.hpp"

#define CRC32R_MIN_CHUNK 16u           /* tickets per chunk once there are enough of them: one search per >= 16 segments */

// the pass's two atomics, agent scope, relaxed (tests/emu: the host compiler's)
#ifdef MSPACK_WAVE_EMU
static inline u32 crc32r_fetch_xor(u32 *p, u32 v) { return __atomic_fetch_xor(p, v, __ATOMIC_RELAXED); }
static inline u32 crc32r_fetch_add(u32 *p, u32 v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ u32 crc32r_fetch_xor(u32 *p, u32 v) { return __hip_atomic_fetch_xor(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u32 crc32r_fetch_add(u32 *p, u32 v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

// what a lane knows of its position of the list: plain loads, no cross-lane operation (so several blocks' loads can be in flight)
struct Crc32rLane { u32 ui, len; u64 off; bool is_crc, part; };      // is_crc: a unit of the kind; part: ... whose range lies inside out_bytes
__device__ __forceinline__ Crc32rLane crc32r_lane(const mspack_hip_unit *units, const u32 *order, const u32 n, const u32 b, const u64 out_bytes, const u32 lane)
{
  Crc32rLane r; r.ui = 0u; r.len = 0u; r.off = 0u; r.is_crc = false; r.part = false;
  const u64 j = (u64) b * 64u + lane;
  if (j >= n) return r;
  r.ui = order ? gld(order + j) : (u32) j;
  const mspack_hip_unit *u = units + r.ui;
  if (gld(&u->kind) != MSPACK_HIP_KIND_CRC32) return r;
  r.is_crc = true;
  r.off = gld(&u->out_off); r.len = gld(&u->out_len);
  r.part = r.off <= out_bytes && (u64) r.len <= out_bytes - r.off;
  return r;
}
// segments of a range: its bytes and the `head` bytes in front that share its first 16-byte row
__device__ __forceinline__ u32 crc32r_head(const u8 *out_arena, const u64 off) { return (u32)((size_t)(out_arena + off) & 15u); }
__device__ __forceinline__ u32 crc32r_nseg(const u8 *out_arena, const Crc32rLane &r)
{
  if (!r.part || r.len == 0u) return 0u;
  return (u32)(((u64) r.len + crc32r_head(out_arena, r.off) + CRC_SEG - 1u) / CRC_SEG);
}
// a block as the wave sees it: per lane the unit, its first ticket inside the block and its tickets; uniform: the range units'
// lanes, the block's tickets
struct Crc32rBlock { Crc32rLane r; u32 nseg, lpfx; u64 parts; u32 total; };
__device__ __forceinline__ Crc32rBlock crc32r_block(const Crc32rLane &r, const u8 *out_arena)
{
  Crc32rBlock k; k.r = r;
  k.nseg = crc32r_nseg(out_arena, r);
  const u32 incl = wave_incl_scan(k.nseg);
  k.lpfx = incl - k.nseg;
  k.total = rdl(incl, 63u);
  k.parts = ballot(r.part);
  return k;
}
__device__ __forceinline__ u32 crc32r_first_unit(const Crc32rBlock &k) { return rdl(k.r.ui, (u32) __ffsll((long long) k.parts) - 1u); }
__device__ __forceinline__ u64 crc32r_read64(const mspack_hip_result *res) { return (u64) rfl(gld(&res->good_len)) | ((u64) rfl(gld(&res->in_next)) << 32); }

// ---- launch 1: every range unit's result (one per lane).  out_len = 0xFFFFFFFF * x^(8n) ^ 0xFFFFFFFF: the start value's share with
// zlib's final inversion already in it (0 for n == 0); the spare words 0 ----
__device__ __forceinline__ void crc32r_init_lane(const mspack_hip_unit *units, const u32 *order, const u32 n, const u64 out_bytes, mspack_hip_result *results)
{
  const Crc32rLane r = crc32r_lane(units, order, n, blockIdx.x, out_bytes, threadIdx.x);
  if (!r.is_crc) return;
  mspack_hip_result o;
  o.err = r.part ? ERR_OK : ERR_ARGS; o.flags = 0u; o.out_len = 0u; o.in_used = 0u; o.good_len = 0u; o.in_next = 0u;
  if (r.part) {
    u32 v = 0xFFFFFFFFu;
    for (u32 k = 0; k < 32u && (r.len >> k) != 0u; k++)
      if ((r.len >> k) & 1u) v = crc_mulmod(v, crc_x2n8[k]);
    o.out_len = v ^ 0xFFFFFFFFu;
  }
  gst(&results[r.ui], o);
}

// ---- launch 2: ONE wave.  P[b] into the first range unit of every block that has one; T into the control unit ----
__device__ __forceinline__ void crc32r_scan_wave(const mspack_hip_unit *units, const u32 *order, const u32 n, const u8 *out_arena, const u64 out_bytes,
                                                 mspack_hip_result *results)
{
  const u32 lane = threadIdx.x;
  const u32 B = (u32)(((u64) n + 63u) / 64u);
  u64 P = 0;
  bool have_ctl = false;
  u32 ctl = 0;
  for (u32 b0 = 0; b0 < B; b0 += 4u) {
    Crc32rLane raw[4];
#pragma unroll
    for (u32 q = 0; q < 4u; q++) raw[q] = crc32r_lane(units, order, n, b0 + q, out_bytes, lane);      // (beyond B: no position is < n)
#pragma unroll
    for (u32 q = 0; q < 4u; q++) {
      const Crc32rBlock k = crc32r_block(raw[q], out_arena);
      if (k.parts == 0ull) continue;
      const u32 fu = crc32r_first_unit(k);
      if (!have_ctl) { have_ctl = true; ctl = fu; }              // (P == 0 here: its words are the control's)
      else if (lane == 0) { gst(&results[fu].good_len, (u32) P); gst(&results[fu].in_next, (u32)(P >> 32)); }
      P += k.total;
    }
  }
  if (have_ctl && lane == 0) { gst(&results[ctl].good_len, (u32) P); gst(&results[ctl].in_next, (u32)(P >> 32)); }
}

// ---- launch 3: the pass ----
// tickets per chunk: about four chunks per wave of the grid, at least CRC32R_MIN_CHUNK once every wave has that many; the chunk
// count stays far below 2^32 (T < 2^49, K >= T / (4 * waves))
__device__ __forceinline__ u64 crc32r_chunk(const u64 T, const u32 waves)
{
  const u64 w = waves ? waves : 1u;
  u64 K = (T + 4u * w - 1u) / (4u * w);
  const u64 per_wave = (T + w - 1u) / w;
  const u64 floor_k = per_wave < CRC32R_MIN_CHUNK ? per_wave : CRC32R_MIN_CHUNK;
  if (K < floor_k) K = floor_k;
  return K ? K : 1u;
}
// segment s of the range (off, len): its share of the range's raw value
__device__ __forceinline__ u32 crc32r_share(const u8 *out_arena, const u64 off, const u32 len, const u32 s, const CrcShared *sh, const u32 lane)
{
  const u8 *p = out_arena + off;
  const u32 head = (u32)((size_t) p & 15u);
  const u8 *row0 = p - head;
  const u64 nv = (u64) len + head;
  const u64 vlo = (u64) s * CRC_SEG, vhi = vlo + CRC_SEG < nv ? vlo + CRC_SEG : nv;
  u32 c = crc_segment(row0, head, vlo, vhi, sh, lane);
  const u32 behind = (u32)(nv - vhi);
  if (behind) c = crc_mulmod(c, crc_xpow8(behind, lane));
  return c;
}
__device__ __forceinline__ void crc32r_pass_wave(const mspack_hip_unit *units, const u32 *order, const u32 n, const u8 *out_arena, const u64 out_bytes,
                                                 mspack_hip_result *results, CrcShared *sh)
{
  const u32 lane = threadIdx.x;
  const u32 B = (u32)(((u64) n + 63u) / 64u);
  // the control unit: the first range unit of the list
  u32 b_ctl = 0, ctl = 0;
  Crc32rBlock k;
  for (;; b_ctl++) {
    if (b_ctl >= B) return;                                     // no range unit at all
    k = crc32r_block(crc32r_lane(units, order, n, b_ctl, out_bytes, lane), out_arena);
    if (k.parts) { ctl = crc32r_first_unit(k); break; }
  }
  const u64 T = crc32r_read64(&results[ctl]);
  if (T == 0ull) return;
  const u64 K = crc32r_chunk(T, gridDim.x);
  u32 *const counter = &results[ctl].in_used;
  bool tables = false;
  for (;;) {
    u32 c = 0;
    if (lane == 0) c = crc32r_fetch_add(counter, 1u);
    c = rfl(c);
    const u64 t0 = (u64) c * K;
    if (t0 >= T) return;                                        // the counter is past the end
    const u64 t1 = t0 + K < T ? t0 + K : T;
    if (!tables) { crc_build_tables(sh, lane); tables = true; }
    // the block that holds ticket t0: P[b] <= t0 < P[b] + total[b]
    u32 lo = b_ctl, hi = B - 1u, b = b_ctl;
    u64 P = 0;
    for (;;) {
      const u32 mid = lo + (hi - lo) / 2u;
      bool any = false;
      for (b = mid;; b--) {                                     // the nearest block at or below mid that has a range unit
        k = crc32r_block(crc32r_lane(units, order, n, b, out_bytes, lane), out_arena);
        if (k.parts) { any = true; break; }
        if (b == lo) break;
      }
      if (!any) { if (mid >= hi) return; lo = mid + 1u; continue; }
      const u32 fu = crc32r_first_unit(k);
      P = fu == ctl ? 0ull : crc32r_read64(&results[fu]);
      if (t0 < P) { if (b == lo) return; hi = b - 1u; }
      else if (t0 - P < k.total) break;
      else { if (mid >= hi) return; lo = mid + 1u; }
    }
    // walk: ticket t = P + o of block b
    u32 o = (u32)(t0 - P);
    u32 acc = 0, acc_ui = 0;
    bool acc_any = false;
    for (u64 t = t0; t < t1; t++) {
      while (o >= k.total) {                                    // on to the next block that has tickets
        o = 0;
        if (++b >= B) break;
        k = crc32r_block(crc32r_lane(units, order, n, b, out_bytes, lane), out_arena);
      }
      if (b >= B) break;
      const u64 own = ballot(o >= k.lpfx && o - k.lpfx < k.nseg);
      if (own == 0ull) break;
      const u32 l = (u32) __ffsll((long long) own) - 1u;
      const u32 ui = rdl(k.r.ui, l), len = rdl(k.r.len, l), s = o - rdl(k.lpfx, l);
      const u64 off = (u64) rdl((u32) k.r.off, l) | ((u64) rdl((u32)(k.r.off >> 32), l) << 32);
      if (acc_any && ui != acc_ui) {
        if (lane == 0 && acc) crc32r_fetch_xor(&results[acc_ui].out_len, acc);
        acc = 0;
      }
      acc_any = true; acc_ui = ui;
      acc ^= crc32r_share(out_arena, off, len, s, sh, lane);
      o++;
    }
    if (acc_any && lane == 0 && acc) crc32r_fetch_xor(&results[acc_ui].out_len, acc);
  }
}

// ---- launch 4: the spare words of every range unit back to 0 (one per lane) ----
__device__ __forceinline__ void crc32r_finish_lane(const mspack_hip_unit *units, const u32 *order, const u32 n, const u64 out_bytes, mspack_hip_result *results)
{
  const Crc32rLane r = crc32r_lane(units, order, n, blockIdx.x, out_bytes, threadIdx.x);
  if (!r.part) return;
  gst(&results[r.ui].in_used, 0u); gst(&results[r.ui].good_len, 0u); gst(&results[r.ui].in_next, 0u);
}
