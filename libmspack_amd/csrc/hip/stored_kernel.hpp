// stored_kernel.hpp -- MSPACK_HIP_KIND_STORED: CAB method 0 ("not compressed", noned_decompress, cabd.c:1500-1542) as a unit -- the
// first min(in_len, out_len) bytes of the unit's input copied to [out_off, ...) of the output arena, at any alignment of either.
//
// Units are folders: 0 bytes to 2 GiB, thousands of them in one list, a few of them most of the bytes.  The WORK SPLIT is
// crc32_range_kernel.hpp's, with a copy where that file takes a checksum:
//
//   segments       a unit's bytes as ALIGNED 16-byte rows of the OUTPUT arena (`head` = the bytes below out_off that share its first
//                  row), cut every STORED_SEG = 64 KiB of that row stream: a whole segment is 4096 rows, 64 per lane.
//   ticket space   the segments of ALL stored units of the list, unit after unit in list order, numbered 0 .. T - 1 (64-bit).  Waves
//                  take chunks of K consecutive tickets from one counter (crc32r_chunk: about four chunks per wave) until the counter
//                  is past the end; then they leave.  One 2 GiB folder beside 100 000 short ones is 32 768 tickets among 132 768.
//   blocks         the list is read 64 positions at a time; within a block the tickets' owners follow from a wave scan of the lanes'
//                  segment counts, across blocks from P[b], the tickets in front of block b.  mspack_stored_scan, ONE wave in front of
//                  the pass, leaves P[b] in two result words (good_len, in_next) of block b's first stored unit.  A chunk's first ticket
//                  is found by a binary search over the blocks, the chunk's other tickets by walking on.
//   control        the FIRST stored unit of the list has P = 0 by construction: its in_used is the chunk counter (the scan sets it to
//                  0), its (good_len, in_next) hold T.
//   results        mspack_stored_results, the LAST launch, writes every stored unit's whole result (one unit per lane) -- the words the
//                  run borrowed hold their final values when it ends.  Precondition, as for the CRC-32 range pass: the order list names
//                  no stored unit twice (two places of the list would share one unit's words: bytes of those units could be copied
//                  twice or not at all -- every access stays inside the checked ranges).
//   no waiting     no wave reads anything another wave of the same launch writes, except through the one atomic (the chunk counter,
//                  relaxed, agent scope).  Launch boundaries order the rest: scan, pass, results.  Every loop is bounded by the unit
//                  table: blocks of the list, tickets of a chunk, rows of a segment.
//
// A unit whose input leaves in_bytes or whose output leaves out_bytes is no stored unit for any of this: MSPACK_ERR_ARGS with zeros,
// nothing of it is read or written, it owns no ticket and no scratch.  Every arena access is bounded by a range that was checked
// against in_bytes / out_bytes in the same wave (a block read re-derives everything from the unit table; the scratch words only say
// WHERE in the ticket space a block stands).
//
// The copy.  Whole rows are ALIGNED 16-byte stores, 64 consecutive rows per wave instruction (1 KiB), four independent rows in flight
// per lane.  Their sixteen source bytes lie at (in_off - out_off) mod 16 = sh inside an aligned source row: sh == 0 is one aligned
// 16-byte load; otherwise the two aligned source rows around them are loaded and shifted together in registers (v_alignbyte; sh is
// wave-uniform).  Both of those rows hold at least one byte of the unit's input; one that reaches below the unit's first or beyond its
// last input byte is read as two 8-byte halves, each only if it holds a byte of the unit -- at most 7 bytes next to the unit's input
// are read and ignored (the arena's 8 bytes of slack).  The first and the last row of a unit that the unit does not fill may belong to
// a neighbouring unit that another wave writes at the same time: those bytes are loaded and stored ONE BY ONE (one lane each), never
// by read-modify-write of the row.  Plain loads and stores: the data is touched once, and non-temporal stores were measured slower on
// this part for the parse waves' rows (wave_common.hpp: gst_row).  No LDS.
#pragma once
#include "crc32_range_kernel.hpp"

#define STORED_SEG 65536u

// what a lane knows of its position of the list: plain loads, no cross-lane operation
struct StoredLane { u32 ui, n, in_len, out_len; u64 in_off, out_off; bool is_st, part; };   // is_st: a unit of the kind; part: ... inside both arenas; n: bytes to copy
__device__ __forceinline__ StoredLane stored_lane(const mspack_hip_unit *units, const u32 *order, const u32 n_units, const u32 b, const u64 in_bytes,
                                                  const u64 out_bytes, const u32 lane)
{
  StoredLane r; r.ui = 0u; r.n = 0u; r.in_len = 0u; r.out_len = 0u; r.in_off = 0u; r.out_off = 0u; r.is_st = false; r.part = false;
  const u64 j = (u64) b * 64u + lane;
  if (j >= n_units) return r;
  r.ui = order ? gld(order + j) : (u32) j;
  const mspack_hip_unit *u = units + r.ui;
  if (gld(&u->kind) != MSPACK_HIP_KIND_STORED) return r;
  r.is_st = true;
  r.in_off = gld(&u->in_off); r.in_len = gld(&u->in_len); r.out_off = gld(&u->out_off); r.out_len = gld(&u->out_len);
  r.part = r.in_off <= in_bytes && (u64) r.in_len <= in_bytes - r.in_off && r.out_off <= out_bytes && (u64) r.out_len <= out_bytes - r.out_off;
  r.n = r.part ? (r.in_len < r.out_len ? r.in_len : r.out_len) : 0u;
  return r;
}
__device__ __forceinline__ u32 stored_head(const u8 *out_arena, const u64 off) { return (u32)((size_t)(out_arena + off) & 15u); }
__device__ __forceinline__ u32 stored_nseg(const u8 *out_arena, const StoredLane &r)
{
  if (r.n == 0u) return 0u;
  return (u32)(((u64) r.n + stored_head(out_arena, r.out_off) + STORED_SEG - 1u) / STORED_SEG);
}
// a block as the wave sees it: per lane the unit, its first ticket inside the block and its tickets; uniform: the stored units' lanes,
// the block's tickets
struct StoredBlock { StoredLane r; u32 nseg, lpfx; u64 parts; u32 total; };
__device__ __forceinline__ StoredBlock stored_block(const StoredLane &r, const u8 *out_arena)
{
  StoredBlock k; k.r = r;
  k.nseg = stored_nseg(out_arena, r);
  const u32 incl = wave_incl_scan(k.nseg);
  k.lpfx = incl - k.nseg;
  k.total = rdl(incl, 63u);
  k.parts = ballot(r.part);
  return k;
}
__device__ __forceinline__ u32 stored_first_unit(const StoredBlock &k) { return rdl(k.r.ui, (u32) __ffsll((long long) k.parts) - 1u); }

// ---- launch 1: ONE wave.  P[b] into the first stored unit of every block that has one; T and the counter's 0 into the control unit ----
__device__ __forceinline__ void stored_scan_wave(const mspack_hip_unit *units, const u32 *order, const u32 n, const u64 in_bytes, const u8 *out_arena,
                                                 const u64 out_bytes, mspack_hip_result *results)
{
  const u32 lane = threadIdx.x;
  const u32 B = (u32)(((u64) n + 63u) / 64u);
  u64 P = 0;
  bool have_ctl = false;
  u32 ctl = 0;
  for (u32 b0 = 0; b0 < B; b0 += 4u) {
    StoredLane raw[4];
#pragma unroll
    for (u32 q = 0; q < 4u; q++) raw[q] = stored_lane(units, order, n, b0 + q, in_bytes, out_bytes, lane);      // (beyond B: no position is < n)
#pragma unroll
    for (u32 q = 0; q < 4u; q++) {
      const StoredBlock k = stored_block(raw[q], out_arena);
      if (k.parts == 0ull) continue;
      const u32 fu = stored_first_unit(k);
      if (!have_ctl) { have_ctl = true; ctl = fu; }              // (P == 0 here: its words are the control's)
      else if (lane == 0) { gst(&results[fu].good_len, (u32) P); gst(&results[fu].in_next, (u32)(P >> 32)); }
      P += k.total;
    }
  }
  if (have_ctl && lane == 0) { gst(&results[ctl].good_len, (u32) P); gst(&results[ctl].in_next, (u32)(P >> 32)); gst(&results[ctl].in_used, 0u); }
}

// ---- launch 2: the pass ----
// an aligned 16-byte source row of which only [lo, hi) is the unit's: whole where it lies inside, else by 8-byte halves that hold a
// byte of the unit (addresses as integers: a row may begin below the unit)
__device__ __forceinline__ uint4 stored_src_row(const u64 p, const u64 lo, const u64 hi)
{
  if (p >= lo && p + 16u <= hi) return gld((const uint4 *)(size_t) p);
  uint2 a = make_uint2(0u, 0u), b = make_uint2(0u, 0u);
  if (p + 8u > lo && p < hi) a = gld((const uint2 *)(size_t) p);
  if (p + 16u > lo && p + 8u < hi) b = gld((const uint2 *)(size_t)(p + 8u));
  return make_uint4(a.x, a.y, b.x, b.y);
}
// bytes sh .. sh + 15 of the 32 bytes lo || hi (sh = 1 .. 15, wave-uniform)
__device__ __forceinline__ uint4 stored_realign(const uint4 lo, const uint4 hi, const u32 sh)
{
  const u32 bs = sh & 3u;
  u32 q0, q1, q2, q3, q4;
  switch (sh >> 2) {
  case 0:  q0 = lo.x; q1 = lo.y; q2 = lo.z; q3 = lo.w; q4 = hi.x; break;
  case 1:  q0 = lo.y; q1 = lo.z; q2 = lo.w; q3 = hi.x; q4 = hi.y; break;
  case 2:  q0 = lo.z; q1 = lo.w; q2 = hi.x; q3 = hi.y; q4 = hi.z; break;
  default: q0 = lo.w; q1 = hi.x; q2 = hi.y; q3 = hi.z; q4 = hi.w; break;
  }
  return make_uint4(__builtin_amdgcn_alignbyte(q1, q0, bs), __builtin_amdgcn_alignbyte(q2, q1, bs), __builtin_amdgcn_alignbyte(q3, q2, bs),
                    __builtin_amdgcn_alignbyte(q4, q3, bs));
}
// the sixteen source bytes at address a (all of them the unit's): src = [lo, hi)
__device__ __forceinline__ uint4 stored_load16(const u64 a, const u32 sh, const u64 lo, const u64 hi)
{
  if (sh == 0u) return gld((const uint4 *)(size_t) a);
  const u64 p = a - sh;
  return stored_realign(stored_src_row(p, lo, hi), stored_src_row(p + 16u, lo, hi), sh);
}
// the bytes of the row at v0 (a multiple of 16) of the unit's row stream that are the unit's, one lane each
__device__ __forceinline__ void stored_edge_row(u8 *row0, const u64 src_v, const u64 v0, const u32 head, const u64 nv, const u32 lane)
{
  const u64 v = v0 + lane;
  if (lane < 16u && v >= head && v < nv) gst(row0 + v, gld((const u8 *)(size_t)(src_v + v)));
}
// segment s of the unit (in_off, out_off, n bytes)
__device__ __forceinline__ void stored_copy_seg(const u8 *in_arena, u8 *out_arena, const u64 in_off, const u64 out_off, const u32 n, const u32 s, const u32 lane)
{
  u8 *const d = out_arena + out_off;
  const u32 head = (u32)((size_t) d & 15u);
  u8 *const row0 = d - head;
  const u64 src = (u64)(size_t)(in_arena + in_off), src_end = src + n;
  const u64 src_v = src - head;                                // the source address of position v of the row stream is src_v + v
  const u32 sh = (u32)(src_v & 15u);
  const u64 nv = (u64) n + head;
  const u64 vlo = (u64) s * STORED_SEG, vhi = vlo + STORED_SEG < nv ? vlo + STORED_SEG : nv;
  // whole rows of the segment: [flo, fhi)
  const u64 flo = (vlo == 0u && head != 0u) ? 16u : vlo;
  const u64 fhi = vhi < (nv & ~15ull) ? vhi : (nv & ~15ull);
  if (fhi > flo) {
    const u32 rows = (u32)((fhi - flo) >> 4);
    for (u32 r0 = 0; r0 < rows; r0 += 256u) {                  // four rows per lane and step, 64 lanes: at most 16 steps
      uint4 w[4];
#pragma unroll
      for (u32 q = 0; q < 4u; q++) {
        const u32 r = r0 + q * 64u + lane;
        if (r < rows) w[q] = stored_load16(src_v + flo + ((u64) r << 4), sh, src, src_end);
      }
#pragma unroll
      for (u32 q = 0; q < 4u; q++) {
        const u32 r = r0 + q * 64u + lane;
        if (r < rows) gst((uint4 *)(row0 + flo + ((u64) r << 4)), w[q]);
      }
    }
  }
  // the unit's first row and its last one where the unit does not fill them: byte by byte (a neighbour may own the rest)
  if (vlo == 0u && head != 0u) stored_edge_row(row0, src_v, 0u, head, nv, lane);
  const u64 vt = nv & ~15ull;                                  // the row behind the last whole one
  if ((nv & 15u) != 0u && vt >= vlo && vt < vhi && !(vt == 0u && head != 0u)) stored_edge_row(row0, src_v, vt, head, nv, lane);
}

__device__ __forceinline__ void stored_pass_wave(const mspack_hip_unit *units, const u32 *order, const u32 n, const u8 *in_arena, const u64 in_bytes,
                                                 u8 *out_arena, const u64 out_bytes, mspack_hip_result *results)
{
  const u32 lane = threadIdx.x;
  const u32 B = (u32)(((u64) n + 63u) / 64u);
  // the control unit: the first stored unit of the list
  u32 b_ctl = 0, ctl = 0;
  StoredBlock k;
  for (;; b_ctl++) {
    if (b_ctl >= B) return;                                     // no stored unit at all
    k = stored_block(stored_lane(units, order, n, b_ctl, in_bytes, out_bytes, lane), out_arena);
    if (k.parts) { ctl = stored_first_unit(k); break; }
  }
  const u64 T = crc32r_read64(&results[ctl]);
  if (T == 0ull) return;
  const u64 K = crc32r_chunk(T, gridDim.x);
  u32 *const counter = &results[ctl].in_used;
  for (;;) {
    u32 c = 0;
    if (lane == 0) c = crc32r_fetch_add(counter, 1u);
    c = rfl(c);
    const u64 t0 = (u64) c * K;
    if (t0 >= T) return;                                        // the counter is past the end
    const u64 t1 = t0 + K < T ? t0 + K : T;
    // the block that holds ticket t0: P[b] <= t0 < P[b] + total[b]
    u32 lo = b_ctl, hi = B - 1u, b = b_ctl;
    u64 P = 0;
    for (;;) {
      const u32 mid = lo + (hi - lo) / 2u;
      bool any = false;
      for (b = mid;; b--) {                                     // the nearest block at or below mid that has a stored unit
        k = stored_block(stored_lane(units, order, n, b, in_bytes, out_bytes, lane), out_arena);
        if (k.parts) { any = true; break; }
        if (b == lo) break;
      }
      if (!any) { if (mid >= hi) return; lo = mid + 1u; continue; }
      const u32 fu = stored_first_unit(k);
      P = fu == ctl ? 0ull : crc32r_read64(&results[fu]);
      if (t0 < P) { if (b == lo) return; hi = b - 1u; }
      else if (t0 - P < k.total) break;
      else { if (mid >= hi) return; lo = mid + 1u; }
    }
    // walk: ticket t = P + o of block b
    u32 o = (u32)(t0 - P);
    for (u64 t = t0; t < t1; t++) {
      while (o >= k.total) {                                    // on to the next block that has tickets
        o = 0;
        if (++b >= B) break;
        k = stored_block(stored_lane(units, order, n, b, in_bytes, out_bytes, lane), out_arena);
      }
      if (b >= B) break;
      const u64 own = ballot(o >= k.lpfx && o - k.lpfx < k.nseg);
      if (own == 0ull) break;
      const u32 l = (u32) __ffsll((long long) own) - 1u;
      const u32 len = rdl(k.r.n, l), s = o - rdl(k.lpfx, l);
      const u64 ioff = (u64) rdl((u32) k.r.in_off, l) | ((u64) rdl((u32)(k.r.in_off >> 32), l) << 32);
      const u64 ooff = (u64) rdl((u32) k.r.out_off, l) | ((u64) rdl((u32)(k.r.out_off >> 32), l) << 32);
      stored_copy_seg(in_arena, out_arena, ioff, ooff, len, s, lane);
      o++;
    }
  }
}

// ---- launch 3: every stored unit's result (one per lane) -- also the words the run borrowed ----
__device__ __forceinline__ void stored_result_lane(const mspack_hip_unit *units, const u32 *order, const u32 n, const u64 in_bytes, const u64 out_bytes,
                                                   mspack_hip_result *results)
{
  const StoredLane r = stored_lane(units, order, n, blockIdx.x, in_bytes, out_bytes, threadIdx.x);
  if (!r.is_st) return;
  mspack_hip_result o;
  o.flags = 0u; o.in_next = 0u;
  if (!r.part) { o.err = ERR_ARGS; o.out_len = 0u; o.in_used = 0u; o.good_len = 0u; }
  else {
    // (in_len < out_len: the feeder ran dry -- every byte it had was copied)
    o.err = r.in_len >= r.out_len ? ERR_OK : ERR_READ;
    o.out_len = r.n; o.in_used = r.n; o.good_len = r.n;
  }
  gst(&results[r.ui], o);
}
