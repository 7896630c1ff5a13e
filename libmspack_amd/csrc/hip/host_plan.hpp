// host_plan.hpp -- the host path's chunk planner: from the caller's unit table to a BatchPlan (units in arena order, frame-slot
// numbers, chunks with their spans, per-kind launch lists and CRC lists, the digest units' list, the units rebased to the spans).  Pure arithmetic: no HIP
// call, no global, no environment variable, no lock -- only <mspack_hip.h> and standard headers, so a test includes this file alone
// (tests/hostcheck/plan_check.cpp).  The knobs come in as a PlanKnobs (host_pipeline.hpp fills one from the environment).
#pragma once
#include <mspack_hip.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#define MSPK_MAX_CHUNKS 8
struct Chunk {
  size_t a, b;                          // local unit range [a, b)
  uint64_t in_lo, in_hi, out_lo, out_hi;
  size_t order_off[MSPACK_HIP_KIND_STORED + 1], order_n[MSPACK_HIP_KIND_STORED + 1];      // per kind (1 .. XORSUM, STORED; [MSPACK_HIP_KIND_MD5] unused: digest units have lists of their own): slice of the order array
  size_t fm_lo, fm_n;
  size_t crc_off, crc_n; uint64_t crc_max;      // the chunk's units that carry MSPACK_HIP_UF_CRC32: slice of the order array, the longest
  bool has_ftab;                        // some LZX unit of the chunk carries a frame table
  bool has_lzss_ring;                   // some LZSS unit of the chunk carries MSPACK_HIP_UF_LZSS_RING: its kernel is launched too
};

// bytes below out_off that belong to the unit, and the room it may write past out_len
static inline bool unit_lzss_ring(const mspack_hip_unit &u) { return u.kind == MSPACK_HIP_KIND_LZSS && (u.flags & MSPACK_HIP_UF_LZSS_RING); }
static inline uint64_t unit_below(const mspack_hip_unit &u) {
  if (unit_lzss_ring(u)) return 0u;                    // (its window is in LDS)
  return (u.kind == MSPACK_HIP_KIND_LZSS || u.kind == MSPACK_HIP_KIND_KWAJ_LZH) ? 4096u
       : (u.kind == MSPACK_HIP_KIND_LZX_DELTA ? u.ref_len : 0u);
}
static inline uint64_t unit_above(const mspack_hip_unit &u) {
  if (u.kind == MSPACK_HIP_KIND_LZX && (u.flags & MSPACK_HIP_UF_LZX_LOG))                   // the reset log, where MSZIP's would be
    return ((((uint64_t) u.out_len + 32768u + 15u) & ~15ull) - u.out_len) + 4u + 4u * (uint64_t) u.ref_len;
  if (u.kind == MSPACK_HIP_KIND_QUANTUM && (u.flags & MSPACK_HIP_UF_QTM_MARKS) && u.ref_len)   // the log of its marks
    return ((((uint64_t) u.out_len + 15u) & ~15ull) - u.out_len) + 4u * (uint64_t) u.ref_len;
  if (u.kind != MSPACK_HIP_KIND_MSZIP) return 0u;
  uint64_t a = 32768u;
  if ((u.flags & MSPACK_HIP_UF_MSZIP_REPAIR) && (u.flags & MSPACK_HIP_UF_MSZIP_LOG))      // the repair log behind the slack
    a = ((((uint64_t) u.out_len + 32768u + 15u) & ~15ull) - u.out_len) + 4u + 8u * (uint64_t)(u.e8_base > 0 ? u.e8_base : 0);
  return a;
}
static inline bool unit_has_ftab(const mspack_hip_unit &u) {
  if (!(u.flags & MSPACK_HIP_UF_FRAME_TABLE)) return false;
  if (u.kind == MSPACK_HIP_KIND_LZX) return true;
  return u.kind == MSPACK_HIP_KIND_MSZIP && !(u.flags & (MSPACK_HIP_UF_MSZIP_REPAIR | MSPACK_HIP_UF_MSZIP_KWAJ));
}
static inline uint64_t unit_ftab_bytes(const mspack_hip_unit &u) { return (((uint64_t) u.out_len + 32767u) / 32768u) * 4u; }
// a table the unit reads out of the input arena besides its stream (in_chunk * 4: a frame / block table, a Quantum unit's marks)
static inline bool unit_side_table(const mspack_hip_unit &u, uint64_t &lo, uint64_t &hi) {
  if (unit_has_ftab(u)) { lo = (uint64_t) u.in_chunk * 4u; hi = lo + unit_ftab_bytes(u); return true; }
  if (u.kind == MSPACK_HIP_KIND_QUANTUM && (u.flags & MSPACK_HIP_UF_QTM_MARKS) && u.ref_len) {
    lo = (uint64_t) u.in_chunk * 4u; hi = lo + 4u * (uint64_t) u.ref_len; return true;
  }
  return false;
}
// digest units: the heads (MD5 and CRC-32 ranges; SHA-1, SHA-256, SHA-384 and SHA-512, whose results go on in the next units') and the
// tails of the wide ones
static inline bool unit_is_sha512(const mspack_hip_unit &u) { return u.kind == MSPACK_HIP_KIND_SHA384 || u.kind == MSPACK_HIP_KIND_SHA512; }
static inline bool unit_is_wide_head(const mspack_hip_unit &u) { return u.kind == MSPACK_HIP_KIND_SHA1 || u.kind == MSPACK_HIP_KIND_SHA256 || unit_is_sha512(u); }
// the tails a head needs behind it: ceil(digest bytes / 16) - 1 (mspack_hip.h)
static inline size_t unit_wide_tails(const mspack_hip_unit &u) { return u.kind == MSPACK_HIP_KIND_SHA384 ? 2u : u.kind == MSPACK_HIP_KIND_SHA512 ? 3u : unit_is_wide_head(u) ? 1u : 0u; }
static inline bool unit_is_digest_head(const mspack_hip_unit &u) { return u.kind == MSPACK_HIP_KIND_MD5 || u.kind == MSPACK_HIP_KIND_CRC32 || unit_is_wide_head(u); }
static inline bool unit_is_digest(const mspack_hip_unit &u) { return unit_is_digest_head(u) || u.kind == MSPACK_HIP_KIND_DIGEST_MORE; }
static inline size_t unit_frames(const mspack_hip_unit &u) {
  if (u.kind == MSPACK_HIP_KIND_LZX || u.kind == MSPACK_HIP_KIND_LZX_DELTA) return (size_t) u.out_len / 32768u + 1u;
  if (u.kind == MSPACK_HIP_KIND_MSZIP && unit_has_ftab(u)) return ((size_t) u.out_len + 32767u) / 32768u;   // one per CFDATA block
  return 0u;
}

struct PlanKnobs {
  size_t max_chunks, chunk_bytes, chunk_units;      // at most so many chunks, each >= chunk_bytes of input and >= chunk_units units
  int shape;                                        // the chunks' shares (plan_batch); -1 = by destination
  std::vector<uint64_t> weights;                    // the first shares spelled out (sweeps)
};
// what plan_batch computes.  local[i] is unit idx[i] of the caller's table, offsets relative to in_lo / out_lo; the chunks are
// ranges of local[]; order holds every chunk's per-kind lists and its CRC list (indices into local[]).
// Digest units (MSPACK_HIP_KIND_MD5, _SHA1, _SHA256, _SHA384, _SHA512 and the wide ones' _DIGEST_MORE tails) read no input and own no
// output: they stand BEHIND the chunks in local[] -- indices [n - n_dig, n), in the caller's order, so a head keeps its tails at
// i + 1 ..; no chunk holds them, no per-kind list, no weight in the cutting -- and order holds four consecutive lists of HEADS, one per
// kernel (MD5 at md5_off, SHA-1 at sha1_off, SHA-256 at sha256_off, SHA-384 and SHA-512 together at sha512_off: they share a kernel),
// each longest range first (one lane each: lanes of similar length next to each other) for that kernel's one pass behind the last
// chunk; behind them the list of the CRC-32 range units (crc32r_off), in the caller's order: their pass takes segments, not units,
// so the order carries no weight
struct BatchPlan {
  std::vector<uint32_t> idx;
  std::vector<mspack_hip_unit> local;
  std::vector<uint32_t> order;
  std::vector<Chunk> chunks;
  uint64_t in_lo, in_hi, out_lo, out_hi, in_sum;
  size_t n_frames, n_rec_slots, n_crc;              // n_crc: units that want a digest (MSPACK_HIP_UF_CRC32)
  size_t n_md5 = 0, md5_off = 0;                    // the MD5 units: how many, their list's place in order
  size_t n_sha1 = 0, sha1_off = 0, n_sha256 = 0, sha256_off = 0;      // the SHA-1 / SHA-256 heads likewise
  size_t n_sha512 = 0, sha512_off = 0;              // the SHA-384 and SHA-512 heads, one list
  size_t n_crc32r = 0, crc32r_off = 0;              // the CRC-32 range units (MSPACK_HIP_KIND_CRC32) likewise
  size_t n_dig = 0;                                 // every digest unit, tails included: local[n - n_dig .. n)
  bool monotone, has_qtm;
};

// plan_batch's first step: the units in arena order, validated, their frame slots numbered, the batch's spans
static int plan_units(mspack_hip_unit *units, const uint32_t *sel, size_t n_sel, size_t in_bytes, size_t out_bytes,
                      bool dev_out, bool per_unit_back, BatchPlan &p, char *errbuf, size_t errcap)
{
  std::vector<uint32_t> &idx = p.idx;
  std::vector<mspack_hip_unit> &local = p.local;
  idx.resize(n_sel);
  for (size_t i = 0; i < n_sel; i++) idx[i] = sel ? sel[i] : (uint32_t) i;
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return units[x].in_off < units[y].in_off; });
  // (digest units behind everything else, in the caller's order: their in_off means nothing)
  {
    const auto mid = std::stable_partition(idx.begin(), idx.end(), [&](uint32_t x) { return !unit_is_digest(units[x]); });
    std::sort(mid, idx.end());
    p.n_dig = (size_t)(idx.end() - mid);
    p.n_md5 = p.n_sha1 = p.n_sha256 = p.n_sha512 = p.n_crc32r = 0;
  }
  local.resize(n_sel);
  bool monotone = !per_unit_back;
  uint64_t in_lo = ~0ull, in_hi = 0, out_lo = ~0ull, out_hi = 0, prev_hi = 0, in_sum = 0;
  size_t n_frames = 0, n_rec_slots = 0, n_crc = 0;
  for (size_t i = 0; i < n_sel; i++) {
    mspack_hip_unit &u = local[i];
    u = units[idx[i]];
    if (u.kind != MSPACK_HIP_KIND_LZX_DELTA && !(u.kind == MSPACK_HIP_KIND_LZX && (u.flags & MSPACK_HIP_UF_LZX_LOG)) &&
        !(u.kind == MSPACK_HIP_KIND_QUANTUM && (u.flags & MSPACK_HIP_UF_QTM_MARKS))) u.ref_len = 0;
    if (u.kind > MSPACK_HIP_KIND_MD5 && u.kind != MSPACK_HIP_KIND_STORED && !unit_is_digest(u)) { snprintf(errbuf, errcap, "unit %u: unknown kind %u", idx[i], u.kind); return -1; }
    if (u.kind == MSPACK_HIP_KIND_XORSUM) {                // reads its input, owns no output
      if (u.flags & MSPACK_HIP_UF_CRC32) { snprintf(errbuf, errcap, "unit %u: a checksum unit decodes nothing to take a CRC-32 of", idx[i]); return -1; }
      if (u.out_len) { snprintf(errbuf, errcap, "unit %u: a checksum unit has no output", idx[i]); return -1; }
      if (u.in_off + u.in_len > in_bytes) { snprintf(errbuf, errcap, "unit outside arena"); return -1; }
      in_lo = std::min<uint64_t>(in_lo, u.in_off); in_hi = std::max<uint64_t>(in_hi, u.in_off + u.in_len);
      continue;
    }
    if (u.kind == MSPACK_HIP_KIND_DIGEST_MORE) {           // a wide digest's tail: names nothing, stands behind its head, among the tails it needs
      // (the digest units are in table order here: neighbours in the table are neighbours in this list)
      size_t k = 1;                                        // the first unit in front of it that is no tail, as far back as a head reaches
      while (k < 3 && i >= n_sel - p.n_dig + k + 1 && idx[i - k] + 1u == idx[i - k + 1] && local[i - k].kind == MSPACK_HIP_KIND_DIGEST_MORE) k++;
      if (i < n_sel - p.n_dig + k || idx[i - k] + 1u != idx[i - k + 1] || unit_wide_tails(local[i - k]) < k) {
        snprintf(errbuf, errcap, "unit %u: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it", idx[i]); return -1;
      }
      if (u.in_len || u.out_len) { snprintf(errbuf, errcap, "unit %u: an MSPACK_HIP_KIND_DIGEST_MORE unit names no bytes (in_len and out_len must be 0)", idx[i]); return -1; }
      u.in_off = 0; u.out_off = 0; u.flags = 0;
      continue;
    }
    if (unit_is_digest_head(u)) {                          // reads a range of the output arena, owns nothing
      if (u.flags & MSPACK_HIP_UF_CRC32) { snprintf(errbuf, errcap, "unit %u: a digest unit decodes nothing to take a CRC-32 of", idx[i]); return -1; }
      if (u.in_len) { snprintf(errbuf, errcap, "unit %u: a digest unit reads no input (in_len must be 0)", idx[i]); return -1; }
      if (u.out_off > out_bytes || u.out_len > out_bytes - u.out_off) { snprintf(errbuf, errcap, "unit %u: a digest unit's range leaves the output arena", idx[i]); return -1; }
      if (unit_is_wide_head(u)) {                          // its result goes on in the next unit's (SHA-384: next two units', SHA-512: three)
        if (!sel && (size_t) idx[i] + 1u >= n_sel) { snprintf(errbuf, errcap, "unit %u: a wide digest unit is the table's last unit (its MSPACK_HIP_KIND_DIGEST_MORE unit is missing)", idx[i]); return -1; }
        if (i + 1 >= n_sel || idx[i + 1] != idx[i] + 1u || units[idx[i + 1]].kind != MSPACK_HIP_KIND_DIGEST_MORE) {
          snprintf(errbuf, errcap, "unit %u: a wide digest unit must be followed by an MSPACK_HIP_KIND_DIGEST_MORE unit", idx[i]); return -1;
        }
        for (size_t k = 2; k <= unit_wide_tails(u); k++)
          if (i + k >= n_sel || idx[i + k] != idx[i] + k || units[idx[i + k]].kind != MSPACK_HIP_KIND_DIGEST_MORE) {
            snprintf(errbuf, errcap, "unit %u: a %s unit must be followed by %u MSPACK_HIP_KIND_DIGEST_MORE units", idx[i],
                     u.kind == MSPACK_HIP_KIND_SHA384 ? "SHA-384" : "SHA-512", (unsigned) unit_wide_tails(u));
            return -1;
          }
      }
      (u.kind == MSPACK_HIP_KIND_MD5 ? p.n_md5 : u.kind == MSPACK_HIP_KIND_SHA1 ? p.n_sha1 : u.kind == MSPACK_HIP_KIND_SHA256 ? p.n_sha256 :
       unit_is_sha512(u) ? p.n_sha512 : p.n_crc32r)++;
      u.in_off = 0; u.flags = 0;
      if (u.out_len) { out_lo = std::min<uint64_t>(out_lo, u.out_off); out_hi = std::max<uint64_t>(out_hi, u.out_off + u.out_len); }
      continue;
    }
    if (u.kind == MSPACK_HIP_KIND_STORED) {                // copies its input: owns exactly [out_off, out_off + out_len), reads exactly its in_len bytes
      if (u.in_off > in_bytes || u.in_len > in_bytes - u.in_off) { snprintf(errbuf, errcap, "unit %u: a stored unit's input leaves the input arena", idx[i]); return -1; }
      if (u.out_off > out_bytes || u.out_len > out_bytes - u.out_off) { snprintf(errbuf, errcap, "unit %u: a stored unit's output leaves the output arena", idx[i]); return -1; }
    }
    // kind 0 = "no codec": the unit is carried along, no kernel takes it, its result says MSPACK_ERR_ARGS
    const uint64_t below = unit_below(u);
    if (below > u.out_off) { snprintf(errbuf, errcap, "unit's lower region outside arena"); return -1; }
    const uint64_t lo = u.out_off - below, hi = u.out_off + u.out_len + unit_above(u);
    if (u.in_off + u.in_len > in_bytes || hi > out_bytes) { snprintf(errbuf, errcap, "unit outside arena"); return -1; }
    if (i && lo < prev_hi) monotone = false;
    prev_hi = hi;
    in_lo = std::min<uint64_t>(in_lo, u.in_off); in_hi = std::max<uint64_t>(in_hi, u.in_off + u.in_len);
    {
      uint64_t tl, th;
      if (unit_side_table(u, tl, th)) {
        if (th > in_bytes) { snprintf(errbuf, errcap, "unit's table outside arena"); return -1; }
        if (u.kind == MSPACK_HIP_KIND_QUANTUM && (u.out_off & 3u)) { snprintf(errbuf, errcap, "unit %u: a Quantum unit with marks needs out_off %% 4 == 0", idx[i]); return -1; }
        in_lo = std::min(in_lo, tl); in_hi = std::max(in_hi, th);
      }
    }
    out_lo = std::min(out_lo, lo); out_hi = std::max(out_hi, hi);
    in_sum += u.in_len;
    if ((u.flags & MSPACK_HIP_UF_CRC32) && u.kind != 0) n_crc++;
  }
  // frame slots: the units that carry a usable frame / block table first -- only their slots hold records and tokens
  for (int pass = 0; pass < 2; pass++) {
    for (size_t i = 0; i < n_sel; i++) {
      mspack_hip_unit &u = local[i];
      if ((pass == 0) != unit_has_ftab(u)) continue;
      u.frame_base = (uint32_t) n_frames; units[idx[i]].frame_base = (uint32_t) n_frames;
      n_frames += unit_frames(u);
    }
    if (pass == 0) n_rec_slots = n_frames;
  }
  if (in_lo > in_hi) in_lo = in_hi = 0;                // (digest units only: nothing is read)
  in_lo &= ~15ull;                                     // keep the units' alignment
  if (out_lo > out_hi) out_lo = out_hi = 0;            // (checksum units only: nothing is written)
  if (dev_out) out_lo = 0;                             // the caller's device buffer is addressed as is
  p.in_lo = in_lo; p.in_hi = in_hi; p.out_lo = out_lo; p.out_hi = out_hi; p.in_sum = in_sum;
  p.n_frames = n_frames; p.n_rec_slots = n_rec_slots; p.n_crc = n_crc; p.monotone = monotone;
  return 0;
}

// the second: which units go into which chunk
static void plan_chunks(bool to_host, const PlanKnobs &kn, BatchPlan &p)
{
  const std::vector<mspack_hip_unit> &local = p.local;
  const size_t n_sel = local.size() - p.n_dig;          // (the digest units stand behind the chunks)
  const bool monotone = p.monotone;
  const uint64_t in_sum = p.in_sum;
  // chunks: arena-contiguous runs of units; enough of them to overlap the copies with the decode, each
  // big enough to be worth a launch.  Outputs that interleave (not monotone) are copied back unit by unit.
  // (a chunk: >= chunk_bytes of input -- 8 MiB: a copy of >= 150 us -- and >= chunk_units units: 256)
  bool has_qtm = false;
  const size_t max_chunks = std::min<size_t>(kn.max_chunks, MSPK_MAX_CHUNKS);
  size_t want = monotone ? std::min<size_t>(max_chunks, std::max<size_t>(1, in_sum / kn.chunk_bytes)) : 1;
  {
    // (units that decode: checksum units ride along and are no reason to cut)
    size_t n_dec = 0;
    for (size_t i = 0; i < n_sel; i++) {
      if (local[i].kind != MSPACK_HIP_KIND_XORSUM) n_dec++;
      if (local[i].kind == MSPACK_HIP_KIND_QUANTUM) has_qtm = true;
    }
    want = std::min(want, std::max<size_t>(1, n_dec / kn.chunk_units));
  }
  p.has_qtm = has_qtm;
  std::vector<Chunk> &chunks = p.chunks;
  chunks.clear();
  {
    // shares of the input bytes.  MSPACK_HIP_CHUNK_SHAPE: 0 equal; 1 = 1 : 1 : 2 : 4 ... (to the device: the default -- the small
    // chunks get the launches going while most of the input is still on its way, and the LAST chunk, whose launches end the call,
    // is the large one that fills the chip: headline 4.64-4.84 -> 4.05-4.15 ms, every growing shape within 0.1 ms of it, falling
    // ones and more than four chunks slower; 1024 and 16 384 units: no difference -- profiles/round6_jobs.txt; round 3 had it at
    // 4.55 against 4.74 and kept the equal shares); 2 = a first chunk of half a share (to the host: the default -- the copy-back,
    // the longest leg, starts as soon as the first chunk is through; 1 there: 8.2 against 7.6 ms); 3, 4: a x1.5 ramp, falling shares
    // (sweeps)
    const int shape = kn.shape >= 0 ? kn.shape : (to_host ? 2 : 1);
    uint64_t wsum = 0, w[MSPK_MAX_CHUNKS];
    // (kn.weights, MSPACK_HIP_CHUNK_WEIGHTS="1,1,2,4": the shares spelled out -- sweeps)
    for (size_t k = 0; k < want; k++) {
      static const uint64_t ramp[MSPK_MAX_CHUNKS] = { 4, 6, 9, 13, 20, 30, 45, 67 };          // (3: every chunk half as large again)
      static const uint64_t fall[MSPK_MAX_CHUNKS] = { 8, 6, 4, 3, 2, 2, 1, 1 };               // (4: the last chunks -- whose launches end the call -- small)
      w[k] = (k < kn.weights.size()) ? kn.weights[k] : shape == 4 ? fall[k] : shape == 3 ? ramp[k] : shape == 1 ? (k >= 2 ? (uint64_t) 2 << (k - 1) : 2) : (shape == 2 && k == 0 && want >= 3 ? 1 : 2);
      wsum += w[k];
    }
    // (a unit weighs what it reads that the NEXT unit does not start inside: a CHM's intervals are all given "to the end of the
    // file" as input, chmd.c:1146-1149 -- by in_len alone config 3's four chunks held 77, 174, 227 and 546 of its 1024 intervals)
    auto weight = [&](size_t i) -> uint64_t {
      uint64_t wgt = local[i].in_len;
      for (size_t j = i + 1; j < n_sel; j++) {
        if (local[j].kind == MSPACK_HIP_KIND_XORSUM) continue;
        if (local[j].in_off > local[i].in_off && local[j].in_off - local[i].in_off < wgt) wgt = local[j].in_off - local[i].in_off;
        break;
      }
      return wgt;
    };
    uint64_t w_sum = 0;
    for (size_t i = 0; i < n_sel; i++) if (local[i].kind != MSPACK_HIP_KIND_XORSUM) w_sum += weight(i);
    size_t a = 0; uint64_t acc = 0, upto = 0;
    for (size_t i = 0; i < n_sel; i++) {
      if (local[i].kind != MSPACK_HIP_KIND_XORSUM) acc += weight(i);           // (the checksum units ride along)
      const uint64_t goal = (uint64_t)((double) w_sum * (double)(upto + w[chunks.size()]) / (double) wsum);
      if (i + 1 == n_sel || (acc >= goal && chunks.size() + 1 < want)) {
        Chunk c; c.a = a; c.b = i + 1; upto += w[chunks.size()]; chunks.push_back(c); a = i + 1;
      }
    }
    if (chunks.empty()) { Chunk c; c.a = c.b = 0; chunks.push_back(c); }      // (digest units only: one chunk that holds nothing)
  }
}

// the third, per chunk: spans, per-kind launch lists (longest compressed unit first: the slowest chain starts first)
static void plan_lists(BatchPlan &p)
{
  const std::vector<mspack_hip_unit> &local = p.local;
  std::vector<Chunk> &chunks = p.chunks;
  const size_t n_sel = local.size(), n_crc = p.n_crc;
  const uint64_t out_lo = p.out_lo;
  std::vector<uint32_t> &order = p.order;
  order.assign(n_sel + n_crc, 0u);                     // (the digest units are in no per-kind list: their own list fills the room)
  size_t op = 0;
  uint64_t ci_prev_hi = out_lo == ~0ull ? 0 : out_lo;
  for (Chunk &c : chunks) {
    c.in_lo = ~0ull; c.in_hi = 0; c.out_lo = ~0ull; c.out_hi = 0;
    c.fm_lo = ~(size_t) 0; c.fm_n = 0; c.has_ftab = false; c.has_lzss_ring = false;
    for (size_t i = c.a; i < c.b; i++) {
      const mspack_hip_unit &u = local[i];
      c.in_lo = std::min<uint64_t>(c.in_lo, u.in_off); c.in_hi = std::max<uint64_t>(c.in_hi, u.in_off + u.in_len);
      { uint64_t tl, th; if (unit_side_table(u, tl, th)) { c.in_lo = std::min(c.in_lo, tl); c.in_hi = std::max(c.in_hi, th); } }
      if (unit_has_ftab(u)) {
        c.has_ftab = true;
        c.fm_lo = std::min<size_t>(c.fm_lo, u.frame_base);          // (the chunk's table units' slots are contiguous)
        c.fm_n += unit_frames(u);
      }
      if (u.kind == MSPACK_HIP_KIND_XORSUM) continue;
      if (unit_lzss_ring(u)) c.has_lzss_ring = true;
      c.out_lo = std::min<uint64_t>(c.out_lo, u.out_off - unit_below(u));
      c.out_hi = std::max<uint64_t>(c.out_hi, u.out_off + u.out_len + unit_above(u));
    }
    if (c.out_lo > c.out_hi) c.out_lo = c.out_hi = (ci_prev_hi);         // (a chunk of checksum units only: an empty span)
    if (c.in_lo > c.in_hi) c.in_lo = c.in_hi = p.in_lo;                  // (the chunk that holds nothing)
    ci_prev_hi = c.out_hi;
    if (c.fm_lo == ~(size_t) 0) c.fm_lo = 0;
    c.in_lo &= ~15ull;
    for (unsigned k = 1; k <= MSPACK_HIP_KIND_STORED; k++) {      // (the stored units' list behind the codecs' and the checksum units')
      c.order_off[k] = op;
      for (size_t i = c.a; i < c.b; i++) if (local[i].kind == k) order[op++] = (uint32_t) i;
      c.order_n[k] = op - c.order_off[k];
      std::stable_sort(order.begin() + c.order_off[k], order.begin() + op, [&](uint32_t x, uint32_t y) {
        return local[x].in_len + (local[x].out_len >> 2) > local[y].in_len + (local[y].out_len >> 2); });
    }
    // the digest pass's list (launched behind the codecs): the chunk's flagged units, in arena order
    c.crc_off = op; c.crc_max = 0;
    if (n_crc)
      for (size_t i = c.a; i < c.b; i++)
        if ((local[i].flags & MSPACK_HIP_UF_CRC32) && local[i].kind != 0 && local[i].kind != MSPACK_HIP_KIND_XORSUM) {
          order[op++] = (uint32_t) i;
          c.crc_max = std::max<uint64_t>(c.crc_max, local[i].out_len);
        }
    c.crc_n = op - c.crc_off;
  }
  // the digest units' lists, one per algorithm, heads only: longest range first
  const unsigned dig_kind[3] = { MSPACK_HIP_KIND_MD5, MSPACK_HIP_KIND_SHA1, MSPACK_HIP_KIND_SHA256 };
  size_t *const dig_off[3] = { &p.md5_off, &p.sha1_off, &p.sha256_off };
  for (int a = 0; a < 3; a++) {
    *dig_off[a] = op;
    for (size_t i = n_sel - p.n_dig; i < n_sel; i++) if (local[i].kind == dig_kind[a]) order[op++] = (uint32_t) i;
    std::stable_sort(order.begin() + *dig_off[a], order.begin() + op, [&](uint32_t x, uint32_t y) { return local[x].out_len > local[y].out_len; });
  }
  // ... SHA-384 and SHA-512 heads in one list (one kernel takes both), longest first over both
  p.sha512_off = op;
  if (p.n_sha512) {
    for (size_t i = n_sel - p.n_dig; i < n_sel; i++) if (unit_is_sha512(local[i])) order[op++] = (uint32_t) i;
    std::stable_sort(order.begin() + p.sha512_off, order.begin() + op, [&](uint32_t x, uint32_t y) { return local[x].out_len > local[y].out_len; });
  }
  // ... and the CRC-32 range units' list behind them
  p.crc32r_off = op;
  if (p.n_crc32r)
    for (size_t i = n_sel - p.n_dig; i < n_sel; i++) if (local[i].kind == MSPACK_HIP_KIND_CRC32) order[op++] = (uint32_t) i;
}

// `sel` lists the unit indices of the batch (NULL = all n_sel units).  to_host: the outputs go back to the caller's host buffer;
// dev_out: they stay in the caller's DEVICE buffer (out_off relative to it); per_unit_back: they are copied back unit by unit (one
// chunk).  Writes frame_base into units[] too.  0, or -1 with the reason in errbuf.
static int plan_batch(mspack_hip_unit *units, const uint32_t *sel, size_t n_sel, size_t in_bytes, size_t out_bytes, bool to_host,
                      bool dev_out, bool per_unit_back, const PlanKnobs &kn, BatchPlan &p, char *errbuf, size_t errcap)
{
  if (plan_units(units, sel, n_sel, in_bytes, out_bytes, dev_out, per_unit_back, p, errbuf, errcap)) return -1;
  plan_chunks(to_host, kn, p);
  plan_lists(p);
  std::vector<mspack_hip_unit> &local = p.local;
  const uint64_t in_lo = p.in_lo, out_lo = p.out_lo;
  for (size_t i = 0; i < n_sel; i++) {
    { uint64_t tl, th; if (unit_side_table(local[i], tl, th)) local[i].in_chunk -= (uint32_t)(in_lo >> 2); }      // in_lo is a multiple of 16
    if (unit_is_digest(local[i])) { if (local[i].out_len) local[i].out_off -= out_lo; else local[i].out_off = 0; continue; }
    local[i].in_off -= in_lo;
    if (local[i].kind != MSPACK_HIP_KIND_XORSUM) local[i].out_off -= out_lo;
  }
  return 0;
}

// mspack_hip_decode_batch_multi's cut: which units go to which of n_shards shards (indices into units[], arena order within a shard).
// false: the batch cannot be cut (digest units over outputs that interleave) -- one device takes it whole.
static bool plan_shards(const mspack_hip_unit *units, size_t n_units, int n_shards, std::vector<std::vector<uint32_t>> &shard, bool &ascending)
{
  // static sharding, no inter-device traffic: units in arena order are cut into n_shards CONTIGUOUS ranges of
  // about equal compressed size, so that every device stages one contiguous span of each arena
  std::vector<uint32_t> idx(n_units);
  for (size_t i = 0; i < n_units; i++) idx[i] = (uint32_t) i;
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return units[a].in_off < units[b].in_off; });
  uint64_t total = 0;
  for (size_t i = 0; i < n_units; i++) if (!unit_is_digest(units[i])) total += (uint64_t) units[i].in_len + (units[i].out_len >> 2) + 256u;
  // every shard copies its whole output span back with one copy -- valid only if the spans do not interleave, i.e. if
  // the outputs ascend with the inputs over the WHOLE batch; otherwise the shards copy back unit by unit
  ascending = true;
  {
    uint64_t prev_hi = 0;
    for (size_t i = 0; i < n_units && ascending; i++) {
      const mspack_hip_unit &u = units[idx[i]];
      if (u.kind == MSPACK_HIP_KIND_XORSUM || unit_is_digest(u)) continue;                   // (no output)
      const uint64_t lo = u.out_off - std::min<uint64_t>(u.out_off, unit_below(u)), hi = u.out_off + u.out_len + unit_above(u);
      if (lo < prev_hi) ascending = false;
      prev_hi = std::max(prev_hi, hi);
    }
  }
  // Digest units: a shard's device holds only what the shard's units stored, so no cut may fall inside a digest range and a
  // digest unit goes to the shard that holds its range.  With outputs that ascend a range covers the regions of CONSECUTIVE units
  // (positions [first, last] of idx): the cuts behind first .. last - 1 are barred; the cuts that stay are taken as before -- at
  // worst there are fewer shards.  (Outputs that interleave: no cut says where a range lies -- one shard.)
  std::vector<uint32_t> md5s;
  for (size_t i = 0; i < n_units; i++) if (unit_is_digest(units[i])) md5s.push_back((uint32_t) i);
  if (!md5s.empty() && !ascending) return false;
  std::vector<uint8_t> barred(n_units, 0);
  std::vector<size_t> md5_first(md5s.size(), (size_t) -1);
  if (!md5s.empty()) {
    struct Region { uint64_t lo, hi; size_t pos; };
    std::vector<Region> dec;                                // the units that own output, ascending and disjoint
    for (size_t i = 0; i < n_units; i++) {
      const mspack_hip_unit &u = units[idx[i]];
      if (u.kind == MSPACK_HIP_KIND_XORSUM || unit_is_digest(u)) continue;
      dec.push_back(Region{ u.out_off - std::min<uint64_t>(u.out_off, unit_below(u)), u.out_off + u.out_len + unit_above(u), i });
    }
    for (size_t m = 0; m < md5s.size(); m++) {
      const mspack_hip_unit &d = units[md5s[m]];
      const uint64_t dlo = d.out_off, dhi = d.out_off + d.out_len;
      // the first region that ends behind dlo, the first that begins at or behind dhi: what lies between them meets the range
      const size_t a = (size_t)(std::upper_bound(dec.begin(), dec.end(), dlo, [](uint64_t v, const Region &r) { return v < r.hi; }) - dec.begin());
      const size_t b = (size_t)(std::lower_bound(dec.begin(), dec.end(), dhi, [](const Region &r, uint64_t v) { return r.lo < v; }) - dec.begin());
      if (d.out_len == 0 || a >= b) continue;
      md5_first[m] = dec[a].pos;
      for (size_t i = dec[a].pos; i < dec[b - 1].pos; i++) barred[i] = 1;
    }
  }
  shard.assign((size_t) n_shards, std::vector<uint32_t>());
  std::vector<int> shard_of(n_units, 0);                    // by position in idx
  {
    uint64_t acc = 0; int s = 0;
    for (size_t i = 0; i < n_units; i++) {
      if (unit_is_digest(units[idx[i]])) continue;
      shard[s].push_back(idx[i]);
      shard_of[i] = s;
      acc += (uint64_t) units[idx[i]].in_len + (units[idx[i]].out_len >> 2) + 256u;
      if (s + 1 < n_shards && acc * n_shards >= total * (uint64_t)(s + 1) && !barred[i]) s++;
    }
  }
  // (a wide digest's tails go where their head went: md5s is in table order, so the head is the first entry before them that is no tail)
  for (size_t m = 0, at = 0; m < md5s.size(); m++) {
    size_t k = 1;
    while (k < 3 && k < m && md5s[m - k] + 1u == md5s[m - k + 1] && units[md5s[m - k]].kind == MSPACK_HIP_KIND_DIGEST_MORE) k++;
    const bool tail = units[md5s[m]].kind == MSPACK_HIP_KIND_DIGEST_MORE && m >= k && md5s[m - k] + 1u == md5s[m - k + 1] && unit_wide_tails(units[md5s[m - k]]) >= k;
    if (!tail) at = md5_first[m] == (size_t) -1 ? 0 : (size_t) shard_of[md5_first[m]];
    shard[at].push_back(md5s[m]);
  }
  return true;
}
