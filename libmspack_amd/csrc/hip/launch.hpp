// launch.hpp -- the launch layer and the device-resident C ABI: the thread's error text, launch<> (a kernel launch whose status is
// returned), the launch-level environment knobs, launch_kind (one codec's launches over a compact unit list), launch_crc32, launch_md5, launch_sha1 /
// launch_sha256, launch_sha512, launch_crc32_ranges, launch_stored, the
// analysis builds' debug exports, version / features / device functions, mspack_hip_decode_batch_device and _time_batch_device.
#pragma once
#include <mutex>
#include <tuple>
#include <utility>
// ---------------------------------------------------------------------------------------------------
// Host side of the C ABI.
// ---------------------------------------------------------------------------------------------------
#define MSPK_MAX_DEV_CACHE 64
static thread_local char g_err[256] = "";
static int fail(hipError_t e, const char *what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return -(int) e;
}
#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(e_, #call); } while (0)

static int env_int(const char *name, int dflt, int lo, int hi) {
  const char *e = getenv(name);
  int v = e ? atoi(e) : dflt;
  return v < lo ? lo : (v > hi ? hi : v);
}

// one launch per codec over a COMPACT list of that codec's units (order[0..n) = unit indices).  LZX units
// that carry a frame table get their frames parsed by one wave each first (slots [slot_lo, slot_lo + n_slots)
// of the work scratch belong to this launch).
static const bool g_no_frames = getenv("MSPACK_HIP_NO_FRAME_PARSE") != nullptr;     // experiments: serial path only
// MSPACK_HIP_FOLD: 0 = a folder's copies always through lzx_pipe_resolve, 1 (default) = through mspack_lzx_fold when the launch is few
// long units, 2 = whenever the units allow it (tests, A/B runs)
// MSPACK_HIP_STREAM_RESOLVE=0: resolve tasks never take frames up while they are parsed (A/B runs)
static const int g_stream_resolve = getenv("MSPACK_HIP_STREAM_RESOLVE") ? atoi(getenv("MSPACK_HIP_STREAM_RESOLVE")) : 1;     // (2: also in launches that run beside others -- A/B runs)
static const u32 g_fold_policy = getenv("MSPACK_HIP_FOLD") ? (u32) atoi(getenv("MSPACK_HIP_FOLD")) : 1u;
// MSPACK_HIP_TICKET_ORDER (A/B runs, tests): 0 level order, 1 mixed sections, 2 unit-major; 3 (default): by the launch's shape --
// unit-major when every ticket finds a wave at once, mixed sections from 1.5 x as many units as waves on, level order in between
static const u32 g_ticket_order = getenv("MSPACK_HIP_TICKET_ORDER") ? (u32) atoi(getenv("MSPACK_HIP_TICKET_ORDER")) : 3u;
// persistent waves of mspack_lzx_pipe: as many as the device holds at once (nothing depends on that number being right)
// (cached per device: mspack_hip_decode_batch_multi runs one host thread per device)
static unsigned lzx_pipe_waves()
{
  static std::mutex mu;
  static unsigned cache[MSPK_MAX_DEV_CACHE] = { 0 };
  int dev = 0, per_cu = 0; hipDeviceProp_t pr;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MSPK_MAX_DEV_CACHE) return 4096u;
  std::lock_guard<std::mutex> lock(mu);
  if (!cache[dev]) {
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return 4096u;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mspack_lzx_pipe, 64, 0);
    if (e != hipSuccess || per_cu < 1) per_cu = 16;
    { const char *ev = getenv("MSPACK_HIP_PIPE_WAVES_PER_CU"); if (ev && atoi(ev) > 0) per_cu = atoi(ev); }
    cache[dev] = (unsigned) pr.multiProcessorCount * (unsigned) per_cu;
  }
  return cache[dev];
}
// waves of mspack_lzx_fold: one per CU (its LDS block is most of a CU's)
static unsigned lzx_fold_waves()
{
  int dev = 0; hipDeviceProp_t pr;
  static std::mutex mu;
  static unsigned cache[MSPK_MAX_DEV_CACHE] = { 0 };
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MSPK_MAX_DEV_CACHE) return 256u;
  std::lock_guard<std::mutex> lock(mu);
  if (!cache[dev]) {
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return 256u;
    cache[dev] = (unsigned) pr.multiProcessorCount;
  }
  return cache[dev];
}
// a kernel launch whose status is RETURNED (hipLaunchKernelGGL leaves it in the thread's "last error", which is whoever's:
// an application's stale error made round 4's entry points fail, and clearing it on entry was the application's to do)
template <typename... P, typename... A>
static hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t st, A... a)
{
  static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
  std::tuple<P...> vals{ (P) a... };
#ifdef MSPACK_WAVE_EMU             /* tests/emu: the kernel is a host function, a launch runs it on the emulator's wave threads */
  (void) st;
  emu_launch(grid, block, [=]() { std::apply(kernel, vals); });
  return hipSuccess;
#else
  void *args[sizeof...(P)];
  size_t i = 0;
  std::apply([&](auto &... v) { ((args[i++] = (void *) &v), ...); }, vals);
  return hipLaunchKernel((const void *) kernel, grid, block, args, 0, st);
#endif
}
#define LK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
#ifdef MSPACK_HOST_CHECK
hipError_t hostcheck_launch_kind(unsigned kind, const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n,
                                 const void *d_in, void *d_out, mspack_hip_result *d_results, hipStream_t st);
#endif

static hipError_t launch_kind(unsigned kind, const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n,
                              const void *d_in, void *d_out, mspack_hip_result *d_results, void *d_fm, size_t n_frames_total,
                              size_t slot_lo, size_t n_slots, hipStream_t st, bool frame_tables = true, unsigned launch_ix = 0,
                              size_t n_rec_slots = (size_t) -1, bool alone = true, bool lzss_ring = false)
{
  if (n_rec_slots == (size_t) -1) n_rec_slots = n_frames_total;
  if (n == 0) return hipSuccess;
#ifdef MSPACK_HOST_CHECK      /* tests/hostcheck: the HOST half of this file under real sanitizers -- no kernel runs, a CPU stand-in takes the launch's place in the stream */
  return hostcheck_launch_kind(kind, d_units, d_order, n, d_in, d_out, d_results, st);
#endif
  const dim3 grid((unsigned) n), block(64);
  const u8 *const in = (const u8 *) d_in;
  u8 *const out = (u8 *) d_out;
  static const u32 hdr_init[8] = { 0u, 0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u };
  static const u32 hdr_init_stream[8] = { 0u, 0xFFFFFFFFu, 0u, 1u, 0u, 0u, 0u, 0u };
  switch (kind) {
  case MSPACK_HIP_KIND_LZX: {
    LzxScratch L = lzx_scratch(d_fm, n_frames_total, n_rec_slots);
    const bool frames = d_fm != nullptr && n_slots != 0 && !g_no_frames && frame_tables;
    // launches of one batch that run on different streams (host path, several chunks) have their own control words, and
    // their own part of the record pool: the part that belongs to their frame slots
    u32 *hdr = L.hdr + 8u * (launch_ix & 15u);
    uint2 *pool = L.pool + slot_lo * REC_SLOT_RECORDS;
    const u32 pool_chunks = (u32)(n_slots * REC_POOL_PER_SLOT);
    if (frames) {
      // one dependency-driven launch: parse and resolve tasks from a ticket counter (mspack_lzx_pipe)
      LK(hipMemsetAsync(L.frame_unit + slot_lo, 0xFF, n_slots * sizeof(u32), st));
      // (resolve tasks that take their frames up while they are parsed: only where every ticket finds a wave at once -- a resolve
      // wave that has started holds its slot until its frame's parse task is through -- and no other launch runs beside this one)
      const bool stream = (alone && g_stream_resolve != 0) || g_stream_resolve >= 2;      // (and the kernel knows how many tickets the launch has)
      LK(hipMemcpyAsync(hdr, stream ? hdr_init_stream : hdr_init, sizeof(hdr_init), hipMemcpyHostToDevice, st));
      LK(launch(mspack_lzx_pipe_map, dim3((unsigned)((n + 63) / 64)), block, st, d_units, d_order, (u32) n, L.frame_unit, L.recs, hdr));
      const size_t tickets = 2u * n_slots;
      // A launch that runs beside other chunks' launches asks for a third as many waves as it has tickets (MSPACK_HIP_CHUNK_WAVE_DIV): with
      // a wave for every ticket it ran unit-major, its resolve waves waiting on their slots for the parse waves -- slots the next chunk's
      // launch could use (the first chunk's 586 intervals were through after 1.9 ms instead of the 1.25 they take alone).  Headline batch
      // to the host 7.56-7.75 -> 7.38-7.48 ms, 1024 intervals to the device / host 2.16-2.24 / 3.38-3.47 -> 2.10-2.17 / 3.30-3.36 ms; 2 and 4
      // within 0.05 ms of 3 (profiles/round6_jobs.txt)
      static const size_t wave_div = (size_t) env_int("MSPACK_HIP_CHUNK_WAVE_DIV", 3, 1, 16);
      const unsigned waves = (unsigned) std::min<size_t>(alone ? tickets : std::max<size_t>(64, tickets / wave_div), lzx_pipe_waves());
      LK(launch(mspack_lzx_pipe, dim3(waves), block, st, d_units, d_order, (u32) n, (u32) slot_lo, (u32) n_slots, in, out, d_results,
                L.meta, L.frame_unit, hdr, L.recs, pool, pool_chunks, g_fold_policy, g_ticket_order));
      // few long units: the frames' copies as fold tasks, one wave per CU (the kernel decides from what the map kernel counted and
      // leaves at once otherwise; a launch of more units than the rule allows is not even asked)
      if (g_fold_policy >= 2u || (g_fold_policy == 1u && n <= LZX_FOLD_MAX_UNITS && n_slots >= LZX_FOLD_MIN_FRAMES))
        LK(launch(mspack_lzx_fold, dim3((unsigned) std::min<size_t>(n_slots, lzx_fold_waves())), dim3(FOLD_THREADS), st, d_units, (u32) slot_lo, (u32) n_slots,
                  out, L.frame_unit, hdr, L.recs, pool, g_fold_policy));
      // what the pipe leaves: the last bytes of every unit's input (the EOF-exact reader's), the look-ahead frame, frames
      // that are not one regular block, errors, E8, the results -- the unit kernel, resuming where each unit's chain of frames ended
      LK(launch(mspack_decode_lzx, grid, block, st, d_units, d_order, (u32) n, in, out, d_results, L.meta, L.recs, pool, 1u));
      break;
    }
    LK(launch(mspack_decode_lzx, grid, block, st, d_units, d_order, (u32) n, in, out, d_results, d_fm ? L.meta : (int32_t *) nullptr,
              (const lzxn::LzxFrameRec *) nullptr, (const uint2 *) nullptr, 0u));
    break; }
  case MSPACK_HIP_KIND_LZX_DELTA:
    LK(launch(mspack_decode_lzxd, grid, block, st, d_units, d_order, (u32) n, in, out, d_results, (int32_t *) d_fm)); break;
  case MSPACK_HIP_KIND_MSZIP: {
    LzxScratch L = lzx_scratch(d_fm, n_frames_total, n_rec_slots);
    const bool frames = d_fm != nullptr && n_slots != 0 && !g_no_frames && frame_tables;
    uint2 *pool = nullptr;
    u32 pool_chunks = 0;
    if (frames) {
      // one parse wave per CFDATA block first (mszip_kernel.hpp: "Block-level parse parallelism"); a pipe of the LZX kind
      // was measured slower here (profiles/round3_mszip.txt: the blocks' parse tasks do not depend on each other)
      u32 *hdr = L.hdr + 8u * (16u + (launch_ix & 15u));
      pool = L.pool + slot_lo * REC_SLOT_RECORDS;
      pool_chunks = (u32)(n_slots * REC_POOL_PER_SLOT);
      LK(hipMemsetAsync(L.frame_unit + slot_lo, 0xFF, n_slots * sizeof(u32), st));
      LK(hipMemcpyAsync(hdr, hdr_init, sizeof(hdr_init), hipMemcpyHostToDevice, st));
      LK(launch(mspack_lzx_frame_map, grid, block, st, d_units, d_order, (u32) n, L.frame_unit, L.recs, hdr, (u32) MSPACK_HIP_KIND_MSZIP));
      LK(launch(mspack_mszip_parse, dim3((unsigned) n_slots), block, st, d_units, d_order, (u32) n, (u32) slot_lo, (u32) n_slots, in, out,
                L.frame_unit, hdr, L.recs, pool, pool_chunks));
      if (g_fold_policy >= 2u || (g_fold_policy == 1u && n <= LZX_FOLD_MAX_UNITS && n_slots >= LZX_FOLD_MIN_FRAMES))
        LK(launch(mspack_mszip_fold, dim3((unsigned) std::min<size_t>(n_slots, lzx_fold_waves())), dim3(FOLD_THREADS), st, d_units, (u32) slot_lo, (u32) n_slots,
                  out, L.frame_unit, hdr, L.recs, pool, g_fold_policy));
    }
    LK(launch(mspack_decode_mszip, grid, block, st, d_units, d_order, (u32) n, in, out, d_results,
              frames ? L.recs : (lzxn::LzxFrameRec *) nullptr, pool));
    break; }
  case MSPACK_HIP_KIND_QUANTUM:
    LK(launch(mspack_decode_qtm, grid, block, st, d_units, d_order, (u32) n, in, out, d_results));
    LK(launch(mspack_decode_qtm_marks, grid, block, st, d_units, d_order, (u32) n, in, out, d_results)); break;
  case MSPACK_HIP_KIND_LZSS:
    LK(launch(mspack_decode_lzss, grid, block, st, d_units, d_order, (u32) n, in, out, d_results));
    // (units with MSPACK_HIP_UF_LZSS_RING: their own kernel, only when the caller says the list may hold one)
    if (lzss_ring) LK(launch(mspack_decode_lzss_ring, grid, block, st, d_units, d_order, (u32) n, in, out, d_results));
    break;
  case MSPACK_HIP_KIND_KWAJ_LZH:
    LK(launch(mspack_decode_kwaj_lzh, grid, block, st, d_units, d_order, (u32) n, in, out, d_results)); break;
  case MSPACK_HIP_KIND_XORSUM:
    LK(launch(mspack_xorsum, grid, block, st, d_units, d_order, (u32) n, in, d_results)); break;
  default: break;
  }
  return hipSuccess;
}
// the digest pass over units order[0..n): at most max_len bytes per unit.  Enough waves per unit for the longest one, as long as
// the grid stays near 64 Ki blocks (a block whose unit has no segment for it leaves at once)
static hipError_t launch_crc32(const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n, uint64_t max_len, void *d_out,
                               mspack_hip_result *d_results, hipStream_t st)
{
  if (n == 0) return hipSuccess;
#ifdef MSPACK_HOST_CHECK      /* tests/hostcheck runs no kernel and its stand-in for a launch computes no digest */
  return hipErrorInvalidValue;
#endif
  const uint64_t max_seg = std::max<uint64_t>(1, (max_len + 15u + CRC_SEG - 1u) / CRC_SEG);
  const u32 segs_y = (u32) std::min<uint64_t>(max_seg, std::max<uint64_t>(1, 65536u / n));
  LK(launch(mspack_crc32_init, dim3((unsigned)((n + 63) / 64)), dim3(64), st, d_units, d_order, (u32) n, d_results));
  LK(launch(mspack_crc32, dim3((unsigned)(n * segs_y)), dim3(64), st, d_units, d_order, (u32) n, segs_y, (const u8 *) d_out, d_results));
  return hipSuccess;
}
// the MD5 pass over the digest units order[0..n) (or, order == NULL, over every unit: lanes of other kinds leave): one lane each
static hipError_t launch_md5(const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n, const void *d_out, size_t out_bytes,
                             mspack_hip_result *d_results, hipStream_t st)
{
  if (n == 0) return hipSuccess;
#ifdef MSPACK_HOST_CHECK      /* tests/hostcheck runs no kernel and its stand-in for a launch computes no digest */
  return hipErrorInvalidValue;
#endif
  LK(launch(mspack_md5, dim3((unsigned)((n + 63) / 64)), dim3(64), st, d_units, d_order, (u32) n, (const u8 *) d_out, (u64) out_bytes, d_results));
  return hipSuccess;
}
// the SHA-1 / SHA-256 pass over the heads order[0..n) of a table of n_table units (or, order == NULL, over every unit: lanes of other
// kinds leave): one lane each, one launch per algorithm
static hipError_t launch_sha1(const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n, size_t n_table, const void *d_out, size_t out_bytes,
                              mspack_hip_result *d_results, hipStream_t st)
{
  if (n == 0) return hipSuccess;
#ifdef MSPACK_HOST_CHECK
  return hipErrorInvalidValue;
#endif
  LK(launch(mspack_sha1, dim3((unsigned)((n + 63) / 64)), dim3(64), st, d_units, d_order, (u32) n, (u32) n_table, (const u8 *) d_out, (u64) out_bytes, d_results));
  return hipSuccess;
}
static hipError_t launch_sha256(const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n, size_t n_table, const void *d_out, size_t out_bytes,
                                mspack_hip_result *d_results, hipStream_t st)
{
  if (n == 0) return hipSuccess;
#ifdef MSPACK_HOST_CHECK
  return hipErrorInvalidValue;
#endif
  LK(launch(mspack_sha256, dim3((unsigned)((n + 63) / 64)), dim3(64), st, d_units, d_order, (u32) n, (u32) n_table, (const u8 *) d_out, (u64) out_bytes, d_results));
  return hipSuccess;
}
#define SHA512_KINDS ((1u << MSPACK_HIP_KIND_SHA384) | (1u << MSPACK_HIP_KIND_SHA512))
// the SHA-384 / SHA-512 pass: one launch for the heads of both algorithms (`kinds`: which of the two are taken)
static hipError_t launch_sha512(const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n, size_t n_table, const void *d_out, size_t out_bytes,
                                mspack_hip_result *d_results, unsigned kinds, hipStream_t st)
{
  if (n == 0) return hipSuccess;
#ifdef MSPACK_HOST_CHECK
  return hipErrorInvalidValue;
#endif
  LK(launch(mspack_sha512, dim3((unsigned)((n + 63) / 64)), dim3(64), st, d_units, d_order, (u32) n, (u32) n_table, (const u8 *) d_out, (u64) out_bytes, d_results,
            (u32) kinds));
  return hipSuccess;
}
// waves of mspack_crc32r_pass: as many as the device holds at once, eight per CU at most (nothing depends on the number being right)
static unsigned crc32r_waves()
{
  static std::mutex mu;
  static unsigned cache[MSPK_MAX_DEV_CACHE] = { 0 };
  int dev = 0, per_cu = 0; hipDeviceProp_t pr;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MSPK_MAX_DEV_CACHE) return 2048u;
  std::lock_guard<std::mutex> lock(mu);
  if (!cache[dev]) {
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return 2048u;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mspack_crc32r_pass, 64, 0);
    if (e != hipSuccess || per_cu < 1) per_cu = 8;
    cache[dev] = (unsigned) pr.multiProcessorCount * (unsigned) std::min(per_cu, 8);
  }
  return cache[dev];
}
// the CRC-32 pass over the range units order[0..n) (or, order == NULL, over every unit: positions of other kinds own nothing): init, the
// one-wave scan, the pass -- a grid no larger than the tickets the list can hold, bounded by the device's waves --, finish
static hipError_t launch_crc32_ranges(const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n, const void *d_out, size_t out_bytes,
                                      mspack_hip_result *d_results, hipStream_t st)
{
  if (n == 0) return hipSuccess;
#ifdef MSPACK_HOST_CHECK      /* tests/hostcheck runs no kernel and its stand-in for a launch computes no digest */
  return hipErrorInvalidValue;
#endif
  const dim3 per_lane((unsigned)((n + 63) / 64)), block(64);
  const uint64_t most = (uint64_t) n * (std::min<uint64_t>(out_bytes, 0xFFFFFFFFu) / CRC_SEG + 2u);      // no list of n ranges has more tickets
  const unsigned waves = (unsigned) std::min<uint64_t>(most, crc32r_waves());
  LK(launch(mspack_crc32r_init, per_lane, block, st, d_units, d_order, (u32) n, (u64) out_bytes, d_results));
  LK(launch(mspack_crc32r_scan, dim3(1), block, st, d_units, d_order, (u32) n, (const u8 *) d_out, (u64) out_bytes, d_results));
  LK(launch(mspack_crc32r_pass, dim3(waves), block, st, d_units, d_order, (u32) n, (const u8 *) d_out, (u64) out_bytes, d_results));
  LK(launch(mspack_crc32r_finish, per_lane, block, st, d_units, d_order, (u32) n, (u64) out_bytes, d_results));
  return hipSuccess;
}
// waves of mspack_stored_pass: as many as the device holds at once, eight per CU at most (nothing depends on the number being right)
static unsigned stored_waves()
{
  static std::mutex mu;
  static unsigned cache[MSPK_MAX_DEV_CACHE] = { 0 };
  int dev = 0, per_cu = 0; hipDeviceProp_t pr;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MSPK_MAX_DEV_CACHE) return 2048u;
  std::lock_guard<std::mutex> lock(mu);
  if (!cache[dev]) {
    if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return 2048u;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mspack_stored_pass, 64, 0);
    if (e != hipSuccess || per_cu < 1) per_cu = 8;
    cache[dev] = (unsigned) pr.multiProcessorCount * (unsigned) std::min(per_cu, 8);
  }
  return cache[dev];
}
// the stored units order[0..n) (or, order == NULL, every unit: positions of other kinds own nothing): the one-wave scan, the pass -- a
// grid no larger than the tickets the list can hold, bounded by the device's waves --, the results
static hipError_t launch_stored(const mspack_hip_unit *d_units, const uint32_t *d_order, size_t n, const void *d_in, size_t in_bytes, void *d_out,
                                size_t out_bytes, mspack_hip_result *d_results, hipStream_t st)
{
  if (n == 0) return hipSuccess;
#ifdef MSPACK_HOST_CHECK      /* tests/hostcheck runs no kernel and its stand-in for a launch copies nothing */
  return hipErrorInvalidValue;
#endif
  const dim3 per_lane((unsigned)((n + 63) / 64)), block(64);
  const uint64_t most = (uint64_t) n * (std::min<uint64_t>(out_bytes, 0xFFFFFFFFu) / STORED_SEG + 2u);      // no list of n units has more tickets
  const unsigned waves = (unsigned) std::min<uint64_t>(most, stored_waves());
  LK(launch(mspack_stored_scan, dim3(1), block, st, d_units, d_order, (u32) n, (u64) in_bytes, (const u8 *) d_out, (u64) out_bytes, d_results));
  LK(launch(mspack_stored_pass, dim3(waves), block, st, d_units, d_order, (u32) n, (const u8 *) d_in, (u64) in_bytes, (u8 *) d_out, (u64) out_bytes, d_results));
  LK(launch(mspack_stored_results, per_lane, block, st, d_units, d_order, (u32) n, (u64) in_bytes, (u64) out_bytes, d_results));
  return hipSuccess;
}
#undef LK

extern "C" {

#ifdef SPQ_TIMERS
/* analysis builds only: read (and clear) the resolve cycle counters of block 0's wave */
int mspack_hip_debug_counters(unsigned long long *out8) {
  unsigned long long z[8] = {0};
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(spq_tm), sizeof(z)) != hipSuccess) return -1;
  return hipMemcpyToSymbol(HIP_SYMBOL(spq_tm), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef QTM_TIMERS
int mspack_hip_debug_qtm_timers(unsigned long long *out8) {
  return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_qtm_tm), 64) == hipSuccess ? 0 : -1;
}
#endif
#ifdef FOLD_TRACE
int mspack_hip_debug_fold_phases(unsigned long long *out16) {
  unsigned long long z[16] = {0};
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_fold_phase), sizeof(z)) != hipSuccess) return -1;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_fold_phase), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
#ifdef LZX_PIPE_TRACE
int mspack_hip_debug_pipe_trace(unsigned long long *out, size_t n_words) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pipe_trace), n_words * 8) == hipSuccess ? 0 : -1;
}
/* ticks (100 MHz) per phase summed over all waves: lzxp:: phases 0-8 (parse task), lzxn:: phases 9-11 (commit task); cleared on read */
int mspack_hip_debug_pipe_phases(unsigned long long *out32) {
  unsigned long long z[16] = {0};
  if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(lzxp::g_pipe_phase), sizeof(z)) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out32 + 16, HIP_SYMBOL(lzxn::g_pipe_phase), sizeof(z)) != hipSuccess) return -1;
  hipMemcpyToSymbol(HIP_SYMBOL(lzxp::g_pipe_phase), z, sizeof(z));
  return hipMemcpyToSymbol(HIP_SYMBOL(lzxn::g_pipe_phase), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
/* diagnostic (always compiled): what the frame-parallel tasks left in the records of frame slots [first_slot, first_slot + n_slots) of a
 * caller's own scratch -- which path took a frame.  8 words per slot; LZX: status, n_tokens, bytes_done, chain, rst, rs_valid, rs_frame,
 * rs_partial; MSZIP (through ZipBlockRec): status, n_tokens, total_out, fold, then zeros.  Synchronous copies: the caller has
 * synchronised the stream its batch ran on.  Nothing on the decode path reads or writes anything for it */
int mspack_hip_debug_frame_words(const void *d_frame_scratch, size_t n_frames_total, size_t first_slot, size_t n_slots, int mszip,
                                 uint32_t *out)
{
  if (!d_frame_scratch || !out || first_slot > n_frames_total + 1 || n_slots > n_frames_total + 1 - first_slot) {
    snprintf(g_err, sizeof(g_err), "mspack_hip_debug_frame_words: no scratch, or slots beyond it");
    return -1;
  }
  const LzxScratch L = lzx_scratch(const_cast<void *>(d_frame_scratch), n_frames_total, n_frames_total);
  for (size_t i = 0; i < n_slots; i++) {
    alignas(16) unsigned char raw[sizeof(lzxn::LzxFrameRec)];
    CK(hipMemcpy(raw, &L.recs[first_slot + i], sizeof(raw), hipMemcpyDeviceToHost));
    uint32_t *w = out + 8 * i;
    if (mszip) {
      const ZipBlockRec *z = (const ZipBlockRec *) raw;
      w[0] = z->status; w[1] = z->n_tokens; w[2] = z->total_out; w[3] = z->fold; w[4] = w[5] = w[6] = w[7] = 0u;
    }
    else {
      const lzxn::LzxFrameRec *r = (const lzxn::LzxFrameRec *) raw;
      w[0] = r->status; w[1] = r->n_tokens; w[2] = r->bytes_done; w[3] = r->chain; w[4] = r->rst; w[5] = r->rs_valid; w[6] = r->rs_frame;
      w[7] = r->rs_partial;
    }
  }
  return 0;
}
const char *mspack_hip_version(void) { return "mspack-hip 0.4 (gfx950; LZX/LZX-DELTA/Quantum/MSZIP batch decode)"; }
const char *mspack_hip_last_error(void) { return g_err; }
unsigned mspack_hip_features(void) { return MSPACK_HIP_FEAT_CRC32 | MSPACK_HIP_FEAT_MD5 | MSPACK_HIP_FEAT_SHA1 | MSPACK_HIP_FEAT_SHA256 | MSPACK_HIP_FEAT_SLOTS | MSPACK_HIP_FEAT_LZSS_RING | MSPACK_HIP_FEAT_CRC32_RANGES |
         MSPACK_HIP_FEAT_SHA384 | MSPACK_HIP_FEAT_SHA512 | MSPACK_HIP_FEAT_STORED; }

int mspack_hip_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { fail(e, "hipGetDeviceCount"); return 0; }
  return n;
}
int mspack_hip_set_device(int device) { CK(hipSetDevice(device)); return 0; }

size_t mspack_hip_frame_scratch_bytes(size_t n_frames_total) { return lzx_scratch(nullptr, n_frames_total, n_frames_total).bytes; }

int mspack_hip_decode_batch_device(const mspack_hip_unit *d_units, const uint32_t *d_order,
                                   size_t n_units, const void *d_in, size_t in_bytes,
                                   void *d_out, size_t out_bytes, mspack_hip_result *d_results,
                                   void *d_frame_scratch, size_t n_frames_total, unsigned kind_mask,
                                   void *stream)
{
  if (n_units == 0) return 0;
  if ((kind_mask & 0x31309FEu) == 0) kind_mask |= 0x8FEu;  // bit k = units of kind k may be present; none = every codec, stored units included (and no digest units)
  // the caller's unit table lives on the device, so the kinds cannot be compacted here: every codec in the
  // mask gets the whole grid and blocks of other kinds leave at once.  Callers with mixed batches pass one
  // order list per codec and a one-bit mask (what the host-buffer entry points below do).
  for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++)
    if (kind_mask & (1u << k))
      CK(launch_kind(k, d_units, d_order, n_units, d_in, d_out, d_results, d_frame_scratch, n_frames_total, 0, n_frames_total,
                     (hipStream_t) stream, (kind_mask & MSPACK_HIP_MASK_FRAME_TABLES) != 0u, 0, (size_t) -1, true,
                     (kind_mask & MSPACK_HIP_MASK_LZSS_RING) != 0u));
  // the stored units' copy (three launches): in front of the digest passes like every kernel that stores into the arena
  if (kind_mask & (1u << MSPACK_HIP_KIND_STORED))
    CK(launch_stored(d_units, d_order, n_units, d_in, in_bytes, d_out, out_bytes, d_results, (hipStream_t) stream));
  // (the flags are on the device too: the digest pass is launched only when the caller says some unit may carry MSPACK_HIP_UF_CRC32)
  if (kind_mask & MSPACK_HIP_MASK_CRC32)
    CK(launch_crc32(d_units, d_order, n_units, std::min<uint64_t>(out_bytes, 0xFFFFFFFFu), d_out, d_results, (hipStream_t) stream));
  // the MD5 pass, behind everything that stores into the arena: only when the caller says digest units may be present
  if (kind_mask & (1u << MSPACK_HIP_KIND_MD5))
    CK(launch_md5(d_units, d_order, n_units, d_out, out_bytes, d_results, (hipStream_t) stream));
  // ... and the SHA-1 / SHA-256 passes, one launch per algorithm
  if (kind_mask & (1u << MSPACK_HIP_KIND_SHA1))
    CK(launch_sha1(d_units, d_order, n_units, n_units, d_out, out_bytes, d_results, (hipStream_t) stream));
  if (kind_mask & (1u << MSPACK_HIP_KIND_SHA256))
    CK(launch_sha256(d_units, d_order, n_units, n_units, d_out, out_bytes, d_results, (hipStream_t) stream));
  // ... and the SHA-384 / SHA-512 pass, one launch for both
  if (kind_mask & SHA512_KINDS)
    CK(launch_sha512(d_units, d_order, n_units, n_units, d_out, out_bytes, d_results, kind_mask & SHA512_KINDS, (hipStream_t) stream));
  // ... and the CRC-32 range units' pass (four launches)
  if (kind_mask & (1u << MSPACK_HIP_KIND_CRC32))
    CK(launch_crc32_ranges(d_units, d_order, n_units, d_out, out_bytes, d_results, (hipStream_t) stream));
  return 0;
}

double mspack_hip_time_batch_device(const mspack_hip_unit *d_units, const uint32_t *d_order,
                                    size_t n_units, const void *d_in, size_t in_bytes,
                                    void *d_out, size_t out_bytes, mspack_hip_result *d_results,
                                    void *d_frame_scratch, size_t n_frames_total, unsigned kind_mask,
                                    void *stream, int iters)
{
  hipEvent_t e0, e1;
  float ms = 0;
  if (iters < 1) iters = 1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
  hipEventRecord(e0, (hipStream_t) stream);
  for (int i = 0; i < iters; i++) {
    int rc = mspack_hip_decode_batch_device(d_units, d_order, n_units, d_in, in_bytes, d_out, out_bytes,
                                            d_results, d_frame_scratch, n_frames_total, kind_mask, stream);
    if (rc) { hipEventDestroy(e0); hipEventDestroy(e1); return -1.0; }
  }
  hipEventRecord(e1, (hipStream_t) stream);
  if (hipEventSynchronize(e1) != hipSuccess) { hipEventDestroy(e0); hipEventDestroy(e1); return -1.0; }
  hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  return (double) ms / iters;
}

} // extern "C"
