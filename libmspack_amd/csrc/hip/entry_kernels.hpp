// entry_kernels.hpp -- every __global__ entry point of the library and the layout of the work scratch they share.
// Included once by shim.hip, behind the decoders' role headers (the lzxn / lzxd / lzxp namespaces, MSZIP, Quantum, LZSS, CRC-32).
#pragma once
// One wavefront == one workgroup == one unit.  blockIdx -> unit through the optional launch order
// (longest unit first keeps the tail of the batch short).  One kernel per codec (their register
// budgets differ a lot); a block whose unit belongs to another codec exits at once.
__device__ __forceinline__ bool pick_unit(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                                          u32 kind, u32 &ui)
{
  u32 b = blockIdx.x;
  if (b >= n_units) return false;
  ui = rfl(order ? order[b] : b);
  return units[ui].kind == kind;
}

// ---- LZX / MSZIP work scratch (d_frame_scratch of the C ABI), n = n_frames_total + 1 frame slots ----------------
//   int32  meta[n]        per frame: intel_filesize to apply in the E8 pass (0 = none)
//   u32    frame_unit[n]  per frame slot: the unit it belongs to when a parse wave should take it, else ~0
//   u32    hdr[256]       per launch (up to 32 concurrent ones) 8 words: [0] = most, [1] = fewest frames of a unit with a
//                         frame table, [2] = ticket counter of mspack_lzx_pipe, [4] = chunks handed out of the launch's pool
//   LzxFrameRec recs[n]   what the parse wave of that frame assumed and found (lzx_pipe.hpp), incl. its chunk list
//   uint2  pool[n * REC_POOL_PER_SLOT * REC_CHUNK]   the frames' match records (wave_common.hpp: RecPool): 48 KiB per slot
//                         on average instead of round 3's 128 KiB worst case per slot; a launch uses the part that
//                         belongs to its slot range
struct LzxScratch { int32_t *meta; u32 *frame_unit; u32 *hdr; lzxn::LzxFrameRec *recs; uint2 *pool; size_t bytes; };
// n_rec_slots: frame slots that can hold a record + records -- all of them for a caller's own scratch (the size
// mspack_hip_frame_scratch_bytes states); the host path numbers the units that carry a table first and gives only those
// a record and a share of the pool (a batch of OAB blocks or of folders without tables needs the 4-byte meta words only)
#define REC_SLOT_RECORDS ((size_t) REC_POOL_PER_SLOT * REC_CHUNK)
__host__ __device__ static inline LzxScratch lzx_scratch(void *base, size_t n_frames_total, size_t n_rec_slots)
{
  const size_t n0 = n_frames_total + 1, n = n_rec_slots + 1, a = 255;
  const size_t o_fu = (n0 * 4 + a) & ~a, o_hdr = o_fu + ((n * 4 + a) & ~a), o_rec = o_hdr + 1024,
               o_pool = (o_rec + n * sizeof(lzxn::LzxFrameRec) + a) & ~a;
  LzxScratch L;
  const uintptr_t b = (uintptr_t) base;                  // (a NULL base only asks for the size: no arithmetic on a null POINTER)
  L.meta = (int32_t *) b; L.frame_unit = (u32 *)(b + o_fu); L.hdr = (u32 *)(b + o_hdr); L.recs = (lzxn::LzxFrameRec *)(b + o_rec);
  L.pool = (uint2 *)(b + o_pool);
  L.bytes = o_pool + n * REC_SLOT_RECORDS * sizeof(uint2);
  return L;
}

// one unit's frame slots: which of them get a parse wave, and the launch's minimum / maximum frames per unit
__device__ __forceinline__ void frame_map_unit(const mspack_hip_unit &u, const u32 ui, u32 *frame_unit, lzxn::LzxFrameRec *recs,
                                               u32 *hdr, const u32 kind)
{
  const u32 nreal = (u.out_len + LZX_FRAME - 1u) / LZX_FRAME;
  const bool usable = (u.flags & MSPACK_HIP_UF_FRAME_TABLE) != 0u && !(kind == MSPACK_HIP_KIND_MSZIP && (u.flags & (MSPACK_HIP_UF_MSZIP_REPAIR | MSPACK_HIP_UF_MSZIP_KWAJ)));
  // frame slots of a unit: LZX out_len/32768 + 1 (one spare for the look-ahead frame), MSZIP with a table one per block
  const u32 nslots = kind == MSPACK_HIP_KIND_LZX ? u.out_len / LZX_FRAME + 1u : (usable ? nreal : 0u);
  if (threadIdx.x == 0) {                   // (a plain look first: 4096 atomics on one word take 0.1 ms)
    const u32 v = usable ? nreal : 0u;
    if (hdr[0] < v) atomicMax(&hdr[0], v);
    if (hdr[1] > v) atomicMin(&hdr[1], v);
  }
  // (units without a usable table own no record slots -- the host path numbers them behind the last slot that has a
  // record: nothing of theirs is written here; frame_unit[] is preset to ~0 for the launch's slot range)
  if (!usable) return;
  for (u32 f = threadIdx.x; f < nslots; f += 64u) {
    frame_unit[u.frame_base + f] = f < nreal ? ui : 0xFFFFFFFFu;
    recs[u.frame_base + f].status = 0u;
    if (kind == MSPACK_HIP_KIND_MSZIP) ((ZipBlockRec *) &recs[u.frame_base + f])->fold = 0u;
  }
  if (threadIdx.x == 0 && kind == MSPACK_HIP_KIND_MSZIP) atomicAdd(&hdr[5], 1u);      // (units with a table: mspack_mszip_fold's rule)
}

// the same for mspack_lzx_pipe, one unit per LANE (4096 one-wave blocks with two atomics each on the same words took
// 0.19 ms): frame slots -> unit, record status words cleared, most / fewest frames per unit reduced per wave first
__global__ __launch_bounds__(64)
void mspack_lzx_pipe_map(const mspack_hip_unit *units, const u32 *order, u32 n_units, u32 *frame_unit,
                         lzxn::LzxFrameRec *recs, u32 *ctl)
{
  const u32 j = blockIdx.x * 64u + threadIdx.x;
  u32 fr = 0;                                                    // real frames of a unit whose frames get parse tasks
  bool other = false;
  if (j < n_units) {
    const u32 ui = order ? order[j] : j;
    const mspack_hip_unit u = units[ui];
    if (u.kind == MSPACK_HIP_KIND_LZX) {
      const bool usable = (u.flags & MSPACK_HIP_UF_FRAME_TABLE) != 0u;
      const u32 nreal = (u.out_len + LZX_FRAME - 1u) / LZX_FRAME, nslots = u.out_len / LZX_FRAME + 1u;
      // (a unit without a table owns no record slots: the host path numbers such units behind the last slot that has a
      // record, so nothing of theirs may be written -- frame_unit[] is preset to ~0 for the launch's slot range)
      if (usable) {
        for (u32 f = 0; f < nslots; f++) {
          frame_unit[u.frame_base + f] = f < nreal ? ui : 0xFFFFFFFFu;
          recs[u.frame_base + f].status = 0u;
          recs[u.frame_base + f].chain = 0u;
          recs[u.frame_base + f].rst = 0u;
        }
        recs[u.frame_base].rs_valid = 0u;
        // (what decides between lzx_pipe_resolve and mspack_lzx_fold: how many units carry a table; positions beyond 2^31 do not fit the fold's map)
        atomicAdd(&ctl[5], 1u);
        if (u.out_len > 0x7FFF0000u) atomicOr(&ctl[6], 1u);
      }
      fr = usable ? nreal : 0u;
    }
    else other = true;
  }
  const u32 live = j < n_units ? 1u : 0u;
  u32 mx = fr, mn = (live && !other) ? fr : (other ? 0u : 0xFFFFFFFFu);
  for (int o = 32; o >= 1; o >>= 1) {
    const u32 a = (u32) __builtin_amdgcn_ds_bpermute((int)(((threadIdx.x + (u32) o) & 63u) << 2), (int) mx);
    const u32 b = (u32) __builtin_amdgcn_ds_bpermute((int)(((threadIdx.x + (u32) o) & 63u) << 2), (int) mn);
    mx = a > mx ? a : mx; mn = b < mn ? b : mn;
  }
  if (threadIdx.x == 0) { atomicMax(&ctl[0], mx); atomicMin(&ctl[1], mn); }
}

// which frame slots get a parse wave: the real frames of LZX units that carry a frame table
__global__ __launch_bounds__(64)
void mspack_lzx_frame_map(const mspack_hip_unit *units, const u32 *order, u32 n_units, u32 *frame_unit,
                          lzxn::LzxFrameRec *recs, u32 *hdr, u32 kind)
{
  u32 ui;
  if (!pick_unit(units, order, n_units, kind, ui)) { if (threadIdx.x == 0 && hdr[1] != 0u) atomicMin(&hdr[1], 0u); return; }
  frame_map_unit(units[ui], ui, frame_unit, recs, hdr, kind);
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4)))
void mspack_decode_lzx(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                       const u8 *in_arena, u8 *out_arena, mspack_hip_result *results,
                       int32_t *frame_meta, const lzxn::LzxFrameRec *recs, const uint2 *toks, u32 resume)
{
  __shared__ lzxn::LzxShared sh;
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_LZX, ui)) return;
  const mspack_hip_unit u = units[ui];
  mspack_hip_result *res = &results[ui];
  const u32 lane = threadIdx.x;
  lzxn::lzx_decode_unit(u, in_arena, out_arena, frame_meta, res, &sh, recs, toks, resume != 0u);
  // E8 translation, frame by frame, once the unit no longer needs its window (lzxd.c:706-736)
  if (frame_meta) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    u32 produced = rfl(res->out_len);
    u32 nfr = (produced + LZX_FRAME - 1u) / LZX_FRAME;
    for (u32 f = 0; f < nfr; f++) {
      int32_t fs = (int32_t) rfl((u32) frame_meta[u.frame_base + f]);
      if (fs == 0) continue;
      // the frame size the decoder saw: full frames except the last one of the stream
      u32 fsize = u.out_len - f * LZX_FRAME; if (fsize > LZX_FRAME) fsize = LZX_FRAME;
      lzxn::lzx_e8_frame(out_arena + u.out_off + (size_t) f * LZX_FRAME, fsize,
                         (int32_t)((u32) u.e8_base + f * LZX_FRAME), fs, lane);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// mspack_lzx_pipe -- headers, parse and match resolution of a launch's LZX units as ONE dependency-driven launch.
//
// Persistent waves pull TICKETS from a counter; a ticket is the task of one FRAME of one unit:
//   parse (lzx_pipe_parse):     header chain link (waits for the previous frame's code lengths), tables, tokens: literals
//                               stored in place, one record per match;
//   resolve (lzx_pipe_resolve): waits until the unit's previous frame is complete, checks that this frame continues it,
//                               resolves R0-R2 along the records and copies the matches, publishes the frame as complete.
// Tickets are handed out in an order in which every task only waits for tasks with EARLIER tickets -- frame-major (all first
// frames in launch order, longest unit first, then all second frames, ...) when all units have the same number of frames,
// else in frame-slot order (a unit's frames in a row).  No co-residency is assumed: a ticket is pulled by a running wave,
// so whatever a task waits for is held by a live wave or done.  Round 3 had a separate COMMIT task per unit behind the
// unit's last parse task; its ~1-1.8 ms chain was what a launch ended with (waves busy 0.77 of the span).  Now all tasks
// are alike, a wave that took a long first frame takes a short second frame (launch order is longest first in every
// section), and a unit of many frames has the parse of frame f + k running beside the copies of frame f.
// Hand-off: payload by plain stores, agent-scope release, relaxed status store; the reader polls the status relaxed, then
// one agent-scope acquire (lzx_pipe.hpp).  The first frame that is not a complete regular one ends its unit's chain and
// says where serial decoding resumes; mspack_decode_lzx (launched behind the pipe) finishes every unit.
// ---------------------------------------------------------------------------------------------------
// ---- few units of many frames: the folder's chain as one gather pass per frame (lzx_fold.hpp) ----
// Decided per launch from what the map kernel counted (ctl[0] = most frames of a unit with a table, ctl[5] = such units, ctl[6] =
// some unit is too long for the map's positions): policy 0 never, 1 when it pays, 2 whenever it can (tests).  Where it pays: the
// resolve tasks of lzx_pipe_resolve fill 16 waves per CU and cost ~0.25 ms per frame ON a unit's chain; the fold tasks fill ONE wave
// per CU (128 KiB of LDS each) and leave ~15 us per frame on the chain -- so: long units, and too few of them to fill the chip.
#define LZX_FOLD_MIN_FRAMES 4u
#define LZX_FOLD_MAX_UNITS 128u
// (measured, tools/fold_policy_sweep.py, profiles/round6_fold_policy.txt: n folders of f frames, LZX, resolve tasks / fold tasks, ms:
//  4 x 256: 68.5 / 13.4; 16 x 64: 20.9 / 8.3; 32 x 32: 12.2 / 6.5; 64 x 16: 8.1 / 6.0; 128 x 8: 6.2 / 5.8; 128 x 4: 2.7 / 3.1;
//  256 x 8: 8.3 / 9.0 -- so: at most 128 units, and eight frames in the longest, or at least four when every frame gets a task of its
//  own at once; MSZIP folders gain at 128 x 4 too (2.6 / 2.2): four blocks)
#define LZX_FOLD_LONG_FRAMES 8u
__device__ __forceinline__ bool lzx_fold_on(const u32 *ctl, const u32 policy, const u32 n_slots, const bool mszip)
{
  if (policy == 0u || rfl(ctl[6]) != 0u || rfl(ctl[0]) == 0u) return false;
  if (policy >= 2u) return true;
  const u32 fmax = rfl(ctl[0]);
  if (rfl(ctl[5]) > LZX_FOLD_MAX_UNITS || fmax < LZX_FOLD_MIN_FRAMES) return false;
  return mszip || fmax >= LZX_FOLD_LONG_FRAMES || n_slots <= 256u;
}
// (a workgroup of FOLD_WAVES waves per task: fold_common.hpp; wave 0 pulls the tickets)
#define FOLD_TICKET(counter)                                                      \
  if (threadIdx.x == 0) sh.ctl[0] = atomicAdd(counter, 1u);                      \
  fold_barrier();                                                                 \
  const u32 t = rfl(sh.ctl[0]);                                                   \
  fold_barrier();                                    /* (the word is free again) */
// A unit whose matches are long RUNS (the reference's large-files.test: ~127 matches of 257 bytes per frame, one line repeated) is
// better off with lzx_pipe_resolve: its run fill writes such a frame without reading anything back (spec_queue.hpp), while a fold
// task would gather every byte (measured: 1.55-1.78 GB/s against 1.2).  Decided per unit from its FIRST frame's record -- every task
// of the unit, in both kernels, reads the same final words: at least 16 matches, and 96 bytes of output or more per match.
__device__ __forceinline__ bool lzx_unit_runs(const lzxn::LzxFrameRec *r0)
{
  u32 st = lzxn::lzx_status_load(&r0->status);
  // (the unit's first parse task has the unit's earliest ticket: a live wave holds it, or it is done)
  for (u32 tries = 0; (st == LZX_ST_NONE || st == LZX_ST_CLAIMED || st == LZX_ST_HEADER) && tries < (1u << 24); tries++) {
    __builtin_amdgcn_s_sleep(8);
    st = lzxn::lzx_status_load(&r0->status);
  }
  if (st != LZX_ST_EMITTED) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const u32 n = rfl(gld(&r0->n_tokens)), b = rfl(gld(&r0->bytes_done));
  return n >= 16u && b >= 96u * n;
}
__global__ __launch_bounds__(FOLD_THREADS)
void mspack_lzx_fold(const mspack_hip_unit *units, u32 slot_lo, u32 n_slots, u8 *out_arena, const u32 *frame_unit, u32 *ctl,
                     lzxn::LzxFrameRec *recs, const uint2 *toks, u32 fold_policy)
{
  __shared__ lzxn::LzxFoldLds sh;
  if (!lzx_fold_on(ctl, fold_policy, n_slots, false)) return;
  for (;;) {
    FOLD_TICKET(&ctl[7])
    if (t >= n_slots) break;
    const u32 slot = slot_lo + t;
    const u32 ui = rfl(frame_unit[slot]);
    if (ui == 0xFFFFFFFFu) continue;
    const mspack_hip_unit u = units[ui];
    if (u.kind != MSPACK_HIP_KIND_LZX || !(u.flags & MSPACK_HIP_UF_FRAME_TABLE)) continue;
    if (fold_policy == 1u && lzx_unit_runs(&recs[u.frame_base])) continue;      // (resolved by the pipe's own tasks; policy 2 folds these too: tests)
    lzxn::lzx_fold_frame(u, slot - u.frame_base, out_arena, &recs[u.frame_base], toks, &sh);
    fold_barrier();                                   // the next task reuses the LDS
  }
}

union LzxPipeLds { lzxp::LzxShared p; lzxn::LzxResolveLds r; };
static_assert(sizeof(LzxPipeLds) <= 10240, "16 waves per CU");

// the two halves of a task are real calls: each gets its own register allocation (inlined into the ticket loop they spill)
__device__ __attribute__((noinline)) u32 lzx_pipe_task_parse(const mspack_hip_unit *up, const u32 f, const u8 *in_arena, u8 *out_arena,
                                                             lzxn::LzxFrameRec *recs, uint2 *pool, u32 *pool_head, const u32 pool_chunks,
                                                             lzxp::LzxShared *sh, const u32 spec, const u32 stream)
{
  const mspack_hip_unit u = *up;
  RecPool rp; rp.base = pool; rp.head = pool_head; rp.cap = pool_chunks;
  return lzxp::lzx_pipe_parse(u, up, f, in_arena, out_arena, (lzxp::LzxFrameRec *) &recs[u.frame_base], rp, sh, stream != 0u, spec != 0u);
}
// (the rest of a frame whose first block ended inside it: one frame in a few hundred)
__device__ __attribute__((noinline)) void lzx_pipe_task_tail(const mspack_hip_unit *up, const u32 f, const u8 *in_arena, u8 *out_arena,
                                                             lzxn::LzxFrameRec *recs, uint2 *pool, u32 *pool_head, const u32 pool_chunks,
                                                             lzxp::LzxShared *sh)
{
  RecPool rp; rp.base = pool; rp.head = pool_head; rp.cap = pool_chunks;
  lzxp::lzx_pipe_parse_tail(up, f, in_arena, out_arena, (lzxp::LzxFrameRec *) &recs[rfl(up->frame_base)], rp, sh);
}
// (a frame's block header read ahead of the header chain, while the frame below is not that far: lzx_pipe_parse.hpp)
__device__ __attribute__((noinline)) u32 lzx_pipe_task_spec(const mspack_hip_unit *up, const u32 f, const u8 *in_arena, const lzxn::LzxFrameRec *recs,
                                                            lzxp::LzxShared *sh)
{
  const u32 rf = rfl((u32) up->reset_frames);
  if (rf ? (f % rf) == 0u : f == 0u) return 0u;                 // (a frame that starts a reset interval has no chain below it)
  const lzxn::LzxFrameRec *pr = &recs[rfl(up->frame_base) + f - 1u];
  const u32 ps = lzxn::lzx_status_load(&pr->status);
  if (ps != LZX_ST_NONE && ps != LZX_ST_CLAIMED) return 0u;     // the frame below is there: nothing to wait for, nothing to guess
  const u32 in_len = rfl(up->in_len);
  const u32 fo = rfl(((const u32 *)(in_arena + (size_t) rfl(up->in_chunk) * 4u))[f]);
  if (fo >= in_len || in_len - fo <= 64u) return 0u;
  return rfl(lzxp::lzx_pipe_spec_header(up, fo, in_arena, sh) ? 1u : 0u);
}
__device__ __attribute__((noinline)) void lzx_pipe_task_resolve(const mspack_hip_unit *up, const u32 f, u8 *out_arena, lzxn::LzxFrameRec *recs,
                                                                uint2 *toks, lzxn::LzxResolveLds *rl, const bool merged)
{
  const mspack_hip_unit u = *up;
  lzxn::lzx_pipe_resolve(u, f, out_arena, &recs[u.frame_base], toks, rl, merged);
}
// (the same where the launch has wave slots to spare: the frame's records taken up while it is parsed -- lzx_pipe_resolve.hpp)
__device__ __attribute__((noinline)) void lzx_pipe_task_resolve_stream(const mspack_hip_unit *up, const u32 f, u8 *out_arena, lzxn::LzxFrameRec *recs,
                                                                       uint2 *toks, lzxn::LzxResolveLds *rl)
{
  const mspack_hip_unit u = *up;
  lzxn::lzx_pipe_resolve_stream(u, f, out_arena, &recs[u.frame_base], toks, rl);
}

#ifdef LZX_PIPE_TRACE      /* analysis builds: one line per ticket = start, end (s_memrealtime, 100 MHz), task, time waited */
__device__ unsigned long long g_pipe_trace[4 << 16];
#endif
#define LZX_PIPE_WAVES_PER_EU 4
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LZX_PIPE_WAVES_PER_EU)))
void mspack_lzx_pipe(const mspack_hip_unit *units, const u32 *order, u32 n_units, u32 slot_lo, u32 n_slots,
                     const u8 *in_arena, u8 *out_arena, mspack_hip_result *results, int32_t *frame_meta,
                     const u32 *frame_unit, u32 *ctl, lzxn::LzxFrameRec *recs, uint2 *toks, u32 pool_chunks, u32 fold_policy, u32 order_mode)
{
  __shared__ LzxPipeLds sh;
  const u32 lane = threadIdx.x;
  // all units carry a table and have the same number of frames F (CHM reset intervals): 2 * F sections of n_units tickets,
  // each in launch order (longest unit first) -- P(frame 0), ..., P(frame F-1), R(frame 0), ..., R(frame F-1).  A task's
  // dependencies lie at least a section back, so with more units than waves nobody waits (one task per frame -- parse +
  // resolve -- was measured first: the waves that finish the short first frames early take the LONGEST units' second
  // frames and then sit on their slots until those units' first frames are through: 253 us waited per task, headline 3.25 ms).
  // Otherwise: one ticket per frame slot, parse + resolve by the same wave, a unit's frames in a row.
  const u32 Fmax = rfl(ctl[0]), Fmin = rfl(ctl[1]);
  // few units of many frames: this launch only PARSES (a unit's frames in a row: the header chain); mspack_lzx_fold, launched behind
  // it, does what lzx_pipe_resolve would have done (lzx_fold.hpp)
  const bool fold = lzx_fold_on(ctl, fold_policy, n_slots, false);
  // control word 3 (the host's): this launch has a wave for every ticket and nothing runs beside it -- resolve tasks take their
  // frames up while they are parsed (lzx_pipe_resolve_stream)
  const u32 stream_ok = rfl(ctl[3]);
  const u32 F = (Fmax != 0u && Fmax == Fmin && !fold) ? Fmax : 0u;
  const u32 T = F ? 2u * n_units * F : n_slots;
  const u32 stream = (stream_ok != 0u && F != 0u && T <= gridDim.x) ? 1u : 0u;      // (every ticket finds a wave at once)
  // Ticket order of a uniform launch (round 6; measured: profiles/round6_ticket_order.txt).  Every order is correct -- a task only
  // ever waits for earlier tickets --; what differs is who runs beside whom.  Level order (P(f0) | P(f1) | R(f0) | R(f1), §4.1c) is
  // right when the launch has about as many units as the chip has waves: nobody waits.  When every ticket finds a wave at once
  // (T <= gridDim.x: 1024 intervals) the order only says which tasks share a CU, and level order gives a CU sixteen tasks of ONE
  // kind -- unit-major (a unit's tasks in a row) mixes them: 1.53 -> 1.40 ms.  With many more units than waves, sections that
  // alternate P(f_k) and R(f_k-1) keep parse and resolve waves side by side through the launch: 8192 intervals 5.34 -> 5.24 ms.
  // order_mode: 0 level, 1 mixed sections, 2 unit-major; 3 (the default) = by the launch's shape.
  u32 mode = order_mode;
  if (mode >= 3u) mode = T <= gridDim.x ? 2u : (2u * n_units >= 3u * gridDim.x ? 1u : 0u);
  for (;;) {
    u32 t = 0;
    if (lane == 0) t = atomicAdd(&ctl[2], 1u);
    t = rfl(t);
    if (t >= T) break;
    u32 ui = 0xFFFFFFFFu, f = 0;
    bool do_parse = true, do_resolve = !fold;
    if (F) {
      u32 ix;
      if (mode == 1u) {
        // P(f0) | P(f1) and R(f0) alternating | ... | R(f_last): parse and resolve tasks side by side on every CU
        if (t < n_units) { ix = t; f = 0u; do_resolve = false; }
        else {
          const u32 t1 = t - n_units, k = t1 / (2u * n_units) + 1u;
          if (k >= F) { ix = t1 - 2u * n_units * (F - 1u); f = F - 1u; do_parse = false; }
          else {
            const u32 w = t1 % (2u * n_units);
            ix = w >> 1;
            if (w & 1u) { f = k - 1u; do_parse = false; } else { f = k; do_resolve = false; }
          }
        }
      }
      else if (mode == 2u) {
        // a unit's tasks in a row: P(f0) .. P(f_last), R(f0) .. R(f_last) (a launch whose tickets all run at once: the order only
        // says which tasks share a CU)
        ix = t / (2u * F);
        const u32 w = t % (2u * F);
        if (w < F) { f = w; do_resolve = false; } else { f = w - F; do_parse = false; }
      }
      else {
        const u32 sct = t / n_units;
        ix = t % n_units;
        if (sct < F) { f = sct; do_resolve = false; } else { f = sct - F; do_parse = false; }
      }
      ui = rfl(order ? order[ix] : ix);
    }
    else {
      const u32 slot = slot_lo + t;
      ui = rfl(frame_unit[slot]);
      if (ui != 0xFFFFFFFFu) f = slot - rfl(units[ui].frame_base);
    }
    if (ui == 0xFFFFFFFFu) continue;
    const mspack_hip_unit *up = &units[ui];
    if (rfl((u32) up->kind) != MSPACK_HIP_KIND_LZX || !(rfl(up->flags) & MSPACK_HIP_UF_FRAME_TABLE)) continue;
#ifdef LZX_PIPE_TRACE
    const unsigned long long tr0 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) lzxn::g_pipe_wait[blockIdx.x & 0xFFFFu] = 0;
#endif
    if (do_parse) {
      const u32 spec = lzx_pipe_task_spec(up, f, in_arena, recs, &sh.p);
      if (lzx_pipe_task_parse(up, f, in_arena, out_arena, recs, toks, &ctl[4], pool_chunks, &sh.p, spec, stream))
        lzx_pipe_task_tail(up, f, in_arena, out_arena, recs, toks, &ctl[4], pool_chunks, &sh.p);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the resolver reuses the LDS
      if (fold) do_resolve = fold_policy == 1u && lzx_unit_runs(&recs[rfl(up->frame_base)]);    // (a unit of long runs keeps its resolve tasks)
    }
    if (do_resolve) {
      if (stream && !do_parse) lzx_pipe_task_resolve_stream(up, f, out_arena, recs, toks, &sh.r);
      else lzx_pipe_task_resolve(up, f, out_arena, recs, toks, &sh.r, do_parse);
    }
#ifdef LZX_PIPE_TRACE
    if (lane == 0 && t < (1u << 16)) {
      g_pipe_trace[4u * t] = tr0; g_pipe_trace[4u * t + 1u] = __builtin_amdgcn_s_memrealtime();
      g_pipe_trace[4u * t + 2u] = ((unsigned long long) ui << 32) | (f << 1) | (do_parse ? 0u : 1u);
      g_pipe_trace[4u * t + 3u] = lzxn::g_pipe_wait[blockIdx.x & 0xFFFFu] | ((unsigned long long) blockIdx.x << 40);
    }
#endif
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the next task reuses the LDS
  }
}

// LZX DELTA units (OAB blocks): the same decoder compiled with LZX_DELTA (17.4 KiB of LDS: 9 units per CU)
__global__ __launch_bounds__(64)
void mspack_decode_lzxd(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                        const u8 *in_arena, u8 *out_arena, mspack_hip_result *results,
                        int32_t *frame_meta)
{
  __shared__ lzxd::LzxShared sh;
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_LZX_DELTA, ui)) return;
  const mspack_hip_unit u = units[ui];
  mspack_hip_result *res = &results[ui];
  const u32 lane = threadIdx.x;
  lzxd::lzx_decode_unit(u, in_arena, out_arena, frame_meta, res, &sh);
  if (frame_meta) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    u32 produced = rfl(res->out_len);
    u32 nfr = (produced + LZX_FRAME - 1u) / LZX_FRAME;
    for (u32 f = 0; f < nfr; f++) {
      int32_t fs = (int32_t) rfl((u32) frame_meta[u.frame_base + f]);
      if (fs == 0) continue;
      u32 fsize = u.out_len - f * LZX_FRAME; if (fsize > LZX_FRAME) fsize = LZX_FRAME;
      lzxd::lzx_e8_frame(out_arena + u.out_off + (size_t) f * LZX_FRAME, fsize,
                         (int32_t)((u32) u.e8_base + f * LZX_FRAME), fs, lane);
    }
  }
}

// one parse wave per CFDATA block of the MSZIP units that carry a frame table (mszip_kernel.hpp: "Block-level parse
// parallelism")
__global__ __launch_bounds__(64)
void mspack_mszip_parse(const mspack_hip_unit *units, const u32 *order, u32 n_units, u32 slot_lo, u32 n_slots,
                        const u8 *in_arena, u8 *out_arena, const u32 *frame_unit, u32 *hdr, lzxn::LzxFrameRec *recs, uint2 *toks, u32 pool_chunks)
{
  __shared__ MszipShared sh;
  if (blockIdx.x >= n_slots) return;
  u32 slot = slot_lo + blockIdx.x;
  const u32 F = rfl(hdr[0]);
  if (F != 0u && F == rfl(hdr[1])) {
    const u32 j = blockIdx.x / F, f = blockIdx.x % F;
    if (j >= n_units) return;
    const u32 uj = rfl(order ? order[j] : j);
    slot = units[uj].frame_base + f;
  }
  const u32 ui = rfl(frame_unit[slot]);
  if (ui == 0xFFFFFFFFu) return;
  const mspack_hip_unit u = units[ui];
  RecPool rp; rp.base = toks; rp.head = &hdr[4]; rp.cap = pool_chunks;
  zip_parse_block(u, slot - u.frame_base, in_arena, out_arena, (ZipBlockRec *) &recs[slot], rp, &sh);
}

// the copies of a launch's MSZIP blocks as fold tasks (zip_fold_block; the rule is mspack_lzx_fold's: few folders of many blocks)
__global__ __launch_bounds__(FOLD_THREADS)
void mspack_mszip_fold(const mspack_hip_unit *units, u32 slot_lo, u32 n_slots, u8 *out_arena, const u32 *frame_unit, u32 *hdr,
                       lzxn::LzxFrameRec *recs, const uint2 *toks, u32 fold_policy)
{
  __shared__ FoldLds sh;
  if (!lzx_fold_on(hdr, fold_policy, n_slots, true)) return;
  for (;;) {
    FOLD_TICKET(&hdr[7])
    if (t >= n_slots) break;
    const u32 slot = slot_lo + t;
    const u32 ui = rfl(frame_unit[slot]);
    if (ui == 0xFFFFFFFFu) continue;
    const mspack_hip_unit u = units[ui];
    {
      // (a folder of long runs -- its first block says -- stays with zip_run_tokens' run fill: lzx_unit_runs above)
      const ZipBlockRec *r0 = (const ZipBlockRec *) &recs[u.frame_base];
      const u32 n0 = rfl(gld(&r0->n_tokens)), b0 = rfl(gld(&r0->total_out));
      if (fold_policy == 1u && rfl(gld(&r0->status)) == 1u && n0 >= 16u && b0 >= 96u * n0) continue;
    }
    zip_fold_block(u, slot - u.frame_base, out_arena, (ZipBlockRec *) &recs[u.frame_base], toks, &sh);
    fold_barrier();
  }
}

__global__ __launch_bounds__(64)
void mspack_decode_mszip(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                         const u8 *in_arena, u8 *out_arena, mspack_hip_result *results,
                         const lzxn::LzxFrameRec *recs, const uint2 *toks)
{
  __shared__ MszipShared sh;
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_MSZIP, ui)) return;
  const mspack_hip_unit u = units[ui];
  mszip_decode_unit(u, in_arena, out_arena, &results[ui], &sh, (const ZipBlockRec *) recs, toks);
}
static_assert(sizeof(ZipBlockRec) == sizeof(lzxn::LzxFrameRec), "MSZIP and LZX share the work scratch");

__global__ __launch_bounds__(64)
void mspack_decode_qtm(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                       const u8 *in_arena, u8 *out_arena, mspack_hip_result *results)
{
  __shared__ QtmShared sh;
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_QUANTUM, ui)) return;
  const mspack_hip_unit u = units[ui];
  if ((u.flags & MSPACK_HIP_UF_QTM_MARKS) && u.ref_len) return;          // (mspack_decode_qtm_marks' unit)
  qtm_decode_unit<false>(u, in_arena, out_arena, &results[ui], &sh);
}
// the same for the units that carry marks (MSPACK_HIP_UF_QTM_MARKS: what requests ending at the marked positions hold back) -- the
// cabinet driver's Quantum folders; launched behind mspack_decode_qtm over the same list, each kernel leaves the other's units alone
__global__ __launch_bounds__(64)
void mspack_decode_qtm_marks(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                             const u8 *in_arena, u8 *out_arena, mspack_hip_result *results)
{
  __shared__ QtmShared sh;
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_QUANTUM, ui)) return;
  const mspack_hip_unit u = units[ui];
  if (!((u.flags & MSPACK_HIP_UF_QTM_MARKS) && u.ref_len)) return;
  qtm_decode_unit<true>(u, in_arena, out_arena, &results[ui], &sh);
}

__global__ __launch_bounds__(64)
void mspack_decode_lzss(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                        const u8 *in_arena, u8 *out_arena, mspack_hip_result *results)
{
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_LZSS, ui)) return;
  const mspack_hip_unit u = units[ui];
  if (u.flags & MSPACK_HIP_UF_LZSS_RING) return;                         // (mspack_decode_lzss_ring's unit)
  lzss_decode_unit(u, in_arena, out_arena, &results[ui]);
}
// the same for the units that keep their window in LDS (MSPACK_HIP_UF_LZSS_RING, lzss_ring_kernel.hpp) -- launched beside
// mspack_decode_lzss over the same list when the batch holds such a unit; each kernel leaves the other's units alone
__global__ __launch_bounds__(64)
void mspack_decode_lzss_ring(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                             const u8 *in_arena, u8 *out_arena, mspack_hip_result *results)
{
  __shared__ LzssRingShared sh;
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_LZSS, ui)) return;
  const mspack_hip_unit u = units[ui];
  if (!(u.flags & MSPACK_HIP_UF_LZSS_RING)) return;
  lzss_ring_decode_unit(u, in_arena, out_arena, &results[ui], &sh);
}

__global__ __launch_bounds__(64)
void mspack_decode_kwaj_lzh(const mspack_hip_unit *units, const u32 *order, u32 n_units,
                            const u8 *in_arena, u8 *out_arena, mspack_hip_result *results)
{
  __shared__ LzhShared sh;
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_KWAJ_LZH, ui)) return;
  const mspack_hip_unit u = units[ui];
  kwaj_lzh_decode_unit(u, in_arena, out_arena, &results[ui], &sh);
}

// cabd_checksum (cabd.c:1462-1479) of a unit's input bytes with seed 0 -> result.in_next.  The XOR of the unit's dwords taken
// at its own (byte) alignment equals the byte-aligned window of the XORs of the ALIGNED dwords around it -- alignbyte is
// linear over XOR --, so every lane XORs aligned dwords (coalesced), and the two ends are fixed up once.
__global__ __launch_bounds__(64)
void mspack_xorsum(const mspack_hip_unit *units, const u32 *order, u32 n_units, const u8 *in_arena, mspack_hip_result *results)
{
  u32 ui;
  if (!pick_unit(units, order, n_units, MSPACK_HIP_KIND_XORSUM, ui)) return;
  const mspack_hip_unit u = units[ui];
  const u32 lane = threadIdx.x;
  const u8 *p = in_arena + u.in_off;
  const u32 nd = u.in_len >> 2, sh = (u32)((size_t) p & 3u);
  const u32 *w = (const u32 *)(p - sh);                  // aligned dwords; w[nd] exists (the arena's slack) when sh != 0
  u32 a = 0;
  for (u32 j = lane; j < nd; j += WAVE) a ^= w[j];
  for (int o = 32; o >= 1; o >>= 1) a ^= (u32) __builtin_amdgcn_ds_bpermute((int)(((lane ^ (u32) o) & 63u) << 2), (int) a);
  if (lane == 0) {
    u32 sum = a;
    if (sh && nd) {
      const u32 b = a ^ w[0] ^ w[nd];                     // the XOR of w[1 .. nd]
      sum = __builtin_amdgcn_alignbyte(b, a, sh);
    }
    const u8 *t = p + (size_t) nd * 4u;
    u32 tail = 0;
    switch (u.in_len & 3u) {
    case 3: tail |= (u32) *t++ << 16;   /* fall through */
    case 2: tail |= (u32) *t++ << 8;    /* fall through */
    case 1: tail |= *t;
    }
    mspack_hip_result r;
    r.err = ERR_OK; r.flags = 0; r.out_len = 0; r.in_used = u.in_len; r.good_len = 0; r.in_next = sum ^ tail;
    results[ui] = r;
  }
}

// MSPACK_HIP_UF_CRC32 (crc32_kernel.hpp): the digest pass over a compact list of flagged units, launched behind the codec
// kernels that wrote results[] -- stream order is the only ordering.  First the start value's share, one unit per lane ...
__global__ __launch_bounds__(64)
void mspack_crc32_init(const mspack_hip_unit *units, const u32 *order, u32 n_units, mspack_hip_result *results)
{
  const u32 j = blockIdx.x * 64u + threadIdx.x;
  if (j >= n_units) return;
  const u32 ui = order ? order[j] : j;
  const mspack_hip_unit u = units[ui];
  if (crc_unit_wanted(u)) crc_init_unit(u, &results[ui]);
}
// ... then the bytes: segs_y wavefronts per unit, wave y takes the unit's segments y, y + segs_y, ...
__global__ __launch_bounds__(64)
void mspack_crc32(const mspack_hip_unit *units, const u32 *order, u32 n_units, u32 segs_y, const u8 *out_arena, mspack_hip_result *results)
{
  __shared__ CrcShared sh;
  const u32 j = blockIdx.x / segs_y, y = blockIdx.x % segs_y;
  if (j >= n_units) return;
  const u32 ui = rfl(order ? order[j] : j);
  const mspack_hip_unit u = units[ui];
  if (!crc_unit_wanted(u)) return;
  crc_unit_segments(u, out_arena, &results[ui], y, segs_y, &sh);
}

// MSPACK_HIP_KIND_MD5 (md5_kernel.hpp): one digest unit per LANE, launched behind everything that stores into the output arena --
// stream order is the only ordering.  Lanes whose unit is of another kind leave at once.
__global__ __launch_bounds__(64)
void mspack_md5(const mspack_hip_unit *units, const u32 *order, u32 n_units, const u8 *out_arena, u64 out_bytes, mspack_hip_result *results)
{
  const u32 j = blockIdx.x * 64u + threadIdx.x;
  if (j >= n_units) return;
  const u32 ui = order ? order[j] : j;
  const mspack_hip_unit u = units[ui];
  if (u.kind != MSPACK_HIP_KIND_MD5) return;
  md5_unit(u, out_arena, out_bytes, &results[ui]);
}

// MSPACK_HIP_KIND_SHA1 / _SHA256 (sha_kernel.hpp): one head per LANE, one kernel per algorithm -- lanes of one wave never run
// different hash functions --, launched like mspack_md5 behind everything that stores into the output arena.  order[0 .. n_list)
// names the lanes' units in a table of n_table (a head's tail is units[ui + 1]); lanes whose unit is of another kind leave at once
// (a tail met here, the device-resident entry only, is checked for its head).
template <int KIND>
__device__ __forceinline__ void sha_entry(const mspack_hip_unit *units, const u32 *order, u32 n_list, u32 n_table, const u8 *out_arena, u64 out_bytes,
                                          mspack_hip_result *results)
{
  const u32 j = blockIdx.x * 64u + threadIdx.x;
  if (j >= n_list) return;
  const u32 ui = order ? order[j] : j;
  if (ui >= n_table) return;
  const mspack_hip_unit u = units[ui];
  if (u.kind == MSPACK_HIP_KIND_DIGEST_MORE) { sha_tail_unit(units, ui, results); return; }
  if (u.kind != KIND) return;
  sha_unit<KIND>(units, ui, n_table, u, out_arena, out_bytes, results);
}
__global__ __launch_bounds__(64)
void mspack_sha1(const mspack_hip_unit *units, const u32 *order, u32 n_list, u32 n_table, const u8 *out_arena, u64 out_bytes, mspack_hip_result *results)
{
  sha_entry<MSPACK_HIP_KIND_SHA1>(units, order, n_list, n_table, out_arena, out_bytes, results);
}
__global__ __launch_bounds__(64)
void mspack_sha256(const mspack_hip_unit *units, const u32 *order, u32 n_list, u32 n_table, const u8 *out_arena, u64 out_bytes, mspack_hip_result *results)
{
  sha_entry<MSPACK_HIP_KIND_SHA256>(units, order, n_list, n_table, out_arena, out_bytes, results);
}

// MSPACK_HIP_KIND_SHA384 / _SHA512 (sha512_kernel.hpp): one head per LANE, ONE kernel for both -- they share the compression function;
// a lane picks its initial state by its unit's kind --, launched like mspack_sha256.  `kinds`: bit MSPACK_HIP_KIND_SHA384 / _SHA512
// set = heads of that algorithm are taken (the device-resident entry's kind_mask; the host entry points set both)
__global__ __launch_bounds__(64)
void mspack_sha512(const mspack_hip_unit *units, const u32 *order, u32 n_list, u32 n_table, const u8 *out_arena, u64 out_bytes, mspack_hip_result *results,
                   u32 kinds)
{
  const u32 j = blockIdx.x * 64u + threadIdx.x;
  if (j >= n_list) return;
  const u32 ui = order ? order[j] : j;
  if (ui >= n_table) return;
  const mspack_hip_unit u = units[ui];
  if (u.kind == MSPACK_HIP_KIND_DIGEST_MORE) { sha_tail_unit(units, ui, results); return; }
  if ((u.kind != MSPACK_HIP_KIND_SHA384 && u.kind != MSPACK_HIP_KIND_SHA512) || !((kinds >> u.kind) & 1u)) return;
  sha512_unit(units, ui, n_table, u, out_arena, out_bytes, results);
}

// MSPACK_HIP_KIND_CRC32 (crc32_range_kernel.hpp): the CRC-32 of byte ranges of any length, launched behind everything that stores into
// the output arena -- stream order is the only ordering, between these four launches too.  order[0 .. n) names the list's units (NULL:
// the whole table); units of other kinds own nothing here.  init and finish: one position per lane; scan: one wave; the pass: a
// bounded grid of waves that take chunks of segment tickets until the counter is past the end
__global__ __launch_bounds__(64)
void mspack_crc32r_init(const mspack_hip_unit *units, const u32 *order, u32 n, u64 out_bytes, mspack_hip_result *results)
{
  crc32r_init_lane(units, order, n, out_bytes, results);
}
__global__ __launch_bounds__(64)
void mspack_crc32r_scan(const mspack_hip_unit *units, const u32 *order, u32 n, const u8 *out_arena, u64 out_bytes, mspack_hip_result *results)
{
  crc32r_scan_wave(units, order, n, out_arena, out_bytes, results);
}
__global__ __launch_bounds__(64)
void mspack_crc32r_pass(const mspack_hip_unit *units, const u32 *order, u32 n, const u8 *out_arena, u64 out_bytes, mspack_hip_result *results)
{
  __shared__ CrcShared sh;
  crc32r_pass_wave(units, order, n, out_arena, out_bytes, results, &sh);
}
__global__ __launch_bounds__(64)
void mspack_crc32r_finish(const mspack_hip_unit *units, const u32 *order, u32 n, u64 out_bytes, mspack_hip_result *results)
{
  crc32r_finish_lane(units, order, n, out_bytes, results);
}

// MSPACK_HIP_KIND_STORED (stored_kernel.hpp): a stored folder's bytes into the output arena -- the segments of all stored units of the
// list one pool of work.  order[0 .. n) names the list's units (NULL: the whole table); units of other kinds own nothing here.  Stream
// order is the only ordering between the three launches: scan: one wave; the pass: a bounded grid of waves that take chunks of segment
// tickets until the counter is past the end; results: one position per lane, last (the pass keeps its bookkeeping in result words)
__global__ __launch_bounds__(64)
void mspack_stored_scan(const mspack_hip_unit *units, const u32 *order, u32 n, u64 in_bytes, const u8 *out_arena, u64 out_bytes, mspack_hip_result *results)
{
  stored_scan_wave(units, order, n, in_bytes, out_arena, out_bytes, results);
}
__global__ __launch_bounds__(64)
void mspack_stored_pass(const mspack_hip_unit *units, const u32 *order, u32 n, const u8 *in_arena, u64 in_bytes, u8 *out_arena, u64 out_bytes,
                        mspack_hip_result *results)
{
  stored_pass_wave(units, order, n, in_arena, in_bytes, out_arena, out_bytes, results);
}
__global__ __launch_bounds__(64)
void mspack_stored_results(const mspack_hip_unit *units, const u32 *order, u32 n, u64 in_bytes, u64 out_bytes, mspack_hip_result *results)
{
  stored_result_lane(units, order, n, in_bytes, out_bytes, results);
}
