// host_pipeline.hpp -- the host-buffer path: the per-device context, the pipeline over a planned batch (plan -> buffers -> issue ->
// drain: host_plan.hpp makes the plan, CopyBack below brings the bytes home), its statistics, the host-buffer entry points, the jobs,
// the sharded entry and mspack_hip_release.
#pragma once
#include <thread>
#include <chrono>
#include <mutex>
#include <condition_variable>
#include <atomic>
// ---------------------------------------------------------------------------------------------------
// Host-buffer path: a persistent context per device (device arenas and pinned staging grown on demand,
// never freed per call; four streams) and a chunked pipeline.  The batch is cut into up to MSPACK_HIP_NCHUNKS
// chunks of units that are contiguous in the caller's arenas:
//     copy-in stream :  H2D chunk 0, H2D chunk 1, ...                      (one after the other: the link's rate)
//     two compute streams, chunk c on stream c mod 2: wait for chunk c's H2D -> one launch per codec over the
//                       chunk's compact unit lists (a launch's waves leave as its queue runs dry, the next chunk's
//                       launch -- on the other stream -- fills the slots they free: no tail between chunks)
//     copy-out stream:  wait for chunk c's launches -> D2H chunk c          (PCIe is full duplex)
// so the copy of chunk c+1 overlaps the decode of chunk c and the copy-back of chunk c the decode of chunk c+1.
// Round 6's end (profiles/round6_jobs.txt): the chunks' shares GROW to the device (1 : 1 : 2 : 4: the last chunk's launches end the call
// and should fill the chip) and begin with half a share to the host (the copy back is the long leg); a batch that is small beside the
// chip uses all compute streams either way; an LZX launch beside other chunks' launches asks for a third of its tickets' waves; and the
// whole pipeline can run on a thread of its own and hand its chunks over as they come back (JobProgress, mspack_hip_decode_batch_begin).
// (Four streams = four hardware queues: with more, two streams share a queue and a copy waits behind another
// chunk's kernel -- what profiles/round2_hostpath_streams.txt shows for its third chunk.)
// ---------------------------------------------------------------------------------------------------
// Context SLOTS (mspack_hip_set_slots): a device has up to MSPK_MAX_SLOTS such contexts, each with arenas, staging, streams and events of
// its own.  A batch takes the free slot with the lowest index below the configured count, keeps it from plan to drain and hands it
// back; with none free it waits on the pool's condition variable.  Batches in different slots share nothing but the chip: their
// copies and launches are on different streams and the runtime overlaps them.  One slot (the default) is the single context and the
// queue of batches this file always had.  A slot's streams, events and buffers come with the first batch that runs in it.
#define MSPK_MAX_DEV 16
#define MSPK_MAX_STREAMS 8
#define MSPK_MAX_SLOTS 4
struct DevBuf { void *p = nullptr; size_t cap = 0; };
struct DevCtx {
  std::mutex mu;                        // held by the batch that runs in the slot; by mspack_hip_release while it frees it
  bool busy = false;                    // (DevPool::mu) a batch has taken the slot
  bool ready = false;
  int ns = 0;
  hipStream_t st[MSPK_MAX_STREAMS];      // [0] copy-in (and everything of a one-chunk call), [1] copy-out, [2] [3] compute
  hipEvent_t ev_in[MSPK_MAX_CHUNKS], ev_done[MSPK_MAX_CHUNKS], ev_back[MSPK_MAX_CHUNKS];      // chunk c: input there / launches through / output back
  int n_compute = 2;
  DevBuf d_in, d_out, d_units, d_order, d_res, d_fm;
  DevBuf h_stage;                       // pinned: results + (optionally) the output on its way to pageable memory
};
struct DevPool {
  std::mutex mu; std::condition_variable cv;
  DevCtx slot[MSPK_MAX_SLOTS];
  int held = 0;                         // slots taken
};
static DevPool g_pool[MSPK_MAX_DEV];

// the configured number of slots per device: MSPACK_HIP_SLOTS (read once), then whatever mspack_hip_set_slots said last
static std::atomic<int> g_slots{0};
static int slots_now()
{
  int n = g_slots.load(std::memory_order_acquire);
  if (n) return n;
  static const int from_env = env_int("MSPACK_HIP_SLOTS", 1, 1, MSPK_MAX_SLOTS);
  g_slots.compare_exchange_strong(n, from_env);
  return g_slots.load(std::memory_order_acquire);
}
static std::mutex g_slot_stats_mu;
static unsigned long long g_slot_stats[3] = { 0, 0, 0 };      // batches, the most that held slots of one device at once, batches that waited

// a batch's hold on a slot of its device's pool, from plan to drain (and on every way out)
struct SlotLease {
  DevPool &pool; DevCtx *cx = nullptr;
  explicit SlotLease(DevPool &p) : pool(p) {
    bool waited = false;
    {
      std::unique_lock<std::mutex> lk(pool.mu);
      for (;;) {
        const int n = slots_now();
        for (int i = 0; i < n && !cx; i++) if (!pool.slot[i].busy) cx = &pool.slot[i];
        if (cx) break;
        waited = true;
        pool.cv.wait(lk);
      }
      cx->busy = true;
      pool.held++;
      std::lock_guard<std::mutex> sl(g_slot_stats_mu);
      g_slot_stats[0]++;
      if ((unsigned long long) pool.held > g_slot_stats[1]) g_slot_stats[1] = (unsigned long long) pool.held;
      if (waited) g_slot_stats[2]++;
    }
    cx->mu.lock();
  }
  ~SlotLease() {
    cx->mu.unlock();
    { std::lock_guard<std::mutex> lk(pool.mu); cx->busy = false; pool.held--; }
    pool.cv.notify_all();
  }
  SlotLease(const SlotLease &) = delete;
  SlotLease &operator=(const SlotLease &) = delete;
};

// a buffer of slot cx, at least `need` bytes.  What it replaces is freed behind the slot's OWN streams (hipFree itself may wait for the
// whole device: a grow may stall the neighbours, it never touches what is theirs)
static hipError_t grow(DevCtx &cx, DevBuf &b, size_t need, bool pinned) {
  if (need <= b.cap) return hipSuccess;
  hipError_t e;
  if (b.p) {
    for (int i = 0; i < cx.ns; i++) if ((e = hipStreamSynchronize(cx.st[i])) != hipSuccess) return e;
    e = pinned ? hipHostFree(b.p) : hipFree(b.p); b.p = nullptr; b.cap = 0; if (e != hipSuccess) return e;
  }
  size_t cap = need + need / 4 + 4096;
  e = pinned ? hipHostMalloc(&b.p, cap, hipHostMallocDefault) : hipMalloc(&b.p, cap);
  if (e != hipSuccess) { b.p = nullptr; return e; }
  b.cap = cap;
  return hipSuccess;
}

static void host_path_account(double plan_ms, double issue_ms, double drain_ms);
// What a job (mspack_hip_decode_batch_begin) lets its caller see of a batch that is still running: which chunk a unit went into, and
// how many chunks are through -- their bytes in the caller's output buffer, their units' results written.  Chunks finish in order.
struct JobProgress {
  std::mutex mu; std::condition_variable cv;
  bool planned = false;                 // chunk_of is filled in
  std::vector<uint32_t> chunk_of;       // the caller's unit index -> chunk
  size_t done = 0;                      // chunks complete
  bool finished = false; int rc = 0;    // the call has returned (rc); nothing is promised about chunks >= done when rc != 0
};

// the planner's knobs (host_plan.hpp) out of the environment, each read once per process
static const PlanKnobs &plan_knobs()
{
  static const PlanKnobs knobs = []() {
    PlanKnobs k;
    k.max_chunks = (size_t) env_int("MSPACK_HIP_NCHUNKS", 4, 1, MSPK_MAX_CHUNKS);
    // (a chunk: >= 8 MiB of input -- a copy of >= 150 us -- and >= 256 units)
    k.chunk_bytes = (size_t) env_int("MSPACK_HIP_CHUNK_BYTES", 8 << 20, 1, 1 << 30);
    k.chunk_units = (size_t) env_int("MSPACK_HIP_CHUNK_UNITS", 256, 1, 1 << 30);
    k.shape = getenv("MSPACK_HIP_CHUNK_SHAPE") ? env_int("MSPACK_HIP_CHUNK_SHAPE", 0, 0, 4) : -1;
    // (MSPACK_HIP_CHUNK_WEIGHTS="1,1,2,4": the shares spelled out -- sweeps)
    if (const char *q = getenv("MSPACK_HIP_CHUNK_WEIGHTS"))
      while (*q && k.weights.size() < MSPK_MAX_CHUNKS) { const long v = strtol(q, (char **) &q, 10); k.weights.push_back(v > 0 ? (uint64_t) v : 1u); while (*q == ',' || *q == ' ') q++; }
    return k;
  }();
  return knobs;
}

typedef std::chrono::steady_clock::time_point TimePt;
static inline TimePt tnow() { return std::chrono::steady_clock::now(); }
static inline double tms(TimePt a, TimePt b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static bool host_trace() { static const bool trace = getenv("MSPACK_HIP_TRACE") != nullptr; return trace; }

// One call of the pipeline: its arguments, its plan, and where its buffers and streams are.  A step that fails leaves
// "<call>: <hip error string>" in errbuf and returns -(int) the error.
struct PipeCall {
  int dev; DevCtx &cx; const BatchPlan &plan;
  const void *in; void *host_out; mspack_hip_result *results; JobProgress *pg;
  char *errbuf; size_t errcap;
  TimePt t0;                                             // the call began
  size_t in_span, out_span, stage_res;                   // stage_res: the results' part of the pinned staging buffer, the pieces behind it
  u8 *d_in, *d_out;
  mspack_hip_unit *d_units; uint32_t *d_order; mspack_hip_result *d_res, *h_res;
  bool one;                                              // one chunk: everything in order on one stream, no events
  size_t n_comp;                                         // compute streams in use
  hipStream_t st_in, st_out;
  int fail(hipError_t e, const char *what) const { snprintf(errbuf, errcap, "%s: %s", what, hipGetErrorString(e)); return -(int) e; }
};
#define TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return pc.fail(e_, #call); } while (0)

// a device's context: its streams and events, created with its first batch
static int context_setup(DevCtx &cx, const PipeCall &pc)
{
  if (cx.ready) return 0;
  cx.n_compute = env_int("MSPACK_HIP_NCOMPUTE", 4, 1, MSPK_MAX_STREAMS - 2);
  cx.ns = 2 + cx.n_compute;
  // The runtime maps a process's streams onto a few hardware queues PER PRIORITY LEVEL (four by default), and streams that
  // share a queue run one after the other -- whichever library created them: inside a process that has streams of its own
  // (bench.py: torch's) the copy-in stream landed on a compute stream's queue and every chunk's copy waited for the chunk
  // before it (to the device 8.2 ms instead of 4.7, profiles/round3_hostpath.txt).  So the three roles live on three
  // priority levels, i.e. in three queue pools: compute streams high (a pool of their own: the chunks' launches run side
  // by side), copy-in normal, copy-out low.
  int prio_lo = 0, prio_hi = 0;
  TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));           // (least, greatest): numerically high = low priority
  for (int i = 0; i < cx.ns; i++) {
    const int pr = i == 0 ? (prio_lo + prio_hi) / 2 : (i == 1 ? prio_lo : prio_hi);
    TRY(hipStreamCreateWithPriority(&cx.st[i], hipStreamNonBlocking, pr));
  }
  for (int i = 0; i < MSPK_MAX_CHUNKS; i++) {
    TRY(hipEventCreateWithFlags(&cx.ev_in[i], hipEventDisableTiming));
    TRY(hipEventCreateWithFlags(&cx.ev_done[i], hipEventDisableTiming));
    TRY(hipEventCreateWithFlags(&cx.ev_back[i], hipEventDisableTiming));
  }
  cx.ready = true;
  return 0;
}

// ---- buffers (persistent) ----
static const size_t STAGE_PIECE = 8192u, STAGE_SLOTS = 4u * MSPK_MAX_CHUNKS;
static int grow_buffers(PipeCall &pc, void *dev_out)
{
  DevCtx &cx = pc.cx;
  const size_t n_sel = pc.plan.local.size(), n_crc = pc.plan.n_crc, in_span = pc.in_span, out_span = pc.out_span;
  TRY(grow(cx, cx.d_in, in_span + 64, false));
  if (!dev_out) TRY(grow(cx, cx.d_out, out_span + 64, false));
  TRY(grow(cx, cx.d_units, n_sel * sizeof(mspack_hip_unit), false));
  TRY(grow(cx, cx.d_order, (n_sel + n_crc) * sizeof(uint32_t), false));
  TRY(grow(cx, cx.d_res, n_sel * sizeof(mspack_hip_result), false));
  TRY(grow(cx, cx.d_fm, lzx_scratch(nullptr, pc.plan.n_frames, pc.plan.n_rec_slots).bytes, false));
  // (pinned staging: the results, and room for the few output bytes that lie outside every page-locked range -- CopyBack::copy_out)
  pc.stage_res = (n_sel * sizeof(mspack_hip_result) + 255u) & ~(size_t) 255u;
  TRY(grow(cx, cx.h_stage, pc.stage_res + STAGE_PIECE * STAGE_SLOTS, true));
  pc.d_in = (u8 *) cx.d_in.p;
  pc.d_out = dev_out ? (u8 *) dev_out : (u8 *) cx.d_out.p;
  pc.d_units = (mspack_hip_unit *) cx.d_units.p;
  pc.d_order = (uint32_t *) cx.d_order.p;
  pc.d_res = (mspack_hip_result *) cx.d_res.p;
  pc.h_res = (mspack_hip_result *) cx.h_stage.p;
  return 0;
}

// The copies back are issued by a second thread.  A copy into PAGEABLE memory holds its calling thread and (measured,
// profiles/round3_hostpath.txt) does not start before every stream of the device has drained, so this thread first
// page-locks each chunk's part of the caller's buffer (hipHostRegister -- while the main thread is inside the H2D
// copies and the first launches run), after which chunk c's D2H is a plain DMA that starts the moment chunk c's
// launches have ended, next to the H2D of later chunks (PCIe is full duplex).  The pages are released before the
// call returns.  A buffer that cannot be registered (already pinned by its owner, or the runtime refuses) is
// copied the ordinary way.  Only whole pages INSIDE the bytes this call writes are locked (see PinRange, host_pins.hpp); what is
// left over at the two ends of the span (less than a page each; nothing for a page-aligned buffer such as the C
// drivers') goes through the pinned staging buffer and is copied into place at the end.
// Destruction (an error path): the thread is stopped and joined first, then the locks are given up (~Pins: behind a device
// synchronisation) -- the members' order.
struct CopyBack {
  PipeCall &pc;
  Pins pins, pins_in;
  struct Staged { void *host; size_t off, n; };
  // (written by the thread that issues the copies back; read behind it: chunk ci's pieces are staged[.. staged_upto[ci]), final once
  // back_issued says the chunk's copies are on the stream)
  Staged staged[STAGE_SLOTS];
  size_t n_staged = 0, staged_upto[MSPK_MAX_CHUNKS] = { 0 };
  double tr_locked[MSPK_MAX_CHUNKS] = { 0 }, tr_h2d[MSPK_MAX_CHUNKS] = { 0 };      // (trace: ms after the call began)
  std::atomic<size_t> issued{0};                         // chunks whose ev_done has been recorded
  std::atomic<size_t> back_issued{0};                    // chunks whose copies back are on st_out, ev_back recorded behind them
  std::atomic<bool> stop{false}, back_ended{false};
  hipError_t back_err = hipSuccess;
  double pin_ms = 0.0, unpin_ms = 0.0;
  bool pin_out = false, back_started = false;
  size_t handed = 0, staged_done = 0;                    // units / staged pieces already in the caller's memory
  std::thread back;

  explicit CopyBack(PipeCall &call) : pc(call) {}
  ~CopyBack() { if (back.joinable()) { stop.store(true); back.join(); } }

  // one span of the output, device -> caller's memory on st_out: cut at the boundaries of every registration this library
  // knows; pieces outside all of them that are small go through the pinned staging buffer (no pageable copy in the way)
  hipError_t copy_out(uintptr_t lo, uintptr_t hi, const u8 *d_src) {
    std::vector<uintptr_t> cuts;
    pin_cuts(lo, hi, pins.r.data(), pins.n, cuts);
    uintptr_t at = lo;
    for (size_t i = 0; i <= cuts.size(); i++) {
      const uintptr_t to = i < cuts.size() ? cuts[i] : hi;
      if (to <= at) continue;
      bool locked = false;
      for (int k = 0; k < pins.n && !locked; k++) locked = at >= pins.r[k].ra && to <= pins.r[k].rb;
      hipError_t ce;
      if (!locked && pins.n && to - at <= STAGE_PIECE && n_staged < STAGE_SLOTS) {
        const size_t off = pc.stage_res + STAGE_PIECE * n_staged;
        ce = hipMemcpyAsync((char *) pc.cx.h_stage.p + off, d_src + (at - lo), to - at, hipMemcpyDeviceToHost, pc.st_out);
        staged[n_staged++] = Staged{ (void *) at, off, (size_t)(to - at) };
      }
      else ce = hipMemcpyAsync((void *) at, d_src + (at - lo), to - at, hipMemcpyDeviceToHost, pc.st_out);
      if (ce != hipSuccess) return ce;
      at = to;
    }
    return hipSuccess;
  }
  // a whole chunk's span
  hipError_t copy_out_chunk(const Chunk &c) {
    return copy_out((uintptr_t) pc.host_out + c.out_lo, (uintptr_t) pc.host_out + c.out_hi, pc.d_out + (c.out_lo - pc.plan.out_lo));
  }
  // the staged pieces [staged_done, upto) into place
  void unstage(size_t upto) {
    for (; staged_done < upto; staged_done++) memcpy(staged[staged_done].host, (const char *) pc.cx.h_stage.p + staged[staged_done].off, staged[staged_done].n);
  }
  // the results of local units [a, b) into the caller's array
  void hand_over(size_t a, size_t b) {
    for (size_t i = a; i < b; i++) {
      pc.results[pc.plan.idx[i]] = pc.h_res[i];
      if (pc.plan.local[i].kind == 0) { memset(&pc.results[pc.plan.idx[i]], 0, sizeof(mspack_hip_result)); pc.results[pc.plan.idx[i]].err = ERR_ARGS; }
    }
  }
  void thread_body();
  void start();
};

// the helper thread: chunk by chunk, lock the chunk's pages, wait until its launches are on their stream, queue its copies behind them
void CopyBack::thread_body()
{
  const std::vector<Chunk> &chunks = pc.plan.chunks;
  hipError_t be = hipSetDevice(pc.dev);
  const uintptr_t base = (uintptr_t) pc.host_out;
  uintptr_t span_a, span_b;                            // the whole pages inside the bytes this call writes
  const bool any = inner_pages((const void *)(base + pc.plan.out_lo), pc.out_span, span_a, span_b);
  for (size_t ci = 0; ci < chunks.size() && be == hipSuccess; ci++) {
    const Chunk &c = chunks[ci];
    // chunk ci's pages: from the first page boundary at or behind its first byte to the first one at or behind its
    // end (the last chunk: the last one inside the span) -- disjoint from its neighbours' ranges
    uintptr_t ra = (base + c.out_lo + MSPK_PAGE - 1u) & ~(MSPK_PAGE - 1u), rb = (base + c.out_hi + MSPK_PAGE - 1u) & ~(MSPK_PAGE - 1u);
    if (ra < span_a) ra = span_a;
    if (rb > span_b || ci + 1 == chunks.size()) rb = span_b;
    auto r0 = tnow();
    if (pin_out && any) pins.lock(ra, rb);
    pin_ms += tms(r0, tnow());
    tr_locked[ci] = tms(pc.t0, tnow());
    while (issued.load(std::memory_order_acquire) <= ci) { if (stop.load(std::memory_order_relaxed)) return; std::this_thread::yield(); }
    be = hipStreamWaitEvent(pc.st_out, pc.cx.ev_done[ci], 0);
    if (be == hipSuccess) be = copy_out_chunk(c);
    if (be == hipSuccess && (pc.pg || host_trace())) be = hipEventRecord(pc.cx.ev_back[ci], pc.st_out);
    if (be == hipSuccess) { staged_upto[ci] = n_staged; back_issued.store(ci + 1, std::memory_order_release); }
  }
  back_err = be;
  back_ended.store(true, std::memory_order_release);
}

// whether the output gets locked, and the thread (several chunks to the host)
void CopyBack::start()
{
  const std::vector<mspack_hip_unit> &local = pc.plan.local;
  // (LZX DELTA units read their reference data out of the caller's output buffer while this call runs: no locking of it then)
  bool refs_in_out = false;
  for (size_t i = 0; i < local.size() && !refs_in_out; i++) refs_in_out = local[i].kind == MSPACK_HIP_KIND_LZX_DELTA && local[i].ref_len != 0u;
  static const bool pin_out_env = env_int("MSPACK_HIP_PIN_OUT", 1, 0, 1) != 0;
  // (a buffer that is page-locked already -- the drivers' arenas out of mspack_hip_stage_alloc, a caller's hipHostMalloc -- needs
  // no lock, and ASKING for one is not free: the runtime walks the pages before it notices: ~3 ms per 64 MB chunk, on the
  // copy-back's critical path.  Pins::lock_one asks the runtime whose memory a range is before it asks for the lock, per range)
  pin_out = pin_out_env && !refs_in_out;
  if (pc.host_out && !pc.one) try {
    back = std::thread([this]() { thread_body(); });
    back_started = true;
  } catch (...) { back_started = false; }      // (no helper thread: the copies back are issued by copy_back_inline, in the caller's thread)
}

// ---- issue: tables, then every chunk's copy on the copy-in stream and its launches on a compute stream ----
static int issue_chunks(PipeCall &pc, CopyBack &cb)
{
  DevCtx &cx = pc.cx;
  const BatchPlan &plan = pc.plan;
  const std::vector<mspack_hip_unit> &local = plan.local;
  const size_t n_sel = local.size();
  const bool one = pc.one = plan.chunks.size() == 1;
  // compute streams in use: all of them when the output stays on the device (the chunks' launches side by side: the
  // last one ends earliest), two when it goes back to the host (the chunks then finish one after the other and the
  // copy-back, the longest leg, starts early) -- measured, profiles/round3_hostpath.txt
  // (A Quantum unit is one long serial chain: a launch of them takes as long as its slowest folder however few there are.
  // Chunks that hold some must not queue behind each other on one compute stream: all streams then, also to the host --
  // with 16 384 checksum units beside 512 folders config 4 was cut into four chunks on two streams: 794 ms instead of 416)
  // (... unless the whole batch is small beside the chip -- config 3's 1024 intervals are 4096 tickets for 4096 waves: its four
  // chunks' launches then fit side by side, and on two streams the second pair only waited: to the host 4.2 -> 3.3 ms,
  // tools/sessions/round6_sessions.md: session AB; the headline batch on four streams: slower, as it was)
  static const int ncomp_host = env_int("MSPACK_HIP_NCOMP_HOST", 0, 0, MSPK_MAX_STREAMS - 2);
  const size_t few = (ncomp_host > 0) ? (size_t) ncomp_host : (plan.n_frames <= 6144u ? (size_t) cx.n_compute : 2u);
  const size_t n_comp = pc.n_comp = (pc.host_out && !plan.has_qtm) ? std::min<size_t>(few, (size_t) cx.n_compute) : (size_t) cx.n_compute;
  hipStream_t st_in = pc.st_in = cx.st[0];
  pc.st_out = one ? cx.st[0] : cx.st[1];
  u8 *const d_in = pc.d_in, *const d_out = pc.d_out;
  TRY(hipMemcpyAsync(pc.d_units, local.data(), n_sel * sizeof(mspack_hip_unit), hipMemcpyHostToDevice, st_in));
  TRY(hipMemcpyAsync(pc.d_order, plan.order.data(), (n_sel + plan.n_crc) * sizeof(uint32_t), hipMemcpyHostToDevice, st_in));
  TRY(hipMemsetAsync(cx.d_fm.p, 0, (plan.n_frames + 1) * sizeof(int32_t), st_in));
  TRY(hipMemsetAsync(d_in + pc.in_span, 0, 64, st_in));
  cb.start();
  // The INPUT is not locked here by default (MSPACK_HIP_PIN_IN=1 does it, one range per call): for a caller's warm buffer the
  // runtime's pageable path is as fast as the lock costs (to the host 7.4 -> 8.1 ms on the headline batch); for an arena that was
  // just written -- the C drivers' gather -- it runs at 5-6 GB/s, and those callers lock their arena themselves (mspack_hip_pin).
  static const bool pin_in = env_int("MSPACK_HIP_PIN_IN", 0, 0, 1) != 0;
  if (pin_in && slots_now() == 1 && pc.in_span >= ((size_t) 4 << 20)) {
    // (one slot only: beside another batch that reads the same input the copies of the two could not be cut at each other's locks)
  // (ONE range, the whole pages inside what the copies below read: the chunks' input ranges may overlap -- frame tables
    // behind the streams)
    uintptr_t ra, rb;
    if (inner_pages((const char *) pc.in + plan.in_lo, pc.in_span, ra, rb)) cb.pins_in.lock(ra, rb);
  }
  // (what the copies so far have brought: ONE interval -- the chunks' input ranges ascend and may overlap: a CHM's intervals all
  // read "to the end of the file", chmd.c:1146-1149, so its first chunk's range is the whole arena and the later chunks' ranges
  // lie inside it; the copies run one after the other on st_in, and a chunk's launches wait for the event behind ITS copy)
  uint64_t cov_lo = 0, cov_hi = 0;
  for (size_t ci = 0; ci < plan.chunks.size(); ci++) {
    const Chunk &c = plan.chunks[ci];
    hipStream_t st = one ? cx.st[0] : cx.st[2 + ci % n_comp];
    {
      uint64_t lo = c.in_lo, hi = c.in_hi;
      if (cov_hi > cov_lo && lo >= cov_lo && lo <= cov_hi) { lo = std::min(hi, cov_hi); cov_hi = std::max(cov_hi, hi); }
      else { cov_lo = lo; cov_hi = hi; }
      TRY(copy_cut(d_in + (lo - plan.in_lo), (const char *) pc.in + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, st_in,
                   cb.pins_in.r.data(), cb.pins_in.n));
    }
    if (pc.host_out)
      for (size_t i = c.a; i < c.b; i++)               // LZX DELTA reference data sits below the unit's output
        if (local[i].ref_len && local[i].kind == MSPACK_HIP_KIND_LZX_DELTA)
          TRY(copy_cut(d_out + local[i].out_off - local[i].ref_len,
                       (const char *) pc.host_out + plan.out_lo + local[i].out_off - local[i].ref_len, local[i].ref_len,
                       hipMemcpyHostToDevice, st_in));
    cb.tr_h2d[ci] = tms(pc.t0, tnow());
    if (!one) { TRY(hipEventRecord(cx.ev_in[ci], st_in)); TRY(hipStreamWaitEvent(st, cx.ev_in[ci], 0)); }
    for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++)
      TRY(launch_kind(k, pc.d_units, pc.d_order + c.order_off[k], c.order_n[k], d_in, d_out, pc.d_res, cx.d_fm.p, plan.n_frames, c.fm_lo, c.fm_n, st,
                      c.has_ftab, (unsigned) ci, plan.n_rec_slots, one, c.has_lzss_ring));
    // (the stored units' copy: offsets are relative to the spans, the spans are what the device holds of the arenas)
    TRY(launch_stored(pc.d_units, pc.d_order + c.order_off[MSPACK_HIP_KIND_STORED], c.order_n[MSPACK_HIP_KIND_STORED], d_in, pc.in_span, d_out, pc.out_span, pc.d_res, st));
    if (c.crc_n) TRY(launch_crc32(pc.d_units, pc.d_order + c.crc_off, c.crc_n, c.crc_max, d_out, pc.d_res, st));      // behind every codec's store of its results
    if (plan.n_dig && ci + 1 == plan.chunks.size()) {
      // the digest units' passes, one per algorithm: once, on the last chunk's stream, behind every chunk's launches -- the bytes
      // they read are all stored.  The results that go back are the heads' and the tails'
      const size_t m0 = n_sel - plan.n_dig;
      if (!one) for (size_t cj = 0; cj < ci; cj++) TRY(hipStreamWaitEvent(st, cx.ev_done[cj], 0));
      TRY(launch_md5(pc.d_units, pc.d_order + plan.md5_off, plan.n_md5, d_out, pc.out_span, pc.d_res, st));
      TRY(launch_sha1(pc.d_units, pc.d_order + plan.sha1_off, plan.n_sha1, n_sel, d_out, pc.out_span, pc.d_res, st));
      TRY(launch_sha256(pc.d_units, pc.d_order + plan.sha256_off, plan.n_sha256, n_sel, d_out, pc.out_span, pc.d_res, st));
      TRY(launch_sha512(pc.d_units, pc.d_order + plan.sha512_off, plan.n_sha512, n_sel, d_out, pc.out_span, pc.d_res, SHA512_KINDS, st));
      TRY(launch_crc32_ranges(pc.d_units, pc.d_order + plan.crc32r_off, plan.n_crc32r, d_out, pc.out_span, pc.d_res, st));
      TRY(hipMemcpyAsync(pc.h_res + m0, pc.d_res + m0, plan.n_dig * sizeof(mspack_hip_result), hipMemcpyDeviceToHost, st));
    }
    TRY(hipMemcpyAsync(pc.h_res + c.a, pc.d_res + c.a, (c.b - c.a) * sizeof(mspack_hip_result), hipMemcpyDeviceToHost, st));
    if (!one) { TRY(hipEventRecord(cx.ev_done[ci], st)); cb.issued.store(ci + 1, std::memory_order_release); }
  }
  return 0;
}

// ---- copy-back of a one-chunk call, on its one stream: the span, or unit by unit where the outputs interleave ----
static int copy_back_one(PipeCall &pc, CopyBack &cb)
{
  const BatchPlan &plan = pc.plan;
  const std::vector<mspack_hip_unit> &local = plan.local;
  const Chunk &c = plan.chunks[0];
  if (plan.monotone) { TRY(cb.copy_out_chunk(c)); return 0; }
  for (size_t i = c.a; i < c.b; i++) {
    const size_t nb = (size_t) local[i].out_len + ((local[i].flags & (MSPACK_HIP_UF_MSZIP_LOG | MSPACK_HIP_UF_LZX_LOG | MSPACK_HIP_UF_QTM_MARKS)) ? (size_t) unit_above(local[i]) : 0u);   // (a unit's log lies behind its slack)
    const uintptr_t lo = (uintptr_t) pc.host_out + plan.out_lo + local[i].out_off;
    TRY(cb.copy_out(lo, lo + nb, pc.d_out + local[i].out_off));
  }
  return 0;
}
// (the helper thread could not be created: plain copies, chunk by chunk, behind each chunk's launches)
static int copy_back_inline(PipeCall &pc, CopyBack &cb)
{
  for (size_t ci = 0; ci < pc.plan.chunks.size(); ci++) {
    TRY(hipStreamWaitEvent(pc.st_out, pc.cx.ev_done[ci], 0));
    TRY(cb.copy_out_chunk(pc.plan.chunks[ci]));
  }
  return 0;
}
// a job: chunk by chunk as the copies back end -- the caller (mspack_hip_job_wait_unit) takes a chunk's bytes while the later
// chunks are still being decoded and copied
static int hand_over_chunks(PipeCall &pc, CopyBack &cb)
{
  const std::vector<Chunk> &chunks = pc.plan.chunks;
  DevCtx &cx = pc.cx;
  JobProgress *const pg = pc.pg;
  const bool trace = host_trace();
  for (size_t ci = 0; ci < chunks.size(); ci++) {
    while (cb.back_issued.load(std::memory_order_acquire) <= ci && !cb.back_ended.load(std::memory_order_acquire)) std::this_thread::yield();
    if (cb.back_issued.load(std::memory_order_acquire) <= ci) break;          // (the thread gave up: its error is reported by drain)
    double tr_done = 0.0;
    if (trace) { TRY(hipEventSynchronize(cx.ev_done[ci])); tr_done = tms(pc.t0, tnow()); }
    TRY(hipEventSynchronize(cx.ev_back[ci]));            // chunk ci's launches, its results' copy and its bytes' copies are through
    cb.unstage(cb.staged_upto[ci]);
    cb.hand_over(chunks[ci].a, chunks[ci].b);
    cb.handed = chunks[ci].b;
    if (trace) fprintf(stderr, "mspack_hip[dev %d]: chunk %zu of %zu (%zu units, %.1f MB out): input copied %.2f, output pages seen to %.2f, launches through %.2f, "
                       "handed over %.2f ms after the call began\n", pc.dev, ci, chunks.size(),
                       chunks[ci].b - chunks[ci].a, (chunks[ci].out_hi - chunks[ci].out_lo) / 1e6, cb.tr_h2d[ci], cb.tr_locked[ci], tr_done, tms(pc.t0, tnow()));
    if (pg) {
      { std::lock_guard<std::mutex> lk(pg->mu); pg->done = ci + 1; }
      pg->cv.notify_all();
    }
  }
  return 0;
}
// ---- drain: copy-back, chunk by chunk on the copy-out stream (each copy waits for its own chunk's launches only); the thread's
// end, every stream's; what was staged into place, the locks given up, the results handed over ----
static int drain(PipeCall &pc, CopyBack &cb)
{
  int rc = 0;
  if (pc.host_out && pc.one && (rc = copy_back_one(pc, cb)) != 0) return rc;
  if (pc.host_out && !pc.one && !cb.back_started && (rc = copy_back_inline(pc, cb)) != 0) return rc;
  if ((pc.pg || host_trace()) && cb.back_started && (rc = hand_over_chunks(pc, cb)) != 0) return rc;
  if (cb.back.joinable()) {
    cb.back.join();
    const hipError_t back_err = cb.back_err;
    if (back_err != hipSuccess) TRY(back_err);
  }
  for (int i = 0; i < pc.cx.ns; i++) TRY(hipStreamSynchronize(pc.cx.st[i]));
  cb.unstage(cb.n_staged);
  { auto r0 = tnow(); cb.pins.release(); cb.pins_in.release(); cb.unpin_ms = tms(r0, tnow()); }
  cb.hand_over(cb.handed, pc.plan.local.size());
  return 0;
}

// buffers -> issue -> drain of a planned batch.  (The copy-back's state ends with this function: on an error its thread is joined
// and its locks are given up before the caller waits for the streams.)
static int run_plan(PipeCall &pc, void *dev_out)
{
  int rc = grow_buffers(pc, dev_out);
  if (rc) return rc;
  const TimePt t1 = tnow();
  CopyBack cb(pc);
  if ((rc = issue_chunks(pc, cb)) != 0) return rc;
  const TimePt t2 = tnow();
  if ((rc = drain(pc, cb)) != 0) return rc;
  const TimePt t3 = tnow();
  host_path_account(tms(pc.t0, t1), tms(t1, t2), tms(t2, t3));
  if (host_trace())
    fprintf(stderr, "mspack_hip[dev %d]: %zu units in %zu chunks (%d streams): plan+alloc %.2f ms, issue (H2D %.1f MB) %.2f ms, "
            "drain (D2H %.1f MB) %.2f ms (page-locking %.2f ms beside the issue, release %.2f ms)\n", pc.dev, pc.plan.local.size(), pc.plan.chunks.size(), pc.cx.ns,
            tms(pc.t0, t1), pc.in_span / 1e6, tms(t1, t2), pc.host_out ? pc.out_span / 1e6 : 0.0, tms(t2, t3), cb.pin_ms, cb.unpin_ms);
  return 0;
}
#undef TRY

// `sel` lists the unit indices this device handles (NULL = all n_sel units).  host_out != NULL: outputs are
// copied back into it; dev_out != NULL: the caller's DEVICE buffer receives them (out_off relative to it).
// per_unit_back: copy the outputs back unit by unit (a sharded call whose shards' output spans interleave)
// plan -> buffers -> issue -> drain, in one slot of the device's pool from the first step to the last.
static int pipeline_on_current_device(int dev, mspack_hip_unit *units, const uint32_t *sel, size_t n_sel,
                                      const void *in, size_t in_bytes, void *host_out, void *dev_out,
                                      size_t out_bytes, mspack_hip_result *results, char *errbuf, size_t errcap,
                                      bool per_unit_back = false, JobProgress *pg = nullptr)
{
  if (n_sel == 0) return 0;
  if (dev < 0 || dev >= MSPK_MAX_DEV) { snprintf(errbuf, errcap, "device index %d out of range", dev); return -1; }
  SlotLease lease(g_pool[dev]);
  DevCtx &cx = *lease.cx;
  BatchPlan plan;
  PipeCall pc{ dev, cx, plan, in, host_out, results, pg, errbuf, errcap, tnow() };
  // (a batch the planner rejects has touched nothing: no context, no stream to wait for)
  if (plan_batch(units, sel, n_sel, in_bytes, out_bytes, host_out != nullptr, dev_out != nullptr, per_unit_back, plan_knobs(), plan, errbuf, errcap))
    return -1;
  pc.in_span = (size_t)(plan.in_hi - plan.in_lo); pc.out_span = (size_t)(plan.out_hi - plan.out_lo);
  int rc = context_setup(cx, pc);
  if (!rc) {
    if (pg) {
      std::lock_guard<std::mutex> lk(pg->mu);
      for (size_t ci = 0; ci < plan.chunks.size(); ci++) for (size_t i = plan.chunks[ci].a; i < plan.chunks[ci].b; i++) pg->chunk_of[plan.idx[i]] = (uint32_t) ci;
      for (size_t i = plan.local.size() - plan.n_dig; i < plan.local.size(); i++) pg->chunk_of[plan.idx[i]] = (uint32_t) plan.chunks.size();      // (digest units and tails: when the batch is through)
      pg->planned = true;
      pg->cv.notify_all();
    }
    rc = run_plan(pc, dev_out);
  }
  if (rc) for (int i = 0; i < cx.ns; i++) hipStreamSynchronize(cx.st[i]);
  return rc;
}

static int current_device() { int d = 0; if (hipGetDevice(&d) != hipSuccess) d = 0; return d; }

static std::mutex g_stats_mu;
static double g_stats_ms[4] = { 0, 0, 0, 0 };
static void host_path_account(double plan_ms, double issue_ms, double drain_ms) {
  std::lock_guard<std::mutex> lock(g_stats_mu);
  g_stats_ms[0] += plan_ms; g_stats_ms[1] += issue_ms; g_stats_ms[2] += drain_ms; g_stats_ms[3] += 1.0;
}

extern "C" {

int mspack_hip_decode_batch(mspack_hip_unit *units, size_t n_units, const void *in, size_t in_bytes,
                            void *out, size_t out_bytes, mspack_hip_result *results)
{
  return pipeline_on_current_device(current_device(), units, nullptr, n_units, in, in_bytes, out, nullptr, out_bytes,
                                    results, g_err, sizeof(g_err));
}

int mspack_hip_decode_batch_to_device(mspack_hip_unit *units, size_t n_units, const void *in, size_t in_bytes,
                                      void *d_out, size_t out_bytes, mspack_hip_result *results)
{
  return pipeline_on_current_device(current_device(), units, nullptr, n_units, in, in_bytes, nullptr, d_out, out_bytes,
                                    results, g_err, sizeof(g_err));
}

// ---- jobs: the same batch, handed over chunk by chunk while it runs (include/mspack_hip.h) ----
struct mspack_hip_job {
  std::thread th;
  JobProgress pg;
  char err[256];
};

mspack_hip_job *mspack_hip_decode_batch_begin(mspack_hip_unit *units, size_t n_units, const void *in, size_t in_bytes,
                                              void *out, size_t out_bytes, mspack_hip_result *results)
{
  static const bool off = env_int("MSPACK_HIP_JOBS", 1, 0, 1) == 0;          // (A/B runs: every caller takes its synchronous way)
  if (off || !units || !results || !out) return nullptr;
  mspack_hip_job *job = nullptr;
  try {
    job = new mspack_hip_job();
    job->err[0] = 0;
    job->pg.chunk_of.assign(n_units, 0u);
    const int dev = current_device();
    job->th = std::thread([=]() {
      int rc;
      if (hipSetDevice(dev) != hipSuccess) { (void) hipGetLastError(); snprintf(job->err, sizeof(job->err), "hipSetDevice(%d) failed", dev); rc = -1; }
      else rc = pipeline_on_current_device(dev, units, nullptr, n_units, in, in_bytes, out, nullptr, out_bytes, results,
                                           job->err, sizeof(job->err), false, &job->pg);
      { std::lock_guard<std::mutex> lk(job->pg.mu); job->pg.rc = rc; job->pg.finished = true; }
      job->pg.cv.notify_all();
    });
  } catch (...) { delete job; return nullptr; }            // (no thread, no memory: the caller takes the synchronous call)
  return job;
}

int mspack_hip_job_wait_unit(mspack_hip_job *job, size_t i)
{
  if (!job) return -1;
  JobProgress &pg = job->pg;
  std::unique_lock<std::mutex> lk(pg.mu);
  if (i >= pg.chunk_of.size()) return -1;
  pg.cv.wait(lk, [&]() { return pg.finished || (pg.planned && pg.done > pg.chunk_of[i]); });
  if (pg.planned && pg.done > pg.chunk_of[i]) return 0;    // (its chunk came through, whatever became of the later ones)
  if (pg.rc) { snprintf(g_err, sizeof(g_err), "%s", job->err); return pg.rc; }
  return 0;                                                // finished without an error: everything is there
}

int mspack_hip_job_end(mspack_hip_job *job)
{
  if (!job) return -1;
  if (job->th.joinable()) job->th.join();
  const int rc = job->pg.rc;
  if (rc) snprintf(g_err, sizeof(g_err), "%s", job->err);
  delete job;
  return rc;
}

int mspack_hip_decode_batch_multi(mspack_hip_unit *units, size_t n_units, const void *in,
                                  size_t in_bytes, void *out, size_t out_bytes,
                                  mspack_hip_result *results, int n_devices)
{
  int have = mspack_hip_device_count();
  if (n_devices > have) n_devices = have;
  if (n_devices > MSPK_MAX_DEV) n_devices = MSPK_MAX_DEV;
  const bool force_shards = getenv("MSPACK_HIP_FORCE_SHARDS") != nullptr;   // tests: exercise the sharded path on one GPU
  int n_shards = n_devices;
  if (force_shards) n_shards = env_int("MSPACK_HIP_FORCE_SHARDS", 2, 1, MSPK_MAX_DEV);
  if (n_shards <= 1 || n_units < 2) return mspack_hip_decode_batch(units, n_units, in, in_bytes, out, out_bytes, results);
  if (n_devices < 1) { snprintf(g_err, sizeof(g_err), "no HIP device"); return -1; }
  // static sharding, no inter-device traffic: plan_shards (host_plan.hpp)
  std::vector<std::vector<uint32_t>> shard;
  bool ascending = true;
  if (!plan_shards(units, n_units, n_shards, shard, ascending)) return mspack_hip_decode_batch(units, n_units, in, in_bytes, out, out_bytes, results);
  std::vector<int> rcs(n_shards, 0);
  std::vector<std::array<char, 256>> errs(n_shards);
  std::vector<std::thread> th;
  auto run_shard = [&](int sh) {
    const int dv = sh % n_devices;
    errs[sh][0] = 0;
    hipError_t e = hipSetDevice(dv);
    if (e != hipSuccess) { snprintf(errs[sh].data(), 256, "hipSetDevice(%d): %s", dv, hipGetErrorString(e)); rcs[sh] = -(int) e; return; }
    rcs[sh] = pipeline_on_current_device(dv, units, shard[sh].data(), shard[sh].size(), in, in_bytes, out, nullptr,
                                         out_bytes, results, errs[sh].data(), 256, !ascending);
  };
  th.reserve((size_t) n_shards);
  for (int sh = 0; sh < n_shards; sh++) {
    // (a thread that cannot be created must not throw through the C ABI: that shard runs here, after the others were started)
    try { th.emplace_back(run_shard, sh); } catch (...) { run_shard(sh); }
  }
  for (auto &t : th) t.join();
  for (int sh = 0; sh < n_shards; sh++)
    if (rcs[sh]) { snprintf(g_err, sizeof(g_err), "shard %d: %s", sh, errs[sh].data()); return rcs[sh]; }
  return 0;
}

void mspack_hip_host_path_stats(double *ms4, int reset)
{
  std::lock_guard<std::mutex> lock(g_stats_mu);
  if (ms4) for (int i = 0; i < 4; i++) ms4[i] = g_stats_ms[i];
  if (reset) for (int i = 0; i < 4; i++) g_stats_ms[i] = 0.0;
}

int mspack_hip_set_slots(int n)
{
  if (n < 1 || n > MSPK_MAX_SLOTS) return -1;
  g_slots.store(n, std::memory_order_release);
  // (a batch that waits for a slot looks again)
  for (int d = 0; d < MSPK_MAX_DEV; d++) { { std::lock_guard<std::mutex> lk(g_pool[d].mu); } g_pool[d].cv.notify_all(); }
  return 0;
}
int mspack_hip_slots(void) { return slots_now(); }
void mspack_hip_slot_stats(unsigned long long s[3], int reset)
{
  std::lock_guard<std::mutex> lock(g_slot_stats_mu);
  if (s) for (int i = 0; i < 3; i++) s[i] = g_slot_stats[i];
  if (reset) for (int i = 0; i < 3; i++) g_slot_stats[i] = 0;
}

// free every persistent context (device arenas, pinned staging, streams) of this process: device by device, the pool's lock (no
// batch takes a slot meanwhile), then every slot's (the batches that hold one have handed it back), then the slots' resources
void mspack_hip_release(void)
{
  int keep = current_device();
  stage_release_idle();
  for (int d = 0; d < MSPK_MAX_DEV; d++) {
    DevPool &pool = g_pool[d];
    std::lock_guard<std::mutex> pl(pool.mu);
    std::unique_lock<std::mutex> sl[MSPK_MAX_SLOTS];
    bool any = false;
    for (int k = 0; k < MSPK_MAX_SLOTS; k++) {
      sl[k] = std::unique_lock<std::mutex>(pool.slot[k].mu);
      any = any || pool.slot[k].ready || pool.slot[k].d_in.p || pool.slot[k].h_stage.p;
    }
    if (!any) continue;
    if (hipSetDevice(d) != hipSuccess) continue;
    hipDeviceSynchronize();
    for (int k = 0; k < MSPK_MAX_SLOTS; k++) {
      DevCtx &cx = pool.slot[k];
      if (!cx.ready && !cx.d_in.p && !cx.h_stage.p) continue;
      for (DevBuf *b : { &cx.d_in, &cx.d_out, &cx.d_units, &cx.d_order, &cx.d_res, &cx.d_fm }) { if (b->p) hipFree(b->p); b->p = nullptr; b->cap = 0; }
      if (cx.h_stage.p) { hipHostFree(cx.h_stage.p); cx.h_stage.p = nullptr; cx.h_stage.cap = 0; }
      if (cx.ready) {
        for (int i = 0; i < cx.ns; i++) hipStreamDestroy(cx.st[i]);
        for (int i = 0; i < MSPK_MAX_CHUNKS; i++) { hipEventDestroy(cx.ev_in[i]); hipEventDestroy(cx.ev_done[i]); hipEventDestroy(cx.ev_back[i]); }
      }
      cx.ready = false; cx.ns = 0;
    }
  }
  hipSetDevice(keep);
}

} // extern "C"
