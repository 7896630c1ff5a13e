// host_pins.hpp -- page-locked host memory: the registry of the ranges this library locked for its callers (mspack_hip_pin /
// _unpin), the copies cut at their boundaries (pin_cuts, copy_cut), and the locks one call of the host-buffer pipeline takes (Pins).
#pragma once
#include <mutex>
#include <vector>
#include <algorithm>
// ---- page-locked host ranges and the copies that touch them ---------------------------------------------------------
// ROOT CAUSE of round 4's intermittent "GPU batch decode failed ... invalid argument" (DESIGN.md sec. 8h):
// the runtime treats EVERY host address inside a registered range as that registration's memory, and a copy whose host
// side starts inside a registration and ends beyond it is refused with hipErrorInvalidValue.  Rounds 3-4 rounded their
// registrations OUTWARD to whole pages, so the first and last page also held whatever the allocator had put next to the
// caller's buffer -- e.g. this file's own std::vector<> of launch orders, 4 KiB that began in the arena's last page and
// ended behind it (glibc serves a 24 MiB arena from the brk heap once an mmap'd block of that size has been freed: the
// SECOND decompressor of a process).  Rules since:
//   (1) a registration never holds a byte outside the range its owner passed (whole pages INSIDE it);
//   (2) every copy between the device and host memory is cut at the boundaries of the registrations this library made
//       (mspack_hip_pin's registry + the call's own), so that no piece straddles one.
struct PinRange { uintptr_t ra, rb; const void *user; };
static std::mutex g_pin_mu;
static std::vector<PinRange> g_pins;
static const uintptr_t MSPK_PAGE = 4096u;
static inline bool inner_pages(const void *p, size_t bytes, uintptr_t &ra, uintptr_t &rb) {
  ra = ((uintptr_t) p + MSPK_PAGE - 1u) & ~(MSPK_PAGE - 1u);
  rb = ((uintptr_t) p + bytes) & ~(MSPK_PAGE - 1u);
  return rb > ra;
}
// the boundaries of known registrations strictly inside (lo, hi), ascending
static void pin_cuts(uintptr_t lo, uintptr_t hi, const PinRange *extra, int n_extra, std::vector<uintptr_t> &cuts) {
  cuts.clear();
  auto add = [&](const PinRange &r) { if (r.ra > lo && r.ra < hi) cuts.push_back(r.ra); if (r.rb > lo && r.rb < hi) cuts.push_back(r.rb); };
  { std::lock_guard<std::mutex> lock(g_pin_mu); for (const PinRange &r : g_pins) add(r); }
  for (int i = 0; i < n_extra; i++) add(extra[i]);
  std::sort(cuts.begin(), cuts.end());
}
// hipMemcpyAsync with the HOST side cut at registration boundaries
static hipError_t copy_cut(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t st,
                           const PinRange *extra = nullptr, int n_extra = 0) {
  if (!n) return hipSuccess;
  const uintptr_t h = kind == hipMemcpyHostToDevice ? (uintptr_t) src : (uintptr_t) dst;
  std::vector<uintptr_t> cuts;
  pin_cuts(h, h + n, extra, n_extra, cuts);
  uintptr_t at = h;
  for (size_t i = 0; i <= cuts.size(); i++) {
    const uintptr_t to = i < cuts.size() ? cuts[i] : h + n;
    if (to <= at) continue;
    const hipError_t e = hipMemcpyAsync((char *) dst + (at - h), (const char *) src + (at - h), to - at, kind, st);
    if (e != hipSuccess) return e;
    at = to;
  }
  return hipSuccess;
}

// a call's own locks on the caller's buffers (the host-buffer pipeline's: CopyBack, host_pipeline.hpp)
struct Pins {                                          // page-locked ranges of the caller's buffers (this call's own)
  std::vector<PinRange> r; int n = 0;
  bool lock_one(uintptr_t ra, uintptr_t rb) {
    if (rb <= ra) return false;
    // (someone else's registration -- the caller's own hipHostRegister / hipHostMalloc -- is left alone: asking the runtime
    // to register bytes it has registered already fails after it has walked the pages, and is not this library's to undo)
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, (const void *) ra) == hipSuccess) { if (at.type == hipMemoryTypeHost) return false; }
    else (void) hipGetLastError();
    if (hipHostRegister((void *) ra, rb - ra, hipHostRegisterDefault) != hipSuccess) { (void) hipGetLastError(); return false; }
    r.push_back(PinRange{ ra, rb, nullptr }); n = (int) r.size();
    return true;
  }
  // [ra, rb) minus every range of mspack_hip_pin's registry: the library never asks the runtime to register a byte that
  // lies inside a registration it knows about
  bool lock(uintptr_t ra, uintptr_t rb) {
    if (rb <= ra) return false;
    std::vector<PinRange> known;
    { std::lock_guard<std::mutex> lock(g_pin_mu); for (const PinRange &k : g_pins) if (k.rb > ra && k.ra < rb) known.push_back(k); }
    std::sort(known.begin(), known.end(), [](const PinRange &x, const PinRange &y) { return x.ra < y.ra; });
    bool any = false;
    uintptr_t at = ra;
    for (const PinRange &k : known) {
      if (k.ra > at) any = lock_one(at, k.ra) || any;
      if (k.rb > at) at = k.rb;
    }
    if (at < rb) any = lock_one(at, rb) || any;
    return any;
  }
  void release() { for (const PinRange &x : r) if (hipHostUnregister((void *) x.ra) != hipSuccess) (void) hipGetLastError(); r.clear(); n = 0; }
  ~Pins() { if (n) { hipDeviceSynchronize(); release(); } }      // (an error path: nothing may still be writing them)
};

extern "C" {

// page-locked caller arenas (mspack_hip_pin / _unpin): the whole pages INSIDE [p, p + bytes) -- never a byte that is not the
// caller's (PinRange above).  A buffer that starts and ends on page boundaries is locked completely (the C drivers' arenas do:
// mspack_arena_alloc); of any other one the bytes before the first and behind the last boundary are copied the pageable way.
int mspack_hip_pin(const void *p, size_t bytes)
{
  uintptr_t ra, rb;
  if (!p || !bytes || !inner_pages(p, bytes, ra, rb)) return -1;
  const hipError_t e = hipHostRegister((void *) ra, rb - ra, hipHostRegisterPortable);       // (every device of the process: _multi)
  if (e != hipSuccess) { (void) hipGetLastError(); return (int) e; }
  std::lock_guard<std::mutex> lock(g_pin_mu);
  g_pins.push_back(PinRange{ ra, rb, p });
  return 0;
}
void mspack_hip_unpin(const void *p)
{
  uintptr_t base = 0;
  {
    std::lock_guard<std::mutex> lock(g_pin_mu);
    for (size_t i = 0; i < g_pins.size(); i++)
      if (g_pins[i].user == p) { base = g_pins[i].ra; g_pins.erase(g_pins.begin() + (long) i); break; }
  }
  if (base && hipHostUnregister((void *) base) != hipSuccess) (void) hipGetLastError();
}

} // extern "C"
