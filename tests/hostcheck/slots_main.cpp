// tests/hostcheck/slots_main.cpp -- TEST INFRASTRUCTURE ONLY.  Context slots (include/mspack_hip.h: mspack_hip_set_slots) of the host half of
// shim.hip under real ASan / TSan, on the model runtime of hostcheck_runtime.cpp: batches of several application threads side by side
// in different slots of one device.  usage: hostcheck_slots <slots> [rounds] ; exit code 0 = every output equals the plaintext, the
// slot statistics add up, no violation of the runtime's modelled rules; the sanitizer's own exit code otherwise.
// A round: four threads with three batches each of different codecs and sizes (LZX-21 with frame tables, LZX-16, Quantum, MSZIP);
// one thread on the job API that waits for its units out of order; one thread whose first batch the planner rejects, whose second is
// small and whose third is larger than anything before it (its slot's buffers grow while the others run); one thread whose arenas
// are partly page-locked by itself and one whose arenas come out of the staging pool (the two process-global locks under batches
// at once: never a byte outside the caller's range, copies cut at registered boundaries -- the model counts what breaks them).
// Between rounds: mspack_hip_release(), and mspack_hip_set_slots() down to 1 and up again.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <string>
#include <thread>
#include <mutex>
#include <condition_variable>
#include "../../include/mspack_hip.h"
#include "../../libmspack_amd/csrc/corpus/corpus.h"

extern "C" int hostcheck_violations(void);

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "hostcheck_slots: %s:%d: check failed: %s (%s)\n", __FILE__, __LINE__, #c, mspack_hip_last_error()); exit(3); } } while (0)

struct Batch {
  std::vector<uint8_t> plain, comp;                      // plain: the expected output arena's decoded bytes, unit by unit
  std::vector<mspack_hip_unit> units;
  size_t out_bytes = 0;
};
// n LZX units of `ub` bytes (reset intervals of two frames), back to back, outputs back to back
static Batch lzx_batch(uint64_t seed, int n, size_t ub, int wbits, bool tables)
{
  Batch B;
  B.plain.resize((size_t) n * ub);
  B.comp.resize(mspk_lzx_bound(ub) * (size_t) n + 4096 + (tables ? (size_t) n * 64 : 0));
  std::vector<uint64_t> off(n), tab(n);
  std::vector<uint32_t> len(n);
  size_t tot = tables ? mspk_corpus_lzx_units_ft(seed, 0, MSPK_TEXT_MIX, n, ub, wbits, nullptr, 4, B.plain.data(), B.comp.data(), B.comp.size() - 64, off.data(), len.data(), tab.data())
                      : mspk_corpus_lzx_units(seed, MSPK_TEXT_MIX, n, ub, wbits, nullptr, 4, B.plain.data(), B.comp.data(), B.comp.size() - 64, off.data(), len.data());
  CHECK(tot != 0);
  B.comp.resize(tot + 64);
  B.units.resize(n);
  size_t fb = 0;
  for (int i = 0; i < n; i++) {
    mspack_hip_unit &u = B.units[i];
    memset(&u, 0, sizeof(u));
    u.in_off = off[i]; u.in_len = len[i] + 4; u.out_off = (uint64_t) i * ub; u.out_len = (uint32_t) ub;
    u.kind = MSPACK_HIP_KIND_LZX; u.window_bits = (uint8_t) wbits; u.reset_frames = 2; u.frame_base = (uint32_t) fb;
    if (tables) { u.flags |= MSPACK_HIP_UF_FRAME_TABLE; u.in_chunk = (uint32_t)(tab[i] / 4); }
    fb += ub / 32768 + 1;
  }
  B.out_bytes = (size_t) n * ub;
  return B;
}
// n Quantum folders of `ub` bytes: every frame's payload followed by the 0xFF trailer the cabinet driver adds (cabd.c:1330-1332)
static Batch qtm_batch(uint64_t seed, int n, size_t ub, int wbits)
{
  Batch B;
  B.plain.resize((size_t) n * ub);
  B.units.resize(n);
  std::vector<uint8_t> tmp(mspk_qtm_bound(ub));
  std::vector<uint32_t> fs(ub / 32768 + 1);
  for (int i = 0; i < n; i++) {
    uint8_t *p = B.plain.data() + (size_t) i * ub;
    mspk_gen_plaintext(seed + (uint64_t) i, MSPK_TEXT_MIX, p, ub);
    const size_t z = mspk_qtm_encode(p, ub, wbits, 0, tmp.data(), tmp.size(), fs.data());
    CHECK(z != 0);
    mspack_hip_unit &u = B.units[i];
    memset(&u, 0, sizeof(u));
    u.in_off = B.comp.size();
    size_t pos = 0;
    for (size_t k = 0; k < (ub + 32767) / 32768; k++) { B.comp.insert(B.comp.end(), tmp.data() + pos, tmp.data() + pos + fs[k]); B.comp.push_back(0xFF); pos += fs[k]; }
    u.in_len = (uint32_t)(B.comp.size() - u.in_off);
    u.out_off = (uint64_t) i * ub; u.out_len = (uint32_t) ub;
    u.kind = MSPACK_HIP_KIND_QUANTUM; u.window_bits = (uint8_t) wbits;
    while (B.comp.size() & 3u) B.comp.push_back(0);
  }
  B.comp.resize(B.comp.size() + 64);
  B.out_bytes = (size_t) n * ub;
  return B;
}
// n MSZIP folders of `ub` bytes: "CK" blocks of one stored deflate block each (RFC 1951 3.2.4), 32768 bytes per block but the last;
// every unit owns 32 KiB of slack behind its output
static Batch mszip_batch(uint64_t seed, int n, size_t ub)
{
  Batch B;
  const size_t stride = (ub + 32768 + 15) & ~(size_t) 15;
  B.plain.assign((size_t) n * stride, 0);
  B.units.resize(n);
  for (int i = 0; i < n; i++) {
    uint8_t *p = B.plain.data() + (size_t) i * stride;
    mspk_gen_plaintext(seed + (uint64_t) i, MSPK_TEXT_BINARY, p, ub);
    mspack_hip_unit &u = B.units[i];
    memset(&u, 0, sizeof(u));
    u.in_off = B.comp.size();
    for (size_t at = 0; at < ub; at += 32768) {
      const size_t nb = ub - at < 32768 ? ub - at : 32768;
      const uint8_t hdr[7] = { 'C', 'K', 0x01, (uint8_t)(nb & 0xFF), (uint8_t)(nb >> 8), (uint8_t)(~nb & 0xFF), (uint8_t)((~nb >> 8) & 0xFF) };
      B.comp.insert(B.comp.end(), hdr, hdr + 7);
      B.comp.insert(B.comp.end(), p + at, p + at + nb);
    }
    u.in_len = (uint32_t)(B.comp.size() - u.in_off);
    u.out_off = (uint64_t) i * stride; u.out_len = (uint32_t) ub;
    u.kind = MSPACK_HIP_KIND_MSZIP;
    while (B.comp.size() & 3u) B.comp.push_back(0);
  }
  B.comp.resize(B.comp.size() + 64);
  B.out_bytes = (size_t) n * stride;
  return B;
}
// every unit's result and bytes against the plaintext (the bytes between units are unspecified)
static void compare(const Batch &B, const uint8_t *out, const mspack_hip_result *res)
{
  for (size_t i = 0; i < B.units.size(); i++) {
    CHECK(res[i].err == 0 && res[i].out_len == B.units[i].out_len);
    CHECK(memcmp(out + B.units[i].out_off, B.plain.data() + B.units[i].out_off, B.units[i].out_len) == 0);
  }
}
static void decode_and_compare(const Batch &B, const uint8_t *in, uint8_t *out, size_t out_room)
{
  std::vector<mspack_hip_result> res(B.units.size());
  std::vector<mspack_hip_unit> u = B.units;
  memset(out, 0x5A, B.out_bytes);
  CHECK(mspack_hip_decode_batch(u.data(), u.size(), in, B.comp.size(), out, out_room, res.data()) == 0);
  compare(B, out, res.data());
}

// all threads of a round leave together
struct Gate {
  std::mutex mu; std::condition_variable cv; int left;
  explicit Gate(int n) : left(n) {}
  void pass() { std::unique_lock<std::mutex> lk(mu); if (--left == 0) cv.notify_all(); else cv.wait(lk, [&]() { return left == 0; }); }
};

struct Corpus { Batch lzx21, lzx16, qtm, zip, job, small, big; };

// four batches of different codecs and sizes, three per worker, every worker in another order
static void worker(const Corpus &K, int t, Gate &g)
{
  const Batch *all[4] = { &K.lzx21, &K.lzx16, &K.qtm, &K.zip };
  g.pass();
  for (int i = 0; i < 3; i++) {
    const Batch &B = *all[(t + i) % 4];
    std::vector<uint8_t> out(B.out_bytes + 64 + 100);
    decode_and_compare(B, B.comp.data(), out.data() + 7 * t, B.out_bytes + 64);
  }
}
// the job API beside them: the last unit first, then every third one backwards, then the rest
static void job_thread(const Corpus &K, Gate &g)
{
  const Batch &B = K.job;
  const size_t n = B.units.size();
  std::vector<uint8_t> out(B.out_bytes + 64);
  std::vector<mspack_hip_result> res(n);
  std::vector<mspack_hip_unit> u = B.units;
  g.pass();
  mspack_hip_job *job = mspack_hip_decode_batch_begin(u.data(), n, B.comp.data(), B.comp.size(), out.data(), out.size(), res.data());
  CHECK(job);
  auto look = [&](size_t i) {
    CHECK(mspack_hip_job_wait_unit(job, i) == 0);
    CHECK(res[i].err == 0 && res[i].out_len == B.units[i].out_len);
    CHECK(memcmp(out.data() + B.units[i].out_off, B.plain.data() + B.units[i].out_off, B.units[i].out_len) == 0);
  };
  look(n - 1);
  for (size_t i = n; i-- > 0; ) if (i % 3 == 0) look(i);
  for (size_t i = 0; i < n; i++) look(i);
  CHECK(mspack_hip_job_wait_unit(job, n) != 0);            // (no such unit)
  CHECK(mspack_hip_job_end(job) == 0);
  compare(B, out.data(), res.data());
}
// a batch the planner rejects (it has taken a slot and hands it back), a small batch, then one that makes its slot's buffers grow
static void grow_thread(const Corpus &K, Gate &g)
{
  g.pass();
  {
    const Batch &B = K.small;
    std::vector<mspack_hip_unit> u = B.units;
    std::vector<mspack_hip_result> res(u.size());
    std::vector<uint8_t> out(B.out_bytes + 64, 0x5A);
    u[u.size() - 1].in_off = B.comp.size() + 5;            // a unit outside the arena
    CHECK(mspack_hip_decode_batch(u.data(), u.size(), B.comp.data(), B.comp.size(), out.data(), out.size(), res.data()) != 0);
    for (size_t i = 0; i < out.size(); i++) CHECK(out[i] == 0x5A);
  }
  for (const Batch *B : { &K.small, &K.big, &K.small }) {
    std::vector<uint8_t> out(B->out_bytes + 64);
    decode_and_compare(*B, B->comp.data(), out.data(), out.size());
  }
}
// arenas of which the caller has page-locked the middle half: every copy crosses a registration's boundary, beside the others' copies
static void pin_thread(const Corpus &K, Gate &g)
{
  const Batch &B = K.lzx16;
  std::vector<uint8_t> arena(B.comp.size() + 8192), outv(B.out_bytes + 4096 + 64);
  uint8_t *a = arena.data() + 100, *out = outv.data() + 36;
  memcpy(a, B.comp.data(), B.comp.size());
  g.pass();
  for (int rep = 0; rep < 2; rep++) {
    const uint8_t *p_in = a + B.comp.size() / 4;
    uint8_t *p_out = out + B.out_bytes / 4;
    mspack_hip_pin(p_in, B.comp.size() / 2);
    mspack_hip_pin(p_out, B.out_bytes / 2);
    decode_and_compare(B, a, out, B.out_bytes + 64);
    mspack_hip_unpin(p_in); mspack_hip_unpin(p_out);
  }
}
// arenas out of the library's staging pool, taken and handed back while the others run
static void stage_thread(const Corpus &K, Gate &g)
{
  const Batch &B = K.lzx21;
  g.pass();
  for (int rep = 0; rep < 2; rep++) {
    uint8_t *in = (uint8_t *) mspack_hip_stage_alloc(B.comp.size()), *out = (uint8_t *) mspack_hip_stage_alloc(B.out_bytes + 64);
    CHECK(in && out);
    memcpy(in, B.comp.data(), B.comp.size());
    decode_and_compare(B, in, out, B.out_bytes + 64);
    mspack_hip_stage_free(in); mspack_hip_stage_free(out);
  }
}

// the batches one round runs: 4 workers x 3, the job, the rejected one + 3, 2 + 2
static const unsigned long long ROUND_BATCHES = 12 + 1 + 4 + 2 + 2;
static void round_of(const Corpus &K, int slots)
{
  CHECK(mspack_hip_set_slots(slots) == 0 && mspack_hip_slots() == slots);
  mspack_hip_slot_stats(nullptr, 1);
  Gate g(8);
  std::vector<std::thread> th;
  for (int t = 0; t < 4; t++) th.emplace_back(worker, std::cref(K), t, std::ref(g));
  th.emplace_back(job_thread, std::cref(K), std::ref(g));
  th.emplace_back(grow_thread, std::cref(K), std::ref(g));
  th.emplace_back(pin_thread, std::cref(K), std::ref(g));
  th.emplace_back(stage_thread, std::cref(K), std::ref(g));
  for (auto &t : th) t.join();
  unsigned long long s[3] = { 0, 0, 0 };
  mspack_hip_slot_stats(s, 0);
  printf("slots %d: %llu batches, at most %llu at once, %llu waited\n", slots, s[0], s[1], s[2]);
  CHECK(s[0] == ROUND_BATCHES);
  CHECK(s[1] >= 1 && s[1] <= (unsigned long long) slots);
  if (slots == 1) CHECK(s[1] == 1);
  // (eight threads leave a gate together with batches of milliseconds each: with more than one slot two of them meet)
  else CHECK(s[1] >= 2);
  mspack_hip_release();
}

int main(int argc, char **argv)
{
  const int slots = argc > 1 ? atoi(argv[1]) : 2, rounds = argc > 2 ? atoi(argv[2]) : 1;
  if (slots < 2 || slots > 4 || rounds < 1) { fprintf(stderr, "usage: hostcheck_slots 2..4 [rounds]\n"); return 2; }
  // the argument's range: refused values change nothing
  CHECK(mspack_hip_slots() >= 1);
  const int before = mspack_hip_slots();
  CHECK(mspack_hip_set_slots(0) == -1 && mspack_hip_set_slots(5) == -1 && mspack_hip_set_slots(-1) == -1 && mspack_hip_slots() == before);
  CHECK(mspack_hip_features() & MSPACK_HIP_FEAT_SLOTS);
  Corpus K;
  K.lzx21 = lzx_batch(0x5101, 24, 65536, 21, true);
  K.lzx16 = lzx_batch(0x5102, 40, 32768, 16, false);
  K.qtm = qtm_batch(0x5103, 6, 65536, 16);
  K.zip = mszip_batch(0x5104, 20, 40000);
  K.job = lzx_batch(0x5105, 48, 65536, 21, true);
  K.small = lzx_batch(0x5106, 4, 32768, 16, false);
  K.big = lzx_batch(0x5107, 64, 65536, 21, false);
  for (int r = 0; r < rounds; r++) {
    round_of(K, slots);                                     // up ...
    round_of(K, 1);                                         // ... down: "serialised inside", as before slots existed ...
    round_of(K, slots == 4 ? 2 : slots);                    // ... and up again (4: to another count)
    round_of(K, slots);
  }
  if (hostcheck_violations()) { fprintf(stderr, "hostcheck_slots: %d violation(s) of the runtime's modelled rules\n", hostcheck_violations()); return 4; }
  printf("HOSTCHECK_SLOTS_OK %d\n", slots);
  return 0;
}
