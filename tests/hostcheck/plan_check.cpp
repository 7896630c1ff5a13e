// tests/hostcheck/plan_check.cpp -- TEST INFRASTRUCTURE ONLY.  The host path's chunk planner (libmspack_amd/csrc/hip/host_plan.hpp:
// plan_batch) asked what plan it makes: this file includes that header alone -- no HIP, no emulator -- and is built with
// -fsanitize=address,undefined by tests/test_host_plan.py.   usage: plan_check <case> | plan_check list
// Every case builds its unit table by hand; an accepted plan also has to satisfy check_plan's general invariants.
#include "host_plan.hpp"
#include <string.h>
#include <stdlib.h>
#include <string>
#include <set>
#include <functional>

#define REQUIRE(cond) do { if (!(cond)) { printf("PLAN_FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static mspack_hip_unit U(unsigned kind, uint64_t in_off, uint32_t in_len, uint64_t out_off, uint32_t out_len, uint32_t flags = 0,
                         uint32_t ref_len = 0, uint32_t in_chunk = 0)
{
  mspack_hip_unit u;
  memset(&u, 0, sizeof(u));
  u.kind = (uint8_t) kind; u.in_off = in_off; u.in_len = in_len; u.out_off = out_off; u.out_len = out_len;
  u.flags = flags; u.ref_len = ref_len; u.in_chunk = in_chunk; u.window_bits = 16; u.frame_base = 0xDEADu;
  return u;
}
static PlanKnobs K(size_t max_chunks, size_t chunk_bytes, size_t chunk_units, int shape = -1, std::vector<uint64_t> weights = {})
{
  PlanKnobs k; k.max_chunks = max_chunks; k.chunk_bytes = chunk_bytes; k.chunk_units = chunk_units; k.shape = shape; k.weights = weights;
  return k;
}
static const PlanKnobs DEFAULTS = K(4, 8u << 20, 256);

struct Case {
  std::vector<mspack_hip_unit> units;      // the caller's table (plan_batch writes frame_base into it)
  std::vector<mspack_hip_unit> given;      // ... as it was handed in
  size_t in_bytes = 0, out_bytes = 0;
  BatchPlan p;
  char err[256];
  int plan(const PlanKnobs &kn, bool to_host = true, bool dev_out = false, bool per_unit_back = false) {
    given = units; err[0] = 0; p = BatchPlan();
    const int rc = plan_batch(units.data(), nullptr, units.size(), in_bytes, out_bytes, to_host, dev_out, per_unit_back, kn, p, err, sizeof(err));
    if (rc == 0) check_plan(kn);
    return rc;
  }
  // what every accepted plan has to satisfy
  void check_plan(const PlanKnobs &kn) const {
    const size_t n = units.size();
    REQUIRE(p.idx.size() == n && p.local.size() == n && p.order.size() == n + p.n_crc);
    REQUIRE(!p.chunks.empty() && p.chunks.size() <= kn.max_chunks);
    REQUIRE(p.chunks.front().a == 0 && p.chunks.back().b == n);
    std::set<uint32_t> seen;
    for (size_t i = 0; i < n; i++) {
      const mspack_hip_unit &g = given[p.idx[i]], &l = p.local[i];
      REQUIRE(seen.insert(p.idx[i]).second);
      REQUIRE(l.in_off + p.in_lo == g.in_off);                                   // the rebased offsets reproduce the caller's
      if (g.kind != MSPACK_HIP_KIND_XORSUM) REQUIRE(l.out_off + p.out_lo == g.out_off);
      if (i) REQUIRE(given[p.idx[i - 1]].in_off <= g.in_off);                    // ascending in_off
      uint64_t tl, th;
      if (unit_side_table(g, tl, th)) REQUIRE(((uint64_t) l.in_chunk << 2) + p.in_lo == tl);
      REQUIRE(units[p.idx[i]].frame_base == l.frame_base);                       // written back into the caller's array
    }
    for (size_t ci = 0; ci < p.chunks.size(); ci++) {
      const Chunk &c = p.chunks[ci];
      REQUIRE(c.a < c.b);
      REQUIRE((c.in_lo & 15u) == 0);                                             // every chunk's copy keeps the units' alignment
      if (ci) REQUIRE(c.a == p.chunks[ci - 1].b);                                // consecutive ranges
      REQUIRE(c.in_lo >= p.in_lo && c.in_hi <= p.in_hi && c.out_lo >= p.out_lo && c.out_hi <= p.out_hi);
      for (size_t i = c.a; i < c.b; i++) {
        const mspack_hip_unit &g = given[p.idx[i]];
        REQUIRE(c.in_lo <= g.in_off && g.in_off + g.in_len <= c.in_hi);          // the unit's stream ...
        uint64_t tl, th;
        mspack_hip_unit t = g; t.ref_len = p.local[i].ref_len;                   // (ref_len as the planner kept it)
        if (unit_side_table(t, tl, th)) REQUIRE(c.in_lo <= tl && th <= c.in_hi); // ... and its side table
        if (g.kind == MSPACK_HIP_KIND_XORSUM) continue;
        REQUIRE(c.out_lo <= g.out_off - unit_below(t) && g.out_off + g.out_len + unit_above(t) <= c.out_hi);
      }
      // the per-kind slices partition the chunk's units of that kind, longest first
      for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++) {
        std::set<uint32_t> want, got;
        for (size_t i = c.a; i < c.b; i++) if (p.local[i].kind == k) want.insert((uint32_t) i);
        REQUIRE(c.order_off[k] + c.order_n[k] <= p.order.size());
        for (size_t j = 0; j < c.order_n[k]; j++) {
          const uint32_t x = p.order[c.order_off[k] + j];
          REQUIRE(got.insert(x).second);
          if (j) {
            const mspack_hip_unit &a = p.local[p.order[c.order_off[k] + j - 1]], &b = p.local[x];
            REQUIRE(a.in_len + (a.out_len >> 2) >= b.in_len + (b.out_len >> 2));
          }
        }
        REQUIRE(want == got);
      }
      REQUIRE(c.crc_off + c.crc_n <= p.order.size());
    }
  }
  size_t chunk_units(size_t ci) const { return p.chunks[ci].b - p.chunks[ci].a; }
  uint64_t chunk_weight(size_t ci) const { uint64_t w = 0; for (size_t i = p.chunks[ci].a; i < p.chunks[ci].b; i++) w += p.local[i].in_len; return w; }
};

// n plain LZX units, in_len bytes in / out_len out each, back to back
static Case lzx_row(size_t n, uint32_t in_len, uint32_t out_len)
{
  Case c;
  for (size_t i = 0; i < n; i++) c.units.push_back(U(MSPACK_HIP_KIND_LZX, i * in_len, in_len, (uint64_t) i * out_len, out_len));
  c.in_bytes = n * in_len; c.out_bytes = (uint64_t) n * out_len;
  return c;
}

static void case_one_unit()
{
  Case c;
  c.units.push_back(U(MSPACK_HIP_KIND_LZX, 48, 1000, 4096, 65536));
  c.in_bytes = 2048; c.out_bytes = 4096 + 65536;
  REQUIRE(c.plan(DEFAULTS) == 0);
  REQUIRE(c.p.chunks.size() == 1 && c.p.monotone && !c.p.has_qtm && c.p.n_crc == 0);
  REQUIRE(c.p.in_lo == 48 && c.p.in_hi == 1048 && c.p.out_lo == 4096 && c.p.out_hi == 4096 + 65536);
  const Chunk &k = c.p.chunks[0];
  REQUIRE(k.in_lo == 48 && k.in_hi == 1048 && k.out_lo == 4096 && k.out_hi == 4096 + 65536);
  REQUIRE(k.order_n[MSPACK_HIP_KIND_LZX] == 1 && k.fm_n == 0 && !k.has_ftab);
  REQUIRE(c.p.n_frames == 3 && c.p.n_rec_slots == 0 && c.p.in_sum == 1000);
  REQUIRE(c.plan(DEFAULTS, false, true) == 0 && c.p.out_lo == 0 && c.p.local[0].out_off == 4096);      // dev_out: addressed as is
  c.units[0].in_off = 40;                                                           // in_lo keeps the units' alignment
  REQUIRE(c.plan(DEFAULTS) == 0 && c.p.in_lo == 32 && c.p.local[0].in_off == 8);
}

static void case_shapes()
{
  Case c = lzx_row(64, 8192, 65536);
  REQUIRE(c.plan(K(4, 4096, 4, 0)) == 0 && c.p.chunks.size() == 4);
  for (size_t ci = 0; ci < 4; ci++) REQUIRE(c.chunk_units(ci) == 16);               // equal shares of equal units
  REQUIRE(c.plan(K(4, 4096, 4, 1)) == 0 && c.p.chunks.size() == 4);                 // 1 : 1 : 2 : 4
  for (size_t ci = 1; ci < 4; ci++) REQUIRE(c.chunk_weight(ci) >= c.chunk_weight(ci - 1));
  for (size_t ci = 0; ci < 3; ci++) REQUIRE(c.chunk_units(3) > c.chunk_units(ci));
  REQUIRE(c.plan(K(4, 4096, 4, 2)) == 0 && c.p.chunks.size() == 4);                 // a first chunk of half a share
  REQUIRE(c.chunk_units(0) < c.chunk_units(1));
  REQUIRE(c.plan(K(4, 4096, 4, 0, { 4, 3, 2, 1 })) == 0 && c.p.chunks.size() == 4); // spelled out: they win over the shape
  REQUIRE(c.chunk_units(0) > c.chunk_units(3));
  // by destination: to the host shape 2, to the device shape 1
  REQUIRE(c.plan(K(4, 4096, 4), true) == 0 && c.p.chunks.size() == 4 && c.chunk_units(0) < c.chunk_units(1));
  REQUIRE(c.plan(K(4, 4096, 4), false, true) == 0 && c.p.chunks.size() == 4 && c.chunk_units(3) > c.chunk_units(2));
}

static void case_unit_cap()
{
  Case c = lzx_row(10, 8192, 65536);
  for (int i = 0; i < 3; i++) c.units.push_back(U(MSPACK_HIP_KIND_XORSUM, i * 8192, 8192, 0, 0));      // (ride along: no reason to cut)
  REQUIRE(c.plan(K(8, 1, 4, 0)) == 0);
  REQUIRE(c.p.chunks.size() <= 2);                                                  // 10 decoding units / 4 per chunk
  REQUIRE(c.plan(K(8, 8192 * 3, 1, 0)) == 0 && c.p.chunks.size() <= 3);             // ... and the bytes' cap: 80 KiB / 24 KiB
  REQUIRE(c.plan(K(2, 1, 1, 0)) == 0 && c.p.chunks.size() == 2);                    // ... and max_chunks
}

static void case_mixed_kinds()
{
  Case c;
  const uint32_t FT = MSPACK_HIP_UF_FRAME_TABLE;
  uint64_t in = 8, out = 0, tab = 32768;      // streams of 1000 bytes at 1 KiB strides, 8 bytes off a 16-byte row; the side tables behind them, 64 bytes apart
  size_t table_slots = 0;
  auto add = [&](unsigned kind, uint32_t out_len, uint32_t flags, uint32_t ref_len, bool side_table) {
    mspack_hip_unit u = U(kind, in, 1000, 0, out_len, flags, ref_len, side_table ? (uint32_t)(tab >> 2) : 0);
    if (side_table) tab += 64;
    out = (out + unit_below(u) + 15) & ~15ull;
    u.out_off = out;
    out += out_len + unit_above(u);
    in += 1024;
    c.units.push_back(u);
  };
  for (int round = 0; round < 2; round++) {
    add(MSPACK_HIP_KIND_LZX, 65536, FT, 7, true); table_slots += 3;                 // (ref_len means nothing here: cleared)
    add(MSPACK_HIP_KIND_LZX, 65536, 0, 0, false);
    add(MSPACK_HIP_KIND_MSZIP, 65536, FT, 0, true); table_slots += 2;
    add(MSPACK_HIP_KIND_MSZIP, 65536, FT | MSPACK_HIP_UF_MSZIP_REPAIR, 0, false);
    add(MSPACK_HIP_KIND_QUANTUM, 40000, MSPACK_HIP_UF_QTM_MARKS, 4, true);
    add(MSPACK_HIP_KIND_LZX_DELTA, 40000, 0, 5000, false);
    add(MSPACK_HIP_KIND_LZSS, 3000, 0, 0, false);
    add(MSPACK_HIP_KIND_XORSUM, 0, 0, 0, false);
  }
  c.in_bytes = tab; c.out_bytes = out;
  REQUIRE(c.plan(K(4, 1, 2, 0)) == 0);
  REQUIRE(c.p.chunks.size() == 4 && c.p.monotone && c.p.has_qtm);
  REQUIRE(c.p.n_rec_slots == table_slots && table_slots == 10);
  REQUIRE(c.p.n_frames == 10 + 2 * (3 + 2));                                        // + LZX without a table, LZX DELTA (40000 / 32768 + 1)
  for (size_t i = 0; i < c.p.local.size(); i++) {
    const mspack_hip_unit &l = c.p.local[i];
    if (unit_has_ftab(l)) REQUIRE(l.frame_base + unit_frames(l) <= table_slots);    // table units: the lowest slots
    else if (unit_frames(l)) REQUIRE(l.frame_base >= table_slots);
    REQUIRE(c.units[c.p.idx[i]].frame_base == l.frame_base && l.frame_base != 0xDEADu);
    if (l.kind == MSPACK_HIP_KIND_LZX) REQUIRE(l.ref_len == 0);
    if (l.kind == MSPACK_HIP_KIND_LZX_DELTA) REQUIRE(l.ref_len == 5000);
  }
  size_t slots = 0;
  for (const Chunk &k : c.p.chunks) {
    std::set<size_t> got;
    for (size_t i = k.a; i < k.b; i++)
      if (unit_has_ftab(c.p.local[i])) for (size_t f = 0; f < unit_frames(c.p.local[i]); f++) REQUIRE(got.insert(c.p.local[i].frame_base + f).second);
    REQUIRE(got.size() == k.fm_n && k.has_ftab == !got.empty());
    if (!got.empty()) REQUIRE(*got.begin() == k.fm_lo && *got.rbegin() == k.fm_lo + k.fm_n - 1);
    slots += k.fm_n;
  }
  REQUIRE(slots == table_slots);
}

static void case_chm_style()
{
  Case c;
  const size_t n = 64;
  const uint64_t tabs = n * 1024;
  c.in_bytes = tabs + 16 * n; c.out_bytes = n * 65536;
  for (size_t i = 0; i < n; i++)               // every interval reads "to the end of the file"; the frame tables lie behind the streams
    c.units.push_back(U(MSPACK_HIP_KIND_LZX, i * 1024, (uint32_t)(c.in_bytes - i * 1024), i * 65536, 65536, MSPACK_HIP_UF_FRAME_TABLE, 0,
                        (uint32_t)((tabs + 16 * i) >> 2)));
  REQUIRE(c.plan(K(4, 4096, 4, 0)) == 0 && c.p.chunks.size() == 4);
  for (size_t ci = 0; ci < 4; ci++) {
    // balanced by distance to the next in_off, not by in_len: 63 units weigh 1024, the last one its 2048 to the end of the arena,
    // so the three cuts fall behind 16.25, 32.5 and 48.75 units' worth -- no chunk is further than one unit from n / 4.  (By
    // in_len the early units weigh most and the last chunk would hold about half of all units.)
    REQUIRE(c.chunk_units(ci) + 1 >= n / 4 && c.chunk_units(ci) <= n / 4 + 1);
    for (size_t i = c.p.chunks[ci].a; i < c.p.chunks[ci].b; i++) {
      const uint64_t tl = tabs + 16 * c.p.idx[i];
      REQUIRE(c.p.chunks[ci].in_lo <= tl && tl + 8 <= c.p.chunks[ci].in_hi);
    }
  }
  REQUIRE(c.p.n_rec_slots == n * 3 && c.p.n_frames == n * 3);
}

static void case_xorsum_only()
{
  Case c;
  for (int i = 0; i < 5; i++) c.units.push_back(U(MSPACK_HIP_KIND_XORSUM, 16 + i * 100, 100, 0, 0));
  c.in_bytes = 1024; c.out_bytes = 0;
  REQUIRE(c.plan(K(4, 1, 1, 0)) == 0);
  REQUIRE(c.p.chunks.size() == 1 && c.p.out_lo == c.p.out_hi && c.p.chunks[0].out_lo == c.p.chunks[0].out_hi);
  REQUIRE(c.p.chunks[0].order_n[MSPACK_HIP_KIND_XORSUM] == 5 && c.p.in_sum == 0 && c.p.n_frames == 0);
}

static void case_not_monotone()
{
  Case c = lzx_row(16, 8192, 65536);
  for (size_t i = 0; i < 16; i++) c.units[i].out_off = (15 - i) * 65536;            // the outputs descend while the inputs ascend
  REQUIRE(c.plan(K(4, 4096, 4, 0), true, false, true) == 0);
  REQUIRE(!c.p.monotone && c.p.chunks.size() == 1);
  REQUIRE(c.plan(K(4, 4096, 4, 0), true, false, false) == 0);                       // found by the planner too
  REQUIRE(!c.p.monotone && c.p.chunks.size() == 1);
  Case d = lzx_row(16, 8192, 65536);                                                // ascending, but the caller says unit by unit
  REQUIRE(d.plan(K(4, 4096, 4, 0), true, false, true) == 0 && !d.p.monotone && d.p.chunks.size() == 1);
  REQUIRE(d.plan(K(4, 4096, 4, 0), true, false, false) == 0 && d.p.monotone && d.p.chunks.size() == 4);
}

static void case_crc_lists()
{
  Case c;
  for (size_t j = 0; j < 10; j++) {              // the caller's table runs against the arena: unit j lies at position 9 - j
    const size_t i = 9 - j;
    c.units.push_back(U(MSPACK_HIP_KIND_LZX, i * 4096, 4096, i * 65536, (uint32_t)(1000 * (10 - i))));      // (the longer ones first)
  }
  c.in_bytes = 10 * 4096; c.out_bytes = 10 * 65536;
  c.units[9 - 2].flags |= MSPACK_HIP_UF_CRC32;                                      // arena positions 2 and 7 decode ...
  c.units[9 - 7].flags |= MSPACK_HIP_UF_CRC32;
  c.units[9 - 4].flags |= MSPACK_HIP_UF_CRC32; c.units[9 - 4].kind = 0;             // ... position 4 is carried along: no digest
  REQUIRE(c.plan(DEFAULTS) == 0 && c.p.chunks.size() == 1 && c.p.n_crc == 2);
  const Chunk &k = c.p.chunks[0];
  REQUIRE(k.crc_n == 2 && k.crc_max == 8000);                                      // position 2's, not the last flagged unit's 3000
  REQUIRE(c.p.order[k.crc_off] == 2 && c.p.order[k.crc_off + 1] == 7);
  REQUIRE(c.p.idx[2] == 9 - 2 && c.p.idx[7] == 9 - 7);
  REQUIRE(k.crc_off == 9);                                                          // behind the nine units that have a kind
  REQUIRE(c.plan(K(2, 1, 4, 0)) == 0 && c.p.chunks.size() == 2 && c.p.n_crc == 2);  // one flagged unit per chunk
  for (size_t ci = 0; ci < 2; ci++) {
    const Chunk &h = c.p.chunks[ci];
    const uint32_t x = ci ? 7u : 2u;
    REQUIRE(h.crc_n == 1 && c.p.order[h.crc_off] == x && h.crc_max == 1000u * (10 - x) && h.a <= x && x < h.b);
  }
}

static void case_rejections()
{
  struct R { std::function<void(Case &)> make; const char *msg; };
  const R rs[] = {
    { [](Case &c) { c.units[1].kind = 9; }, "unit 1: unknown kind 9" },
    { [](Case &c) { c.units[0] = U(MSPACK_HIP_KIND_XORSUM, 0, 100, 0, 4); }, "unit 0: a checksum unit has no output" },
    { [](Case &c) { c.units[0] = U(MSPACK_HIP_KIND_XORSUM, 0, 100, 0, 0, MSPACK_HIP_UF_CRC32); }, "unit 0: a checksum unit decodes nothing to take a CRC-32 of" },
    { [](Case &c) { c.units[0] = U(MSPACK_HIP_KIND_XORSUM, 4 * 8192 - 50, 100, 0, 0); }, "unit outside arena" },
    { [](Case &c) { c.units[3].in_len = 8193; }, "unit outside arena" },
    { [](Case &c) { c.units[3].out_len = 65537; }, "unit outside arena" },
    { [](Case &c) { c.units[3].kind = MSPACK_HIP_KIND_MSZIP; }, "unit outside arena" },      // (the last unit's 32 KiB of slack)
    { [](Case &c) { c.units[0].kind = MSPACK_HIP_KIND_LZSS; c.units[0].out_off = 100; }, "unit's lower region outside arena" },
    { [](Case &c) { c.units[0].kind = MSPACK_HIP_KIND_LZX_DELTA; c.units[0].out_off = 100; c.units[0].ref_len = 101; }, "unit's lower region outside arena" },
    { [](Case &c) { c.units[1].flags = MSPACK_HIP_UF_FRAME_TABLE; c.units[1].in_chunk = (4 * 8192 - 4) >> 2; }, "unit's table outside arena" },
    { [](Case &c) { c.units[0] = U(MSPACK_HIP_KIND_QUANTUM, 0, 8192, 2, 1000, MSPACK_HIP_UF_QTM_MARKS, 2, 64); }, "unit 0: a Quantum unit with marks needs out_off % 4 == 0" },
  };
  for (const R &r : rs) {
    Case c = lzx_row(4, 8192, 65536);
    r.make(c);
    if (c.plan(DEFAULTS) != -1 || strcmp(c.err, r.msg) != 0) { printf("PLAN_FAIL rejection \"%s\": got \"%s\"\n", r.msg, c.err); exit(1); }
    for (size_t i = 0; i < c.units.size(); i++) REQUIRE(c.units[i].frame_base == 0xDEADu);      // refused before anything was written
  }
  Case ok = lzx_row(4, 8192, 65536);
  REQUIRE(ok.plan(DEFAULTS) == 0);
}

int main(int argc, char **argv)
{
  const struct { const char *name; void (*run)(); } cases[] = {
    { "one_unit", case_one_unit }, { "shapes", case_shapes }, { "unit_cap", case_unit_cap }, { "mixed_kinds", case_mixed_kinds },
    { "chm_style", case_chm_style }, { "xorsum_only", case_xorsum_only }, { "not_monotone", case_not_monotone },
    { "crc_lists", case_crc_lists }, { "rejections", case_rejections },
  };
  const std::string which = argc > 1 ? argv[1] : "all";
  bool ran = false;
  for (const auto &c : cases) {
    if (which == "list") { printf("%s\n", c.name); ran = true; continue; }
    if (which != "all" && which != c.name) continue;
    c.run();
    printf("PLAN_OK %s\n", c.name);
    ran = true;
  }
  return ran ? 0 : 2;
}
