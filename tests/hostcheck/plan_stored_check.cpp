// tests/hostcheck/plan_stored_check.cpp -- TEST INFRASTRUCTURE ONLY.  The host path's chunk planner (libmspack_amd/csrc/hip/host_plan.hpp)
// and stored units (MSPACK_HIP_KIND_STORED): built with -fsanitize=address,undefined by tests/test_host_plan_stored.py.
// usage: plan_stored_check <case> | list | dump
// The tables, the helpers and `dump` are plan_md5_check.cpp's: that file is included whole, its main under another name.
#define main plan_md5_check_main
#include "plan_md5_check.cpp"
#undef main

static mspack_hip_unit S(uint64_t in_off, uint32_t in_len, uint64_t out_off, uint32_t out_len) { return U(MSPACK_HIP_KIND_STORED, in_off, in_len, out_off, out_len); }

// n stored units of `len` bytes back to back in both arenas, at odd offsets
static Table stored_row(size_t n, uint32_t len)
{
  Table c;
  for (size_t i = 0; i < n; i++) c.units.push_back(S(3 + i * len, len, 5 + (uint64_t) i * len, len));
  c.in_bytes = 3 + n * len; c.out_bytes = 5 + (uint64_t) n * len;
  return c;
}

// accepted, no slack and nothing below out_off, a list of their own behind the other kinds', weighted by their bytes when chunks are cut
static void case_accepted_and_listed()
{
  Table t = stored_row(8, 1000);
  BatchPlan p; char err[256];
  REQUIRE(plan(t, K(4, 8u << 20, 256), p, err) == 0 && p.chunks.size() == 1);
  const Chunk &c = p.chunks[0];
  REQUIRE(c.a == 0 && c.b == 8 && c.order_n[MSPACK_HIP_KIND_STORED] == 8 && p.in_sum == 8000 && p.n_frames == 0 && p.n_crc == 0);
  for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++) REQUIRE(c.order_n[k] == 0);
  REQUIRE(c.order_off[MSPACK_HIP_KIND_STORED] == 0 && p.order.size() == 8);
  // the spans are exactly the units' bytes (in_lo rounded down to a row): no slack above, nothing below
  REQUIRE(p.in_lo == 0 && p.in_hi == 8003 && p.out_lo == 5 && p.out_hi == 8005 && c.out_lo == 5 && c.out_hi == 8005);
  for (size_t i = 0; i < 8; i++) REQUIRE(p.local[i].kind == MSPACK_HIP_KIND_STORED && p.local[i].in_off == 3 + i * 1000 && p.local[i].out_off == i * 1000);
  // among other kinds: every kind's list holds its own units, the stored list stands behind the checksum units' and in front of the CRC list
  Table m = lzx_row(4, 8192, 65536);
  m.units.push_back(U(MSPACK_HIP_KIND_XORSUM, 100, 50, 0, 0));
  m.units.push_back(S(4 * 8192, 300, 4 * 65536, 300)); m.units.push_back(S(4 * 8192 + 300, 0, 4 * 65536 + 300, 0));
  m.units.push_back(S(4 * 8192 + 300, 70000, 4 * 65536 + 300, 70000));
  m.units[6].flags = MSPACK_HIP_UF_CRC32; m.units[7].flags = MSPACK_HIP_UF_CRC32 | MSPACK_HIP_UF_HARD_EOF | MSPACK_HIP_UF_FRAME_TABLE; m.units[1].flags = MSPACK_HIP_UF_CRC32;
  m.in_bytes = 4 * 8192 + 70300; m.out_bytes = 4 * 65536 + 70300;
  REQUIRE(plan(m, K(4, 8u << 20, 256), p, err) == 0 && p.chunks.size() == 1 && p.n_crc == 3 && p.n_frames == 12);
  const Chunk &d = p.chunks[0];
  REQUIRE(d.order_n[MSPACK_HIP_KIND_LZX] == 4 && d.order_n[MSPACK_HIP_KIND_XORSUM] == 1 && d.order_n[MSPACK_HIP_KIND_STORED] == 3 && d.order_n[MSPACK_HIP_KIND_MD5] == 0);
  REQUIRE(d.order_off[MSPACK_HIP_KIND_STORED] == d.order_off[MSPACK_HIP_KIND_XORSUM] + 1 && d.crc_off == d.order_off[MSPACK_HIP_KIND_STORED] + 3 && d.crc_n == 3);
  REQUIRE(d.crc_max == 70000 && !d.has_lzss_ring && d.out_hi == m.out_bytes && p.order.size() == 8 + 3);
  for (size_t j = 0; j < 3; j++) REQUIRE(p.local[p.order[d.order_off[MSPACK_HIP_KIND_STORED] + j]].kind == MSPACK_HIP_KIND_STORED);
  REQUIRE(p.local[p.order[d.order_off[MSPACK_HIP_KIND_STORED]]].in_len == 70000);      // longest first
  for (const mspack_hip_unit &u : p.local) if (u.kind == MSPACK_HIP_KIND_STORED) REQUIRE(u.frame_base == 12 && unit_frames(u) == 0 && !unit_has_ftab(u));
}

// chunks are cut through stored units like any others: by their bytes
static void case_chunks_by_bytes()
{
  // 64 units of 8 KiB: four chunks of 16
  Table t = stored_row(64, 8192);
  BatchPlan p; char err[256];
  REQUIRE(plan(t, K(4, 4096, 4, 0), p, err) == 0 && p.chunks.size() == 4 && p.monotone);
  for (size_t c = 0; c < 4; c++) {
    const Chunk &ch = p.chunks[c];
    REQUIRE(ch.a == 16 * c && ch.b == 16 * c + 16 && ch.order_n[MSPACK_HIP_KIND_STORED] == 16);
    REQUIRE(ch.out_lo == 5 + 16 * c * 8192 && ch.out_hi == 5 + 16 * (c + 1) * 8192 && ch.in_hi == 3 + 16 * (c + 1) * 8192);
  }
  // one unit that holds most of the bytes among small ones: the cut falls by bytes, not by units
  Table b;
  uint64_t in = 0, out = 0;
  auto add = [&](uint32_t n) { b.units.push_back(S(in, n, out, n)); in += n; out += n; };
  for (int i = 0; i < 20; i++) add(100);
  add(1000000);
  for (int i = 0; i < 20; i++) add(100);
  b.in_bytes = in; b.out_bytes = out;
  REQUIRE(plan(b, K(2, 4096, 4, 0), p, err) == 0 && p.chunks.size() == 2);
  REQUIRE(p.chunks[0].b == 21 && p.chunks[1].a == 21 && p.chunks[1].b == 41);           // the long unit fills the first share
  REQUIRE(p.in_sum == 1004000);
  // the shards of _multi: about equal bytes each
  std::vector<std::vector<uint32_t>> sh; bool asc = false;
  Table s = stored_row(12, 50000);
  REQUIRE(plan_shards(s.units.data(), s.units.size(), 3, sh, asc) && asc && sh.size() == 3 && sh[0].size() == 4 && sh[1].size() == 4 && sh[2].size() == 4);
}

static void case_rejections_stored()
{
  struct Rj { std::function<void(Table &)> make; const char *msg; };
  const Rj rs[] = {
    { [](Table &c) { c.units[3].in_len = 1001; }, "unit 3: a stored unit's input leaves the input arena" },
    { [](Table &c) { c.units[3].in_off = 4004; c.units[3].in_len = 0; }, "unit 3: a stored unit's input leaves the input arena" },
    { [](Table &c) { c.units[1].in_off = ~0ull; }, "unit 1: a stored unit's input leaves the input arena" },
    { [](Table &c) { c.units[3].out_len = 1001; }, "unit 3: a stored unit's output leaves the output arena" },
    { [](Table &c) { c.units[0].out_off = 4006; c.units[0].out_len = 0; }, "unit 0: a stored unit's output leaves the output arena" },
    { [](Table &c) { c.units[2].out_len = 0xFFFFFFFFu; }, "unit 2: a stored unit's output leaves the output arena" },
    { [](Table &c) { c.units[2].kind = 10; }, "unit 2: unknown kind 10" },
    { [](Table &c) { c.units[2].kind = 9; }, "unit 2: unknown kind 9" },
    { [](Table &c) { c.units[2].kind = 12; }, "unit 2: unknown kind 12" },
    { [](Table &c) { c.units[2].kind = 15; }, "unit 2: unknown kind 15" },
  };
  for (const Rj &r : rs) {
    Table c = stored_row(4, 1000);
    for (mspack_hip_unit &u : c.units) u.frame_base = 0xDEADu;
    r.make(c);
    BatchPlan p; char err[256];
    if (plan(c, K(4, 8u << 20, 256), p, err) != -1 || strcmp(err, r.msg) != 0) { printf("PLAN_FAIL rejection \"%s\": got \"%s\"\n", r.msg, err); exit(1); }
    for (size_t i = 0; i < c.units.size(); i++) REQUIRE(c.units[i].frame_base == 0xDEADu);
  }
  // the edges that are fine: a unit that ends exactly where the arenas end, empty units at the ends, a short input
  Table ok = stored_row(4, 1000);
  ok.units.push_back(S(4003, 0, 4005, 0)); ok.units.push_back(S(0, 10, 0, 4005));
  BatchPlan p; char err[256];
  REQUIRE(plan(ok, K(4, 8u << 20, 256), p, err) == 0 && p.chunks[0].order_n[MSPACK_HIP_KIND_STORED] == 6);
}

int main(int argc, char **argv)
{
  const std::string which = argc > 1 ? argv[1] : "all";
  if (which == "dump") { dump_all(); return 0; }
  const struct { const char *name; void (*run)(); } cases[] = {
    { "accepted_and_listed", case_accepted_and_listed }, { "chunks_by_bytes", case_chunks_by_bytes }, { "rejections", case_rejections_stored },
  };
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
