// tests/hostcheck/plan_crc32r_check.cpp -- TEST INFRASTRUCTURE ONLY.  The host path's chunk planner (libmspack_amd/csrc/hip/host_plan.hpp)
// and the CRC-32 range units (MSPACK_HIP_KIND_CRC32): built with -fsanitize=address,undefined by tests/test_host_plan_crc32r.py.
// usage: plan_crc32r_check <case> | list | dump
// The tables, the helpers and `dump` (the plans of tables without digest units, one line per plan, compared with
// tests/golden/plan_parent.txt) are plan_md5_check.cpp's: that file is included whole, its main under another name.
#define main plan_md5_check_main
#include "plan_md5_check.cpp"
#undef main

static mspack_hip_unit R(uint64_t out_off, uint32_t out_len) { return U(MSPACK_HIP_KIND_CRC32, 0xABCDEF, 0, out_off, out_len); }
static mspack_hip_unit TAIL() { return U(MSPACK_HIP_KIND_DIGEST_MORE, 0, 0, 0, 0); }

// a row of 64 LZX units with digest units of every kind scattered through the table; with_ranges: the CRC-32 range units among them
static Table scattered(bool with_ranges)
{
  Table t = lzx_row(64, 8192, 65536), r;
  r.in_bytes = t.in_bytes; r.out_bytes = t.out_bytes;
  for (size_t i = 0; i < 64; i++) {
    r.units.push_back(t.units[i]);
    if (i % 3 == 0) r.units.push_back(D5(i * 65536 + i, (uint32_t)(1000 + (i * 7919) % 5000)));
    if (with_ranges && i % 2 == 1) r.units.push_back(R(i * 65536 - 100, (uint32_t) std::min<uint64_t>(300 + (i * 104729) % 700000, r.out_bytes - (i * 65536 - 100))));
    if (i % 5 == 2) { r.units.push_back(U(MSPACK_HIP_KIND_SHA256, 0, 0, i * 65536 + 3, 500)); r.units.push_back(TAIL()); }
    if (with_ranges && i == 40) { r.units.push_back(R(0, 0)); r.units.push_back(R(r.out_bytes, 0)); r.units.push_back(R(0, (uint32_t) r.out_bytes)); }
  }
  return r;
}

// the range units stand behind the chunks with the other digest units, weigh nothing, and have a list of their own behind the
// SHA-256 list, in the caller's order; everything else of the plan is that of the table without them
static void case_list_placement()
{
  Table t = scattered(true), m = scattered(false);
  BatchPlan p, q; char err[256];
  REQUIRE(plan(t, K(4, 4096, 4, 0), p, err) == 0 && plan(m, K(4, 4096, 4, 0), q, err) == 0);
  size_t nr = 0;
  for (const mspack_hip_unit &u : t.units) nr += u.kind == MSPACK_HIP_KIND_CRC32;
  REQUIRE(nr == 35 && p.n_crc32r == nr && q.n_crc32r == 0 && p.n_dig == q.n_dig + nr);
  REQUIRE(p.n_md5 == q.n_md5 && p.n_sha1 == q.n_sha1 && p.n_sha256 == q.n_sha256 && p.n_crc == 0);
  REQUIRE(p.md5_off + p.n_md5 == p.sha1_off && p.sha1_off + p.n_sha1 == p.sha256_off && p.sha256_off + p.n_sha256 == p.crc32r_off);
  REQUIRE(p.crc32r_off + p.n_crc32r + p.n_sha256 == p.order.size() && p.order.size() == t.units.size());      // (the tails' slots stay unused)
  REQUIRE(q.crc32r_off == q.sha256_off + q.n_sha256);
  const size_t n = t.units.size();
  for (size_t j = 0; j < nr; j++) {
    const uint32_t x = p.order[p.crc32r_off + j];
    REQUIRE(x >= n - p.n_dig && x < n && p.local[x].kind == MSPACK_HIP_KIND_CRC32);
    if (j) REQUIRE(p.idx[p.order[p.crc32r_off + j - 1]] < p.idx[x]);       // the caller's order
    const mspack_hip_unit &o = t.units[p.idx[x]];
    REQUIRE(p.local[x].out_len == o.out_len && p.local[x].in_off == 0 && p.local[x].flags == 0);
    REQUIRE(o.out_len == 0 ? p.local[x].out_off == 0 : p.local[x].out_off + p.out_lo == o.out_off);
  }
  // no chunk and no other list holds one
  for (size_t i = 0; i < n - p.n_dig; i++) REQUIRE(!unit_is_digest(p.local[i]));
  for (size_t j = 0; j < p.crc32r_off; j++) REQUIRE(p.local[p.order[j]].kind != MSPACK_HIP_KIND_CRC32);
  // chunks, spans and the per-kind lists: those of the table without the range units
  REQUIRE(p.chunks.size() == q.chunks.size() && p.chunks.size() == 4 && p.in_lo == q.in_lo && p.in_hi == q.in_hi && p.out_lo == q.out_lo && p.out_hi == q.out_hi);
  for (size_t c = 0; c < p.chunks.size(); c++) {
    REQUIRE(p.chunks[c].a == q.chunks[c].a && p.chunks[c].b == q.chunks[c].b && p.chunks[c].out_lo == q.chunks[c].out_lo && p.chunks[c].out_hi == q.chunks[c].out_hi);
    REQUIRE(p.chunks[c].in_lo == q.chunks[c].in_lo && p.chunks[c].in_hi == q.chunks[c].in_hi);
    for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++) REQUIRE(p.chunks[c].order_off[k] == q.chunks[c].order_off[k] && p.chunks[c].order_n[k] == q.chunks[c].order_n[k]);
  }
  for (size_t j = 0; j < q.md5_off; j++) REQUIRE(p.order[j] == q.order[j]);
  // the other algorithms' lists name the same ranges in the same order
  for (size_t j = 0; j < p.n_md5; j++) REQUIRE(t.units[p.idx[p.order[p.md5_off + j]]].out_off == m.units[q.idx[q.order[q.md5_off + j]]].out_off);
  for (size_t j = 0; j < p.n_sha256; j++) REQUIRE(t.units[p.idx[p.order[p.sha256_off + j]]].out_off == m.units[q.idx[q.order[q.sha256_off + j]]].out_off);
}

// range units alone: one chunk that holds nothing, nothing to read, the span of the ranges
static void case_ranges_only()
{
  Table o; o.in_bytes = 0; o.out_bytes = 5000;
  o.units.push_back(R(100, 4900)); o.units.push_back(R(200, 10)); o.units.push_back(R(5000, 0)); o.units.push_back(R(150, 4000));
  BatchPlan p; char err[256];
  REQUIRE(plan(o, K(4, 8u << 20, 256), p, err) == 0 && p.chunks.size() == 1 && p.chunks[0].a == 0 && p.chunks[0].b == 0);
  REQUIRE(p.n_dig == 4 && p.n_crc32r == 4 && p.n_md5 == 0 && p.n_sha1 == 0 && p.n_sha256 == 0 && p.crc32r_off == 0 && p.order.size() == 4);
  REQUIRE(p.in_lo == 0 && p.in_hi == 0 && p.out_lo == 100 && p.out_hi == 5000);
  for (uint32_t j = 0; j < 4; j++) REQUIRE(p.order[j] == j && p.idx[j] == j);
  REQUIRE(p.local[0].out_off == 0 && p.local[1].out_off == 100 && p.local[2].out_off == 0 && p.local[3].out_off == 50);
  // to a device buffer the ranges are addressed as they are
  REQUIRE(plan(o, K(4, 8u << 20, 256), p, err, false, true) == 0 && p.out_lo == 0 && p.local[0].out_off == 100 && p.local[3].out_off == 150);
  // a range of 2^32 - 1 bytes is a range like any other
  Table g; g.in_bytes = 0; g.out_bytes = (size_t) 5 << 30;
  g.units.push_back(R(7, 0xFFFFFFFFu)); g.units.push_back(R(((uint64_t) 5 << 30) - 0xFFFFFFFFull, 0xFFFFFFFFu));
  REQUIRE(plan(g, K(4, 8u << 20, 256), p, err) == 0 && p.n_crc32r == 2 && p.out_lo == 7 && p.out_hi == ((uint64_t) 5 << 30));
}

// mspack_hip_decode_batch_multi's cut: never inside a range; a range unit goes to the shard that holds its range
static void case_shard_cuts_ranges()
{
  const size_t n = 12;
  Table t = lzx_row(n, 8192, 65536);
  std::vector<std::vector<uint32_t>> sh; bool asc = false;
  t.units.push_back(R(6 * 65536 - 10, 20));              // 12: across the even cut of two shards (units 5 | 6)
  t.units.push_back(R(3 * 65536 + 5, 2 * 65536));        // 13: units 3, 4, 5: across the first cut of three
  t.units.push_back(R(11 * 65536, 65536));               // 14: the last unit alone
  t.units.push_back(R(0, 0));                            // 15: empty
  t.units.push_back(R(8 * 65536 + 1, 65535));            // 16: inside unit 8
  auto where = [&](uint32_t x) { for (size_t s = 0; s < sh.size(); s++) for (uint32_t y : sh[s]) if (y == x) return (int) s; return -1; };
  for (int k = 2; k <= 3; k++) {
    REQUIRE(plan_shards(t.units.data(), t.units.size(), k, sh, asc) && asc && sh.size() == (size_t) k);
    size_t total = 0; for (auto &v : sh) total += v.size();
    REQUIRE(total == t.units.size());
    for (uint32_t x = 0; x < t.units.size(); x++) REQUIRE(where(x) >= 0);
    REQUIRE(where(5) == where(6) && where(12) == where(5));
    REQUIRE(where(3) == where(4) && where(4) == where(5) && where(13) == where(3));
    REQUIRE(where(14) == where(11) && where(15) == 0 && where(16) == where(8));
    REQUIRE(where(0) == 0 && where(11) == k - 1);
    // every shard is a table the planner takes, its ranges inside the shard's own span
    for (auto &v : sh) {
      BatchPlan p; char err[256]; err[0] = 0;
      Table c = t;
      REQUIRE(plan_batch(c.units.data(), v.data(), v.size(), c.in_bytes, c.out_bytes, true, false, false, K(4, 8u << 20, 256), p, err, 256) == 0);
      uint64_t lo = ~0ull, hi = 0;
      for (size_t i = 0; i < p.local.size() - p.n_dig; i++) { lo = std::min<uint64_t>(lo, p.local[i].out_off + p.out_lo); hi = std::max<uint64_t>(hi, p.local[i].out_off + p.out_lo + p.local[i].out_len); }
      for (size_t i = p.local.size() - p.n_dig; i < p.local.size(); i++)
        if (p.local[i].out_len) REQUIRE(p.local[i].out_off + p.out_lo >= lo && p.local[i].out_off + p.out_lo + p.local[i].out_len <= hi);
    }
  }
  // a range over the whole arena: one shard takes everything
  Table w = lzx_row(n, 8192, 65536); w.units.push_back(R(0, (uint32_t)(n * 65536)));
  REQUIRE(plan_shards(w.units.data(), w.units.size(), 3, sh, asc) && sh[0].size() == n + 1 && sh[1].empty() && sh[2].empty());
  // outputs that interleave: with a range unit the batch is not cut at all
  Table r = lzx_row(n, 8192, 65536); for (size_t i = 0; i < n; i++) r.units[i].out_off = (n - 1 - i) * 65536;
  r.units.push_back(R(0, 10));
  REQUIRE(!plan_shards(r.units.data(), r.units.size(), 2, sh, asc));
}

static void case_rejections_ranges()
{
  struct Rj { std::function<void(Table &)> make; const char *msg; };
  const Rj rs[] = {
    { [](Table &c) { c.units.push_back(R(4 * 65536 - 9, 10)); }, "unit 4: a digest unit's range leaves the output arena" },
    { [](Table &c) { c.units.push_back(R(4 * 65536 + 1, 0)); }, "unit 4: a digest unit's range leaves the output arena" },
    { [](Table &c) { c.units.push_back(R(1, 0xFFFFFFFFu)); }, "unit 4: a digest unit's range leaves the output arena" },
    { [](Table &c) { c.units[2] = R(0, 4 * 65536 + 1); }, "unit 2: a digest unit's range leaves the output arena" },
    { [](Table &c) { c.units.push_back(R(0, 10)); c.units[4].in_len = 1; }, "unit 4: a digest unit reads no input (in_len must be 0)" },
    { [](Table &c) { c.units.push_back(R(0, 10)); c.units.push_back(R(0, 10)); c.units[5].flags = MSPACK_HIP_UF_CRC32; }, "unit 5: a digest unit decodes nothing to take a CRC-32 of" },
    { [](Table &c) { c.units.push_back(R(0, 10)); c.units.push_back(TAIL()); }, "unit 5: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { c.units.push_back(R(0, 10)); c.units[4].kind = 19; }, "unit 4: unknown kind 19" },
    { [](Table &c) { c.units.push_back(R(0, 10)); c.units[4].kind = 21; }, "unit 4: unknown kind 21" },
  };
  for (const Rj &r : rs) {
    Table c = lzx_row(4, 8192, 65536);
    r.make(c);
    BatchPlan p; char err[256];
    if (plan(c, K(4, 8u << 20, 256), p, err) != -1 || strcmp(err, r.msg) != 0) { printf("PLAN_FAIL rejection \"%s\": got \"%s\"\n", r.msg, err); exit(1); }
    for (size_t i = 0; i < c.units.size(); i++) REQUIRE(c.units[i].frame_base == 0xDEADu);
  }
  Table ok = lzx_row(4, 8192, 65536);
  ok.units.push_back(R(4 * 65536 - 10, 10)); ok.units.push_back(R(4 * 65536, 0));
  ok.units[4].flags = 0x7Fu;                                            // (every other flag is ignored)
  BatchPlan p; char err[256];
  REQUIRE(plan(ok, K(4, 8u << 20, 256), p, err) == 0 && p.n_dig == 2 && p.n_crc32r == 2 && p.local[4].flags == 0);
}

int main(int argc, char **argv)
{
  const std::string which = argc > 1 ? argv[1] : "all";
  if (which == "dump") { dump_all(); return 0; }
  const struct { const char *name; void (*run)(); } cases[] = {
    { "list_placement", case_list_placement }, { "ranges_only", case_ranges_only }, { "shard_cuts", case_shard_cuts_ranges }, { "rejections", case_rejections_ranges },
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
