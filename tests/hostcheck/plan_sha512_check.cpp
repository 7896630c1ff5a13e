// tests/hostcheck/plan_sha512_check.cpp -- TEST INFRASTRUCTURE ONLY.  The host path's chunk planner (libmspack_amd/csrc/hip/host_plan.hpp)
// and the 64-bit digest units (MSPACK_HIP_KIND_SHA384 / _SHA512 with their two / three MSPACK_HIP_KIND_DIGEST_MORE tails): built with
// -fsanitize=address,undefined by tests/test_host_plan_sha512.py.   usage: plan_sha512_check <case> | list | dump
// The tables, the helpers and `dump` (the plans of tables without digest units, one line per plan, compared with
// tests/golden/plan_parent.txt) are plan_md5_check.cpp's: that file is included whole, its main under another name.
#define main plan_md5_check_main
#include "plan_md5_check.cpp"
#undef main

static mspack_hip_unit DG(unsigned kind, uint64_t out_off, uint32_t out_len) { return U(kind, 0xABCDEF, 0, out_off, out_len); }
static mspack_hip_unit MORE() { return U(MSPACK_HIP_KIND_DIGEST_MORE, 0x1234, 0, 0x5678, 0, 0x7Fu & ~MSPACK_HIP_UF_CRC32); }
static size_t tails_of(unsigned kind)
{
  return kind == MSPACK_HIP_KIND_SHA512 ? 3 : kind == MSPACK_HIP_KIND_SHA384 ? 2 : (kind == MSPACK_HIP_KIND_SHA1 || kind == MSPACK_HIP_KIND_SHA256) ? 1 : 0;
}
static void push_digest(Table &t, unsigned kind, uint64_t out_off, uint32_t out_len)
{
  t.units.push_back(DG(kind, out_off, out_len));
  for (size_t k = 0; k < tails_of(kind); k++) t.units.push_back(MORE());
}
// a row of 64 LZX units with digest units of all five hashes (and CRC-32 ranges) scattered through the table; with_new: SHA-384 / SHA-512 among them
static Table mixed(bool with_new)
{
  Table t = lzx_row(64, 8192, 65536), r;
  r.in_bytes = t.in_bytes; r.out_bytes = t.out_bytes;
  for (size_t i = 0; i < 64; i++) {
    r.units.push_back(t.units[i]);
    if (i % 3 == 0) push_digest(r, MSPACK_HIP_KIND_MD5, i * 65536 + i, (uint32_t)(1000 + (i * 7919) % 5000));
    if (with_new && i % 3 == 1) push_digest(r, MSPACK_HIP_KIND_SHA512, i * 65536 - 50, (uint32_t)(200 + (i * 15485863) % 9000));
    if (i % 4 == 1) push_digest(r, MSPACK_HIP_KIND_SHA256, i * 65536 - 100, (uint32_t)(300 + (i * 104729) % 7000));
    if (with_new && i % 4 == 2) push_digest(r, MSPACK_HIP_KIND_SHA384, i * 65536 + 7, (uint32_t)(100 + (i * 32452843) % 9000));
    if (i % 5 == 2) push_digest(r, MSPACK_HIP_KIND_SHA1, i * 65536 + 3, (uint32_t)(17 + (i * 1299709) % 3000));
    if (i % 7 == 3) push_digest(r, MSPACK_HIP_KIND_CRC32, i * 65536, 70000);
    if (with_new && i == 40) { push_digest(r, MSPACK_HIP_KIND_SHA384, 0, 0); push_digest(r, MSPACK_HIP_KIND_SHA512, r.out_bytes, 0); }
  }
  return r;
}

// heads keep ALL their tails at i + 1 .. in local[], behind the chunks, in the caller's relative order; no chunk holds a digest unit
static void case_tails_follow()
{
  Table t = mixed(true);
  BatchPlan p; char err[256];
  REQUIRE(plan(t, K(4, 4096, 4, 0), p, err) == 0);
  const size_t n = t.units.size();
  size_t heads = 0, tails = 0, want_tails = 0, n384 = 0, n512 = 0;
  for (const mspack_hip_unit &u : t.units) {
    heads += unit_is_digest_head(u); tails += u.kind == MSPACK_HIP_KIND_DIGEST_MORE; want_tails += tails_of(u.kind);
    n384 += u.kind == MSPACK_HIP_KIND_SHA384; n512 += u.kind == MSPACK_HIP_KIND_SHA512;
  }
  REQUIRE(tails == want_tails && n384 >= 10 && n512 >= 10 && p.n_dig == heads + tails && p.n_sha512 == n384 + n512);
  REQUIRE(p.chunks.size() == 4 && p.chunks.back().b == n - p.n_dig);
  for (size_t i = 0; i < n - p.n_dig; i++) REQUIRE(!unit_is_digest(p.local[i]));
  for (size_t i = n - p.n_dig; i < n; i++) {
    REQUIRE(unit_is_digest(p.local[i]) && p.local[i].kind == t.units[p.idx[i]].kind);
    if (i > n - p.n_dig) REQUIRE(p.idx[i - 1] < p.idx[i]);            // the caller's relative order
    REQUIRE(unit_wide_tails(p.local[i]) == tails_of(p.local[i].kind));
    for (size_t k = 1; k <= tails_of(p.local[i].kind); k++)
      REQUIRE(i + k < n && p.local[i + k].kind == MSPACK_HIP_KIND_DIGEST_MORE && p.idx[i + k] == p.idx[i] + k);
    if (p.local[i].kind == MSPACK_HIP_KIND_DIGEST_MORE) REQUIRE(p.local[i].in_off == 0 && p.local[i].out_off == 0 && p.local[i].flags == 0);
    else REQUIRE(p.local[i].out_len == 0 ? p.local[i].out_off == 0 : p.local[i].out_off + p.out_lo == t.units[p.idx[i]].out_off);
  }
}

// order: four consecutive lists of heads -- MD5, SHA-1, SHA-256, then SHA-384 and SHA-512 together --, each longest first, the CRC-32
// range list behind them; everything in front of the fourth list is what the same table without the new kinds gives
static void case_five_kinds_lists()
{
  Table t = mixed(true), m = mixed(false);
  BatchPlan p, q; char err[256];
  REQUIRE(plan(t, K(4, 4096, 4, 0), p, err) == 0 && plan(m, K(4, 4096, 4, 0), q, err) == 0);
  REQUIRE(p.md5_off + p.n_md5 == p.sha1_off && p.sha1_off + p.n_sha1 == p.sha256_off && p.sha256_off + p.n_sha256 == p.sha512_off);
  REQUIRE(p.sha512_off + p.n_sha512 == p.crc32r_off && p.order.size() == t.units.size() && p.md5_off == t.units.size() - p.n_dig);
  size_t n_tails = 0;
  for (const mspack_hip_unit &u : t.units) n_tails += u.kind == MSPACK_HIP_KIND_DIGEST_MORE;
  REQUIRE(p.crc32r_off + p.n_crc32r + n_tails == p.order.size());          // (the tails' slots stay unused behind the last list)
  const struct { size_t off, n; unsigned kind, kind2; } lists[4] = {
    { p.md5_off, p.n_md5, MSPACK_HIP_KIND_MD5, MSPACK_HIP_KIND_MD5 }, { p.sha1_off, p.n_sha1, MSPACK_HIP_KIND_SHA1, MSPACK_HIP_KIND_SHA1 },
    { p.sha256_off, p.n_sha256, MSPACK_HIP_KIND_SHA256, MSPACK_HIP_KIND_SHA256 }, { p.sha512_off, p.n_sha512, MSPACK_HIP_KIND_SHA384, MSPACK_HIP_KIND_SHA512 } };
  std::vector<int> seen(t.units.size(), 0);
  for (const auto &l : lists) {
    REQUIRE(l.n >= 10);
    size_t first = 0;
    for (size_t j = 0; j < l.n; j++) {
      const uint32_t x = p.order[l.off + j];
      REQUIRE(x >= t.units.size() - p.n_dig && x < t.units.size() && (p.local[x].kind == l.kind || p.local[x].kind == l.kind2) && !seen[x]++);
      if (j) REQUIRE(p.local[p.order[l.off + j - 1]].out_len >= p.local[x].out_len);
      first += p.local[x].kind == l.kind;
    }
    if (l.kind != l.kind2) REQUIRE(first >= 10 && l.n - first >= 10);    // the two algorithms together in one list, longest first over both
  }
  for (size_t j = 0; j < p.n_crc32r; j++) REQUIRE(p.local[p.order[p.crc32r_off + j]].kind == MSPACK_HIP_KIND_CRC32 && !seen[p.order[p.crc32r_off + j]]++);
  for (size_t i = t.units.size() - p.n_dig; i < t.units.size(); i++) REQUIRE(seen[i] == (p.local[i].kind != MSPACK_HIP_KIND_DIGEST_MORE));
  // the other lists name the same ranges in the same order as without the new kinds; chunks, spans and per-kind lists alike
  REQUIRE(q.n_md5 == p.n_md5 && q.n_sha1 == p.n_sha1 && q.n_sha256 == p.n_sha256 && q.n_crc32r == p.n_crc32r && q.n_sha512 == 0 && q.sha512_off == q.crc32r_off);
  REQUIRE(q.chunks.size() == p.chunks.size() && p.out_lo == q.out_lo && p.in_lo == q.in_lo && p.in_hi == q.in_hi);
  for (size_t j = 0; j < p.n_md5 + p.n_sha1 + p.n_sha256; j++) {
    const mspack_hip_unit &a = p.local[p.order[p.md5_off + j]], &b = q.local[q.order[q.md5_off + j]];
    REQUIRE(a.kind == b.kind && a.out_off == b.out_off && a.out_len == b.out_len);
  }
  for (size_t j = 0; j < p.n_crc32r; j++) {
    const mspack_hip_unit &a = p.local[p.order[p.crc32r_off + j]], &b = q.local[q.order[q.crc32r_off + j]];
    REQUIRE(a.out_off == b.out_off && a.out_len == b.out_len);
  }
  for (size_t c = 0; c < p.chunks.size(); c++) {
    REQUIRE(p.chunks[c].a == q.chunks[c].a && p.chunks[c].b == q.chunks[c].b && p.chunks[c].out_lo == q.chunks[c].out_lo && p.chunks[c].out_hi == q.chunks[c].out_hi);
    for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++) REQUIRE(p.chunks[c].order_off[k] == q.chunks[c].order_off[k] && p.chunks[c].order_n[k] == q.chunks[c].order_n[k]);
  }
  for (size_t j = 0; j < p.md5_off; j++) REQUIRE(p.order[j] == q.order[j]);
  // the new units alone: one chunk that holds nothing, one list, the longer range first whatever its algorithm
  Table o; o.in_bytes = 0; o.out_bytes = 5000;
  push_digest(o, MSPACK_HIP_KIND_SHA384, 200, 10); push_digest(o, MSPACK_HIP_KIND_SHA512, 100, 4900); push_digest(o, MSPACK_HIP_KIND_SHA384, 300, 20);
  REQUIRE(plan(o, K(4, 8u << 20, 256), p, err) == 0 && p.chunks.size() == 1 && p.chunks[0].b == 0 && p.n_dig == 10 && p.n_md5 + p.n_sha1 + p.n_sha256 + p.n_crc32r == 0);
  REQUIRE(p.n_sha512 == 3 && p.sha512_off == 0 && p.order[0] == 3 && p.order[1] == 7 && p.order[2] == 0 && p.out_lo == 100 && p.out_hi == 5000 && p.order.size() == 10);
}

// mspack_hip_decode_batch_multi's cut: never inside a range; a head and ALL its tails land in one shard, next to each other
static void case_shard_cuts_sha512()
{
  const size_t n = 12;
  Table t = lzx_row(n, 8192, 65536);
  std::vector<std::vector<uint32_t>> sh; bool asc = false;
  push_digest(t, MSPACK_HIP_KIND_SHA512, 6 * 65536 - 10, 20);           // across the even cut of two shards (units 5 | 6): units 12 .. 15
  push_digest(t, MSPACK_HIP_KIND_SHA384, 3 * 65536 + 5, 2 * 65536);     // units 3, 4, 5: across the first cut of three: units 16 .. 18
  push_digest(t, MSPACK_HIP_KIND_MD5, 11 * 65536, 65536);               // the last unit alone: unit 19
  push_digest(t, MSPACK_HIP_KIND_SHA512, 11 * 65536 + 1, 100);          // units 20 .. 23
  push_digest(t, MSPACK_HIP_KIND_SHA256, 11 * 65536 + 2, 100);          // units 24, 25
  push_digest(t, MSPACK_HIP_KIND_SHA384, 0, 0);                         // empty: units 26 .. 28
  auto where = [&](uint32_t x) { for (size_t s = 0; s < sh.size(); s++) for (uint32_t y : sh[s]) if (y == x) return (int) s; return -1; };
  for (int k = 2; k <= 3; k++) {
    REQUIRE(plan_shards(t.units.data(), t.units.size(), k, sh, asc) && asc && sh.size() == (size_t) k);
    size_t total = 0; for (auto &v : sh) total += v.size();
    REQUIRE(total == t.units.size());
    for (uint32_t x = 0; x < t.units.size(); x++) REQUIRE(where(x) >= 0);
    REQUIRE(where(5) == where(6) && where(12) == where(5) && where(13) == where(12) && where(14) == where(12) && where(15) == where(12));
    REQUIRE(where(3) == where(4) && where(4) == where(5) && where(16) == where(3) && where(17) == where(16) && where(18) == where(16));
    REQUIRE(where(19) == where(11) && where(20) == where(11) && where(21) == where(11) && where(22) == where(11) && where(23) == where(11));
    REQUIRE(where(24) == where(11) && where(25) == where(11) && where(26) == 0 && where(27) == 0 && where(28) == 0);
    REQUIRE(where(0) == 0 && where(11) == k - 1);
    // every shard is a table the planner takes: heads with their tails at i + 1 ..
    for (auto &v : sh) {
      for (size_t j = 0; j < v.size(); j++)
        for (size_t q = 1; q <= tails_of(t.units[v[j]].kind); q++) REQUIRE(j + q < v.size() && v[j + q] == v[j] + q);
      BatchPlan p; char err[256]; err[0] = 0;
      Table c = t;
      REQUIRE(plan_batch(c.units.data(), v.data(), v.size(), c.in_bytes, c.out_bytes, true, false, false, K(4, 8u << 20, 256), p, err, 256) == 0);
      for (size_t i = 0; i < p.local.size(); i++)
        for (size_t q = 1; q <= tails_of(p.local[i].kind); q++) REQUIRE(p.local[i + q].kind == MSPACK_HIP_KIND_DIGEST_MORE && p.idx[i + q] == p.idx[i] + q);
    }
  }
  // outputs that interleave: with the new units the batch is not cut at all
  Table r = lzx_row(n, 8192, 65536); for (size_t i = 0; i < n; i++) r.units[i].out_off = (n - 1 - i) * 65536;
  push_digest(r, MSPACK_HIP_KIND_SHA384, 0, 10);
  REQUIRE(!plan_shards(r.units.data(), r.units.size(), 2, sh, asc));
}

static void case_rejections_sha512()
{
  struct R { std::function<void(Table &)> make; const char *msg; };
  const R rs[] = {
    // SHA-384 with 1 tail, SHA-512 with 2 (behind them: the table's end, or a unit of another kind)
    { [](Table &c) { c.units.push_back(DG(MSPACK_HIP_KIND_SHA384, 0, 10)); c.units.push_back(MORE()); }, "unit 4: a SHA-384 unit must be followed by 2 MSPACK_HIP_KIND_DIGEST_MORE units" },
    { [](Table &c) { c.units.push_back(DG(MSPACK_HIP_KIND_SHA384, 0, 10)); c.units.push_back(MORE()); c.units.push_back(DG(MSPACK_HIP_KIND_MD5, 0, 10)); }, "unit 4: a SHA-384 unit must be followed by 2 MSPACK_HIP_KIND_DIGEST_MORE units" },
    { [](Table &c) { c.units.push_back(DG(MSPACK_HIP_KIND_SHA512, 0, 10)); c.units.push_back(MORE()); c.units.push_back(MORE()); }, "unit 4: a SHA-512 unit must be followed by 3 MSPACK_HIP_KIND_DIGEST_MORE units" },
    { [](Table &c) { c.units.push_back(DG(MSPACK_HIP_KIND_SHA512, 0, 10)); c.units.push_back(MORE()); c.units.push_back(MORE()); push_digest(c, MSPACK_HIP_KIND_SHA384, 0, 1); }, "unit 4: a SHA-512 unit must be followed by 3 MSPACK_HIP_KIND_DIGEST_MORE units" },
    { [](Table &c) { c.units.push_back(DG(MSPACK_HIP_KIND_SHA512, 0, 10)); }, "unit 4: a wide digest unit is the table's last unit (its MSPACK_HIP_KIND_DIGEST_MORE unit is missing)" },
    { [](Table &c) { c.units[1] = DG(MSPACK_HIP_KIND_SHA384, 0, 10); }, "unit 1: a wide digest unit must be followed by an MSPACK_HIP_KIND_DIGEST_MORE unit" },
    // more tails than the head needs: SHA-256 with 2, SHA-384 with 3, SHA-512 with 4
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA256, 0, 10); c.units.push_back(MORE()); }, "unit 6: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA1, 0, 10); c.units.push_back(MORE()); }, "unit 6: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA384, 0, 10); c.units.push_back(MORE()); }, "unit 7: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA512, 0, 10); c.units.push_back(MORE()); }, "unit 8: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    // a tail naming bytes, in every place
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA384, 0, 10); c.units[6].out_len = 1; }, "unit 6: an MSPACK_HIP_KIND_DIGEST_MORE unit names no bytes (in_len and out_len must be 0)" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA512, 0, 10); c.units[7].in_len = 4; }, "unit 7: an MSPACK_HIP_KIND_DIGEST_MORE unit names no bytes (in_len and out_len must be 0)" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA512, 0, 10); c.units[5].out_len = 16; }, "unit 5: an MSPACK_HIP_KIND_DIGEST_MORE unit names no bytes (in_len and out_len must be 0)" },
    // a lone tail
    { [](Table &c) { c.units.push_back(MORE()); }, "unit 4: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { c.units[0] = MORE(); }, "unit 0: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { c.units.push_back(DG(MSPACK_HIP_KIND_MD5, 0, 10)); c.units.push_back(MORE()); c.units.push_back(MORE()); }, "unit 5: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    // the conventions of every digest head
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA384, 0, 10); c.units[4].flags = MSPACK_HIP_UF_CRC32; }, "unit 4: a digest unit decodes nothing to take a CRC-32 of" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA512, 0, 10); c.units[4].in_len = 1; }, "unit 4: a digest unit reads no input (in_len must be 0)" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA512, 4 * 65536 - 9, 10); }, "unit 4: a digest unit's range leaves the output arena" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA384, 4 * 65536 + 1, 0); }, "unit 4: a digest unit's range leaves the output arena" },
    // the kinds around the new ones stay undefined
    { [](Table &c) { c.units[2].kind = 21; }, "unit 2: unknown kind 21" },
    { [](Table &c) { c.units[2].kind = 22; }, "unit 2: unknown kind 22" },
    { [](Table &c) { c.units[2].kind = 23; }, "unit 2: unknown kind 23" },
    { [](Table &c) { c.units[2].kind = 26; }, "unit 2: unknown kind 26" },
    { [](Table &c) { c.units[2].kind = 9; }, "unit 2: unknown kind 9" },
    { [](Table &c) { c.units[2].kind = 19; }, "unit 2: unknown kind 19" },
  };
  for (const R &r : rs) {
    Table c = lzx_row(4, 8192, 65536);
    r.make(c);
    BatchPlan p; char err[256];
    if (plan(c, K(4, 8u << 20, 256), p, err) != -1 || strcmp(err, r.msg) != 0) { printf("PLAN_FAIL rejection \"%s\": got \"%s\"\n", r.msg, err); exit(1); }
    for (size_t i = 0; i < c.units.size(); i++) REQUIRE(c.units[i].frame_base == 0xDEADu);
  }
  Table ok = lzx_row(4, 8192, 65536);
  push_digest(ok, MSPACK_HIP_KIND_SHA384, 4 * 65536 - 10, 10); push_digest(ok, MSPACK_HIP_KIND_SHA512, 4 * 65536, 0);
  ok.units[4].flags = 0x7Fu;                                            // (every other flag is ignored)
  BatchPlan p; char err[256];
  REQUIRE(plan(ok, K(4, 8u << 20, 256), p, err) == 0 && p.n_dig == 7 && p.n_sha512 == 2 && p.n_sha1 == 0 && p.n_sha256 == 0 && p.local[4].flags == 0);
}

int main(int argc, char **argv)
{
  const std::string which = argc > 1 ? argv[1] : "all";
  if (which == "dump") { dump_all(); return 0; }
  const struct { const char *name; void (*run)(); } cases[] = {
    { "tails_follow", case_tails_follow }, { "five_kinds_lists", case_five_kinds_lists }, { "shard_cuts", case_shard_cuts_sha512 }, { "rejections", case_rejections_sha512 },
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
