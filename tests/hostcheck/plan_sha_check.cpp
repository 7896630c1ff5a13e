// tests/hostcheck/plan_sha_check.cpp -- TEST INFRASTRUCTURE ONLY.  The host path's chunk planner (libmspack_amd/csrc/hip/host_plan.hpp)
// and the wide digest units (MSPACK_HIP_KIND_SHA1 / _SHA256 with their MSPACK_HIP_KIND_DIGEST_MORE tails): this file includes that
// header alone and is built with -fsanitize=address,undefined by tests/test_host_plan_sha.py.   usage: plan_sha_check <case> | list
#include "host_plan.hpp"
#include <string.h>
#include <stdlib.h>
#include <string>
#include <functional>

#define REQUIRE(cond) do { if (!(cond)) { printf("PLAN_FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static mspack_hip_unit U(unsigned kind, uint64_t in_off, uint32_t in_len, uint64_t out_off, uint32_t out_len, uint32_t flags = 0)
{
  mspack_hip_unit u;
  memset(&u, 0, sizeof(u));
  u.kind = (uint8_t) kind; u.in_off = in_off; u.in_len = in_len; u.out_off = out_off; u.out_len = out_len;
  u.flags = flags; u.window_bits = 16; u.frame_base = 0xDEADu;
  return u;
}
static PlanKnobs K(size_t max_chunks, size_t chunk_bytes, size_t chunk_units, int shape = -1)
{
  PlanKnobs k; k.max_chunks = max_chunks; k.chunk_bytes = chunk_bytes; k.chunk_units = chunk_units; k.shape = shape;
  return k;
}
struct Table { std::vector<mspack_hip_unit> units; size_t in_bytes = 0, out_bytes = 0; };
static Table lzx_row(size_t n, uint32_t in_len, uint32_t out_len)
{
  Table c;
  for (size_t i = 0; i < n; i++) c.units.push_back(U(MSPACK_HIP_KIND_LZX, i * in_len, in_len, (uint64_t) i * out_len, out_len));
  c.in_bytes = n * in_len; c.out_bytes = (uint64_t) n * out_len;
  return c;
}
static int plan(Table &t, const PlanKnobs &kn, BatchPlan &p, char *err)
{
  p = BatchPlan(); err[0] = 0;
  return plan_batch(t.units.data(), nullptr, t.units.size(), t.in_bytes, t.out_bytes, true, false, false, kn, p, err, 256);
}
static mspack_hip_unit D(unsigned kind, uint64_t out_off, uint32_t out_len) { return U(kind, 0xABCDEF, 0, out_off, out_len); }
static mspack_hip_unit MORE() { return U(MSPACK_HIP_KIND_DIGEST_MORE, 0x1234, 0, 0x5678, 0, 0x7Fu & ~MSPACK_HIP_UF_CRC32); }
static void push_digest(Table &t, unsigned kind, uint64_t out_off, uint32_t out_len)
{
  t.units.push_back(D(kind, out_off, out_len));
  if (kind != MSPACK_HIP_KIND_MD5) t.units.push_back(MORE());
}
// a row of 64 LZX units with digest units of all three algorithms scattered through the table (not only behind it)
static Table mixed(bool with_sha)
{
  Table t = lzx_row(64, 8192, 65536), r;
  r.in_bytes = t.in_bytes; r.out_bytes = t.out_bytes;
  for (size_t i = 0; i < 64; i++) {
    r.units.push_back(t.units[i]);
    if (i % 3 == 0) push_digest(r, MSPACK_HIP_KIND_MD5, i * 65536 + i, (uint32_t)(1000 + (i * 7919) % 5000));
    if (with_sha && i % 4 == 1) push_digest(r, MSPACK_HIP_KIND_SHA256, i * 65536 - 100, (uint32_t)(300 + (i * 104729) % 7000));
    if (with_sha && i % 5 == 2) push_digest(r, MSPACK_HIP_KIND_SHA1, i * 65536 + 3, (uint32_t)(17 + (i * 1299709) % 3000));
    if (with_sha && i == 40) { push_digest(r, MSPACK_HIP_KIND_SHA1, 0, 0); push_digest(r, MSPACK_HIP_KIND_SHA256, r.out_bytes, 0); }
  }
  return r;
}

// heads keep their tails at i + 1 in local[], behind the chunks, in the caller's relative order; no chunk holds a digest unit
static void case_tails_follow()
{
  Table t = mixed(true);
  BatchPlan p; char err[256];
  REQUIRE(plan(t, K(4, 4096, 4, 0), p, err) == 0);
  const size_t n = t.units.size();
  size_t heads = 0, tails = 0, md5 = 0;
  for (const mspack_hip_unit &u : t.units) { heads += unit_is_wide_head(u); tails += u.kind == MSPACK_HIP_KIND_DIGEST_MORE; md5 += u.kind == MSPACK_HIP_KIND_MD5; }
  REQUIRE(heads == tails && heads > 20 && md5 > 10);
  REQUIRE(p.n_dig == heads + tails + md5 && p.n_md5 == md5 && p.n_sha1 + p.n_sha256 == heads && p.chunks.size() == 4 && p.chunks.back().b == n - p.n_dig);
  for (size_t i = 0; i < n - p.n_dig; i++) REQUIRE(!unit_is_digest(p.local[i]));
  for (size_t i = n - p.n_dig; i < n; i++) {
    REQUIRE(unit_is_digest(p.local[i]) && p.local[i].kind == t.units[p.idx[i]].kind);
    if (i > n - p.n_dig) REQUIRE(p.idx[i - 1] < p.idx[i]);            // the caller's relative order
    if (unit_is_wide_head(p.local[i])) REQUIRE(i + 1 < n && p.local[i + 1].kind == MSPACK_HIP_KIND_DIGEST_MORE && p.idx[i + 1] == p.idx[i] + 1);
    if (p.local[i].kind == MSPACK_HIP_KIND_DIGEST_MORE) REQUIRE(p.local[i].in_off == 0 && p.local[i].out_off == 0 && p.local[i].flags == 0 && unit_is_wide_head(p.local[i - 1]));
    else REQUIRE(p.local[i].out_len == 0 ? p.local[i].out_off == 0 : p.local[i].out_off + p.out_lo == t.units[p.idx[i]].out_off);
  }
}

// order: three consecutive lists of heads -- MD5, SHA-1, SHA-256 --, each longest first; the MD5 list of the mixed table names the
// units the list of the same table without the SHA units names
static void case_three_lists()
{
  Table t = mixed(true), m = mixed(false);
  BatchPlan p, q; char err[256];
  REQUIRE(plan(t, K(4, 4096, 4, 0), p, err) == 0 && plan(m, K(4, 4096, 4, 0), q, err) == 0);
  // (the order array keeps one slot per unit: the tails' stay unused behind the last list)
  const size_t n_tails = p.n_sha1 + p.n_sha256;
  REQUIRE(p.md5_off + p.n_md5 == p.sha1_off && p.sha1_off + p.n_sha1 == p.sha256_off && p.sha256_off + p.n_sha256 + n_tails == p.order.size());
  REQUIRE(p.order.size() == t.units.size() && p.md5_off == t.units.size() - p.n_dig);
  const struct { size_t off, n; unsigned kind; } lists[3] = { { p.md5_off, p.n_md5, MSPACK_HIP_KIND_MD5 }, { p.sha1_off, p.n_sha1, MSPACK_HIP_KIND_SHA1 },
                                                              { p.sha256_off, p.n_sha256, MSPACK_HIP_KIND_SHA256 } };
  std::vector<int> seen(t.units.size(), 0);
  for (const auto &l : lists) {
    REQUIRE(l.n >= 10);
    for (size_t j = 0; j < l.n; j++) {
      const uint32_t x = p.order[l.off + j];
      REQUIRE(x >= t.units.size() - p.n_dig && x < t.units.size() && p.local[x].kind == l.kind && !seen[x]++);
      if (j) REQUIRE(p.local[p.order[l.off + j - 1]].out_len >= p.local[x].out_len);
    }
  }
  // (every head is in a list, no tail is)
  for (size_t i = t.units.size() - p.n_dig; i < t.units.size(); i++) REQUIRE(seen[i] == (p.local[i].kind != MSPACK_HIP_KIND_DIGEST_MORE));
  // the MD5 list: the same ranges in the same order as without the SHA units; chunks, spans and per-kind lists alike
  REQUIRE(q.n_md5 == p.n_md5 && q.n_sha1 == 0 && q.n_sha256 == 0 && q.n_dig == q.n_md5 && q.chunks.size() == p.chunks.size());
  for (size_t j = 0; j < p.n_md5; j++) {
    const mspack_hip_unit &a = p.local[p.order[p.md5_off + j]], &b = q.local[q.order[q.md5_off + j]];
    REQUIRE(a.out_off + p.out_lo == b.out_off + q.out_lo && a.out_len == b.out_len);
  }
  for (size_t c = 0; c < p.chunks.size(); c++) {
    REQUIRE(p.chunks[c].a == q.chunks[c].a && p.chunks[c].b == q.chunks[c].b && p.chunks[c].out_lo == q.chunks[c].out_lo && p.chunks[c].out_hi == q.chunks[c].out_hi);
    for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++) REQUIRE(p.chunks[c].order_off[k] == q.chunks[c].order_off[k] && p.chunks[c].order_n[k] == q.chunks[c].order_n[k]);
  }
  for (size_t j = 0; j < p.md5_off; j++) REQUIRE(p.order[j] == q.order[j]);
  // wide digest units alone: one chunk that holds nothing
  Table o; o.in_bytes = 0; o.out_bytes = 5000;
  push_digest(o, MSPACK_HIP_KIND_SHA256, 100, 4900); push_digest(o, MSPACK_HIP_KIND_SHA1, 200, 10);
  REQUIRE(plan(o, K(4, 8u << 20, 256), p, err) == 0 && p.chunks.size() == 1 && p.chunks[0].b == 0 && p.n_dig == 4 && p.n_md5 == 0 && p.n_sha1 == 1 && p.n_sha256 == 1);
  REQUIRE(p.out_lo == 100 && p.out_hi == 5000 && p.order.size() == 4 && p.sha1_off == 0 && p.order[0] == 2 && p.sha256_off == 1 && p.order[1] == 0);
}

// mspack_hip_decode_batch_multi's cut: never inside a range of any algorithm; a head and its tail land in one shard, next to each other
static void case_shard_cuts()
{
  const size_t n = 12;
  Table t = lzx_row(n, 8192, 65536);
  std::vector<std::vector<uint32_t>> sh; bool asc = false;
  push_digest(t, MSPACK_HIP_KIND_SHA1, 6 * 65536 - 10, 20);             // across the even cut of two shards (units 5 | 6): units 12, 13
  push_digest(t, MSPACK_HIP_KIND_SHA256, 3 * 65536 + 5, 2 * 65536);     // units 3, 4, 5: across the first cut of three: units 14, 15
  push_digest(t, MSPACK_HIP_KIND_MD5, 11 * 65536, 65536);               // the last unit alone: unit 16
  push_digest(t, MSPACK_HIP_KIND_SHA256, 11 * 65536 + 1, 100);          // units 17, 18
  push_digest(t, MSPACK_HIP_KIND_SHA1, 0, 0);                           // empty: units 19, 20
  auto where = [&](uint32_t x) { for (size_t s = 0; s < sh.size(); s++) for (uint32_t y : sh[s]) if (y == x) return (int) s; return -1; };
  for (int k = 2; k <= 3; k++) {
    REQUIRE(plan_shards(t.units.data(), t.units.size(), k, sh, asc) && asc && sh.size() == (size_t) k);
    size_t total = 0; for (auto &v : sh) total += v.size();
    REQUIRE(total == t.units.size());
    for (uint32_t x = 0; x < t.units.size(); x++) REQUIRE(where(x) >= 0);
    REQUIRE(where(5) == where(6) && where(12) == where(5) && where(13) == where(12));
    REQUIRE(where(3) == where(4) && where(4) == where(5) && where(14) == where(3) && where(15) == where(14));
    REQUIRE(where(16) == where(11) && where(17) == where(11) && where(18) == where(17) && where(19) == 0 && where(20) == 0);
    REQUIRE(where(0) == 0 && where(11) == k - 1);
    // every shard is a table the planner takes: heads with their tails at i + 1
    for (auto &v : sh) {
      for (size_t j = 0; j < v.size(); j++) if (unit_is_wide_head(t.units[v[j]])) REQUIRE(j + 1 < v.size() && v[j + 1] == v[j] + 1);
      BatchPlan p; char err[256]; err[0] = 0;
      Table c = t;
      REQUIRE(plan_batch(c.units.data(), v.data(), v.size(), c.in_bytes, c.out_bytes, true, false, false, K(4, 8u << 20, 256), p, err, 256) == 0);
      for (size_t i = 0; i < p.local.size(); i++) if (unit_is_wide_head(p.local[i])) REQUIRE(p.local[i + 1].kind == MSPACK_HIP_KIND_DIGEST_MORE && p.idx[i + 1] == p.idx[i] + 1);
    }
  }
  // outputs that interleave: with wide digest units the batch is not cut at all
  Table r = lzx_row(n, 8192, 65536); for (size_t i = 0; i < n; i++) r.units[i].out_off = (n - 1 - i) * 65536;
  push_digest(r, MSPACK_HIP_KIND_SHA1, 0, 10);
  REQUIRE(!plan_shards(r.units.data(), r.units.size(), 2, sh, asc));
}

static void case_rejections()
{
  struct R { std::function<void(Table &)> make; const char *msg; };
  const R rs[] = {
    { [](Table &c) { c.units.push_back(D(MSPACK_HIP_KIND_SHA1, 0, 10)); }, "unit 4: a wide digest unit is the table's last unit (its MSPACK_HIP_KIND_DIGEST_MORE unit is missing)" },
    { [](Table &c) { c.units.push_back(D(MSPACK_HIP_KIND_SHA256, 0, 10)); }, "unit 4: a wide digest unit is the table's last unit (its MSPACK_HIP_KIND_DIGEST_MORE unit is missing)" },
    { [](Table &c) { c.units[1] = D(MSPACK_HIP_KIND_SHA256, 0, 10); }, "unit 1: a wide digest unit must be followed by an MSPACK_HIP_KIND_DIGEST_MORE unit" },
    { [](Table &c) { c.units.push_back(D(MSPACK_HIP_KIND_SHA1, 0, 10)); c.units.push_back(D(MSPACK_HIP_KIND_MD5, 0, 10)); }, "unit 4: a wide digest unit must be followed by an MSPACK_HIP_KIND_DIGEST_MORE unit" },
    { [](Table &c) { c.units.push_back(D(MSPACK_HIP_KIND_SHA1, 0, 10)); c.units.push_back(D(MSPACK_HIP_KIND_SHA1, 0, 10)); c.units.push_back(MORE()); }, "unit 4: a wide digest unit must be followed by an MSPACK_HIP_KIND_DIGEST_MORE unit" },
    { [](Table &c) { c.units.push_back(MORE()); }, "unit 4: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { c.units[0] = MORE(); }, "unit 0: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { c.units.push_back(D(MSPACK_HIP_KIND_MD5, 0, 10)); c.units.push_back(MORE()); }, "unit 5: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA1, 0, 10); c.units.push_back(MORE()); }, "unit 6: an MSPACK_HIP_KIND_DIGEST_MORE unit without a SHA-1 / SHA-256 unit in front of it" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA256, 0, 10); c.units[5].out_len = 1; }, "unit 5: an MSPACK_HIP_KIND_DIGEST_MORE unit names no bytes (in_len and out_len must be 0)" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA256, 0, 10); c.units[5].in_len = 4; }, "unit 5: an MSPACK_HIP_KIND_DIGEST_MORE unit names no bytes (in_len and out_len must be 0)" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA1, 0, 10); c.units[4].flags = MSPACK_HIP_UF_CRC32; }, "unit 4: a digest unit decodes nothing to take a CRC-32 of" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA256, 0, 10); c.units[4].flags = MSPACK_HIP_UF_CRC32; }, "unit 4: a digest unit decodes nothing to take a CRC-32 of" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA1, 0, 10); c.units[4].in_len = 1; }, "unit 4: a digest unit reads no input (in_len must be 0)" },
    { [](Table &c) { push_digest(c, MSPACK_HIP_KIND_SHA256, 4 * 65536 - 9, 10); }, "unit 4: a digest unit's range leaves the output arena" },
    { [](Table &c) { c.units[2].kind = 9; }, "unit 2: unknown kind 9" },
    { [](Table &c) { c.units[2].kind = 15; }, "unit 2: unknown kind 15" },
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
  push_digest(ok, MSPACK_HIP_KIND_SHA1, 4 * 65536 - 10, 10); push_digest(ok, MSPACK_HIP_KIND_SHA256, 4 * 65536, 0);
  ok.units[4].flags = 0x7Fu;                                            // (every other flag is ignored)
  BatchPlan p; char err[256];
  REQUIRE(plan(ok, K(4, 8u << 20, 256), p, err) == 0 && p.n_dig == 4 && p.n_sha1 == 1 && p.n_sha256 == 1 && p.local[4].flags == 0);
}

int main(int argc, char **argv)
{
  const std::string which = argc > 1 ? argv[1] : "all";
  const struct { const char *name; void (*run)(); } cases[] = {
    { "tails_follow", case_tails_follow }, { "three_lists", case_three_lists }, { "shard_cuts", case_shard_cuts }, { "rejections", case_rejections },
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
