// tests/hostcheck/plan_md5_check.cpp -- TEST INFRASTRUCTURE ONLY.  The host path's chunk planner (libmspack_amd/csrc/hip/host_plan.hpp)
// and digest units (MSPACK_HIP_KIND_MD5): this file includes that header alone and is built with -fsanitize=address,undefined by
// tests/test_host_plan_md5.py.   usage: plan_md5_check <case> | list | dump
// `dump` prints the plans of the unit tables of plan_check.cpp's nine cases (no digest unit in them), one line per plan: the test
// compares them with tests/golden/plan_parent.txt, recorded from the planner as it was before digest units existed.
#include "host_plan.hpp"
#include <string.h>
#include <stdlib.h>
#include <string>
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
struct Table { std::vector<mspack_hip_unit> units; size_t in_bytes = 0, out_bytes = 0; };
static Table lzx_row(size_t n, uint32_t in_len, uint32_t out_len)
{
  Table c;
  for (size_t i = 0; i < n; i++) c.units.push_back(U(MSPACK_HIP_KIND_LZX, i * in_len, in_len, (uint64_t) i * out_len, out_len));
  c.in_bytes = n * in_len; c.out_bytes = (uint64_t) n * out_len;
  return c;
}
static int plan(Table &t, const PlanKnobs &kn, BatchPlan &p, char *err, bool to_host = true, bool dev_out = false, bool per_unit_back = false)
{
  p = BatchPlan(); err[0] = 0;
  return plan_batch(t.units.data(), nullptr, t.units.size(), t.in_bytes, t.out_bytes, to_host, dev_out, per_unit_back, kn, p, err, 256);
}

// ---- the plans of tables without digest units: one line each ----
static void dump_one(const char *name, Table t, const PlanKnobs &kn, bool to_host = true, bool dev_out = false, bool per_unit_back = false)
{
  BatchPlan p; char err[256];
  const int rc = plan(t, kn, p, err, to_host, dev_out, per_unit_back);
  printf("%s rc=%d", name, rc);
  if (rc) { printf(" err=\"%s\"\n", err); return; }
  printf(" span=%llu,%llu,%llu,%llu,%llu fr=%zu,%zu crc=%zu mono=%d qtm=%d idx=", (unsigned long long) p.in_lo, (unsigned long long) p.in_hi,
         (unsigned long long) p.out_lo, (unsigned long long) p.out_hi, (unsigned long long) p.in_sum, p.n_frames, p.n_rec_slots, p.n_crc, (int) p.monotone, (int) p.has_qtm);
  for (uint32_t x : p.idx) printf("%u,", x);
  printf(" local=");
  for (const mspack_hip_unit &u : p.local) printf("%llu:%llu:%u:%u:%u:%u,", (unsigned long long) u.in_off, (unsigned long long) u.out_off, u.frame_base, u.ref_len, u.in_chunk, u.flags);
  printf(" order=");
  for (uint32_t x : p.order) printf("%u,", x);
  printf(" chunks=");
  for (const Chunk &c : p.chunks) {
    printf("[%zu,%zu|%llu,%llu,%llu,%llu|%zu,%zu|%zu,%zu,%llu|%d|", c.a, c.b, (unsigned long long) c.in_lo, (unsigned long long) c.in_hi, (unsigned long long) c.out_lo,
           (unsigned long long) c.out_hi, c.fm_lo, c.fm_n, c.crc_off, c.crc_n, (unsigned long long) c.crc_max, (int) c.has_ftab);
    for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++) printf("%zu+%zu,", c.order_off[k], c.order_n[k]);
    printf("]");
  }
  printf("\n");
}
static Table mixed_table()
{
  Table c;
  const uint32_t FT = MSPACK_HIP_UF_FRAME_TABLE;
  uint64_t in = 8, out = 0, tab = 32768;
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
    add(MSPACK_HIP_KIND_LZX, 65536, FT, 7, true);
    add(MSPACK_HIP_KIND_LZX, 65536, 0, 0, false);
    add(MSPACK_HIP_KIND_MSZIP, 65536, FT, 0, true);
    add(MSPACK_HIP_KIND_MSZIP, 65536, FT | MSPACK_HIP_UF_MSZIP_REPAIR, 0, false);
    add(MSPACK_HIP_KIND_QUANTUM, 40000, MSPACK_HIP_UF_QTM_MARKS, 4, true);
    add(MSPACK_HIP_KIND_LZX_DELTA, 40000, 0, 5000, false);
    add(MSPACK_HIP_KIND_LZSS, 3000, 0, 0, false);
    add(MSPACK_HIP_KIND_XORSUM, 0, 0, 0, false);
  }
  c.in_bytes = tab; c.out_bytes = out;
  return c;
}
static void dump_all()
{
  const PlanKnobs D = K(4, 8u << 20, 256);
  { Table c; c.units.push_back(U(MSPACK_HIP_KIND_LZX, 48, 1000, 4096, 65536)); c.in_bytes = 2048; c.out_bytes = 4096 + 65536;
    dump_one("one_unit", c, D); dump_one("one_unit_dev", c, D, false, true); c.units[0].in_off = 40; dump_one("one_unit_40", c, D); }
  { Table c = lzx_row(64, 8192, 65536);
    for (int s = 0; s <= 4; s++) dump_one(("shapes_" + std::to_string(s)).c_str(), c, K(4, 4096, 4, s));
    dump_one("shapes_w", c, K(4, 4096, 4, 0, { 4, 3, 2, 1 })); dump_one("shapes_host", c, K(4, 4096, 4), true); dump_one("shapes_dev", c, K(4, 4096, 4), false, true); }
  { Table c = lzx_row(10, 8192, 65536);
    for (int i = 0; i < 3; i++) c.units.push_back(U(MSPACK_HIP_KIND_XORSUM, i * 8192, 8192, 0, 0));
    dump_one("unit_cap_a", c, K(8, 1, 4, 0)); dump_one("unit_cap_b", c, K(8, 8192 * 3, 1, 0)); dump_one("unit_cap_c", c, K(2, 1, 1, 0)); }
  dump_one("mixed_kinds", mixed_table(), K(4, 1, 2, 0));
  { Table c; const size_t n = 64; const uint64_t tabs = n * 1024; c.in_bytes = tabs + 16 * n; c.out_bytes = n * 65536;
    for (size_t i = 0; i < n; i++) c.units.push_back(U(MSPACK_HIP_KIND_LZX, i * 1024, (uint32_t)(c.in_bytes - i * 1024), i * 65536, 65536, MSPACK_HIP_UF_FRAME_TABLE, 0, (uint32_t)((tabs + 16 * i) >> 2)));
    dump_one("chm_style", c, K(4, 4096, 4, 0)); }
  { Table c; for (int i = 0; i < 5; i++) c.units.push_back(U(MSPACK_HIP_KIND_XORSUM, 16 + i * 100, 100, 0, 0)); c.in_bytes = 1024; c.out_bytes = 0;
    dump_one("xorsum_only", c, K(4, 1, 1, 0)); }
  { Table c = lzx_row(16, 8192, 65536); for (size_t i = 0; i < 16; i++) c.units[i].out_off = (15 - i) * 65536;
    dump_one("not_monotone_a", c, K(4, 4096, 4, 0), true, false, true); dump_one("not_monotone_b", c, K(4, 4096, 4, 0));
    Table d = lzx_row(16, 8192, 65536); dump_one("not_monotone_c", d, K(4, 4096, 4, 0), true, false, true); dump_one("not_monotone_d", d, K(4, 4096, 4, 0)); }
  { Table c; for (size_t j = 0; j < 10; j++) { const size_t i = 9 - j; c.units.push_back(U(MSPACK_HIP_KIND_LZX, i * 4096, 4096, i * 65536, (uint32_t)(1000 * (10 - i)))); }
    c.in_bytes = 10 * 4096; c.out_bytes = 10 * 65536;
    c.units[7].flags |= MSPACK_HIP_UF_CRC32; c.units[2].flags |= MSPACK_HIP_UF_CRC32; c.units[5].flags |= MSPACK_HIP_UF_CRC32; c.units[5].kind = 0;
    dump_one("crc_lists_a", c, D); dump_one("crc_lists_b", c, K(2, 1, 4, 0)); }
  { const std::function<void(Table &)> rs[] = {
      [](Table &c) { c.units[1].kind = 9; }, [](Table &c) { c.units[0] = U(MSPACK_HIP_KIND_XORSUM, 0, 100, 0, 4); },
      [](Table &c) { c.units[0] = U(MSPACK_HIP_KIND_XORSUM, 0, 100, 0, 0, MSPACK_HIP_UF_CRC32); }, [](Table &c) { c.units[3].in_len = 8193; },
      [](Table &c) { c.units[3].out_len = 65537; }, [](Table &c) { c.units[0].kind = MSPACK_HIP_KIND_LZSS; c.units[0].out_off = 100; },
      [](Table &c) { c.units[1].flags = MSPACK_HIP_UF_FRAME_TABLE; c.units[1].in_chunk = (4 * 8192 - 4) >> 2; },
      [](Table &c) { c.units[0] = U(MSPACK_HIP_KIND_QUANTUM, 0, 8192, 2, 1000, MSPACK_HIP_UF_QTM_MARKS, 2, 64); } };
    int k = 0;
    for (const auto &r : rs) { Table c = lzx_row(4, 8192, 65536); r(c); dump_one(("rejection_" + std::to_string(k++)).c_str(), c, D); } }
}

#ifndef PLAN_PARENT
static mspack_hip_unit D5(uint64_t out_off, uint32_t out_len) { return U(MSPACK_HIP_KIND_MD5, 0xABCDEF, 0, out_off, out_len); }

// digest units carry no weight in the cutting: the chunks of a table are the same with and without them
static void case_no_weight()
{
  Table a = lzx_row(64, 8192, 65536), b = a;
  for (int i = 0; i < 500; i++) b.units.insert(b.units.begin() + (i % 60), D5((uint64_t) i * 4000, 70000));
  b.units.push_back(D5(0, 64 * 65536));
  for (const PlanKnobs &kn : { K(4, 4096, 4, 0), K(4, 4096, 4, 1), K(8, 1, 1, 2), K(4, 8u << 20, 256) }) {
    BatchPlan pa, pb; char err[256];
    REQUIRE(plan(a, kn, pa, err) == 0 && plan(b, kn, pb, err) == 0);
    REQUIRE(pb.n_md5 == 501 && pa.n_md5 == 0 && pa.chunks.size() == pb.chunks.size());
    REQUIRE(pb.local.size() == 64 + 501 && pb.order.size() == pb.local.size() && pb.chunks.back().b == 64);
    for (size_t ci = 0; ci < pa.chunks.size(); ci++) {
      const Chunk &x = pa.chunks[ci], &y = pb.chunks[ci];
      REQUIRE(x.a == y.a && x.b == y.b && x.in_lo == y.in_lo && x.in_hi == y.in_hi && x.out_lo == y.out_lo && x.out_hi == y.out_hi);
      for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++) REQUIRE(x.order_n[k] == y.order_n[k]);
    }
    for (size_t i = 0; i < 64; i++) REQUIRE(pb.local[i].kind == MSPACK_HIP_KIND_LZX && pb.local[i].in_off == pa.local[i].in_off && pb.local[i].out_off == pa.local[i].out_off);
    REQUIRE(pa.in_lo == pb.in_lo && pa.in_hi == pb.in_hi && pa.out_lo == pb.out_lo && pa.out_hi == pb.out_hi && pa.in_sum == pb.in_sum);
  }
}

// their list: all of them, once, longest first; their offsets rebased like everybody's; the caller's index kept
static void case_longest_first()
{
  Table t = lzx_row(8, 8192, 65536);
  for (auto &u : t.units) u.out_off += 1 << 20;                       // (the decoded span begins at 1 MiB)
  t.out_bytes += 1 << 20;
  const uint32_t lens[] = { 5, 70000, 0, 64, 70000, 1, 300000, 63 };
  for (int i = 0; i < 8; i++) t.units.insert(t.units.begin() + i, D5((1 << 20) + 1000 * i + 3, lens[i]));      // (caller's indices 0, 2, 4 ...)
  BatchPlan p; char err[256];
  REQUIRE(plan(t, K(4, 4096, 2, 0), p, err) == 0);
  REQUIRE(p.n_md5 == 8 && p.md5_off + 8 == p.order.size() && p.out_lo == (1u << 20));
  uint32_t prev = 0xFFFFFFFFu; std::vector<int> seen(16, 0);
  for (size_t j = 0; j < 8; j++) {
    const uint32_t x = p.order[p.md5_off + j];
    REQUIRE(x >= 8 && x < 16 && !seen[x]++);
    const mspack_hip_unit &l = p.local[x], &g = t.units[p.idx[x]];
    REQUIRE(l.kind == MSPACK_HIP_KIND_MD5 && g.kind == MSPACK_HIP_KIND_MD5 && l.out_len == g.out_len && l.out_len <= prev);
    if (l.out_len) REQUIRE(l.out_off + p.out_lo == g.out_off);
    REQUIRE(l.in_len == 0 && l.flags == 0);
    prev = l.out_len;
  }
  REQUIRE(p.local[p.order[p.md5_off]].out_len == 300000);
  // equal lengths keep the caller's order
  REQUIRE(p.idx[p.order[p.md5_off + 1]] < p.idx[p.order[p.md5_off + 2]]);
  // the dev_out flavour addresses the caller's buffer as it is
  REQUIRE(plan(t, K(4, 4096, 2, 0), p, err, false, true) == 0 && p.out_lo == 0);
  for (size_t x = 8; x < 16; x++) if (p.local[x].out_len) REQUIRE(p.local[x].out_off == t.units[p.idx[x]].out_off);
}

// digest units alone: one chunk that holds nothing, nothing read
static void case_md5_only()
{
  Table t; t.in_bytes = 0; t.out_bytes = 5000;
  t.units.push_back(D5(100, 4900)); t.units.push_back(D5(0, 0)); t.units.push_back(D5(5000, 0));
  BatchPlan p; char err[256];
  REQUIRE(plan(t, K(4, 1, 1, 0), p, err) == 0);
  REQUIRE(p.chunks.size() == 1 && p.chunks[0].a == 0 && p.chunks[0].b == 0 && p.n_md5 == 3 && p.in_lo == 0 && p.in_hi == 0);
  REQUIRE(p.chunks[0].in_lo == p.chunks[0].in_hi && p.chunks[0].out_lo == p.chunks[0].out_hi);
  REQUIRE(p.out_lo == 100 && p.out_hi == 5000 && p.md5_off == 0 && p.order[0] == 0);
  for (unsigned k = 1; k <= MSPACK_HIP_KIND_XORSUM; k++) REQUIRE(p.chunks[0].order_n[k] == 0);
}

// mspack_hip_decode_batch_multi's cut: a cut that would fall inside a digest range is moved; a digest unit goes where its range lies
static void case_shard_cuts()
{
  const size_t n = 12;
  Table plain = lzx_row(n, 8192, 65536);
  std::vector<std::vector<uint32_t>> sh; bool asc = false;
  REQUIRE(plan_shards(plain.units.data(), n, 2, sh, asc) && asc && sh.size() == 2 && sh[0].size() == 6 && sh[1].size() == 6);
  REQUIRE(plan_shards(plain.units.data(), n, 3, sh, asc) && sh[0].size() == 4 && sh[1].size() == 4 && sh[2].size() == 4);
  Table t = plain;
  t.units.push_back(D5(6 * 65536 - 10, 20));                          // across the even cut of two shards (units 5 | 6) -> unit 12
  t.units.push_back(D5(3 * 65536 + 5, 2 * 65536));                    // units 3, 4, 5: across the first cut of three (3 | 4)      -> unit 13
  t.units.push_back(D5(11 * 65536, 65536));                           // the last unit alone                                        -> unit 14
  t.units.push_back(D5(0, 0));                                        // empty                                                      -> unit 15
  auto where = [&](uint32_t x) { for (size_t s = 0; s < sh.size(); s++) for (uint32_t y : sh[s]) if (y == x) return (int) s; return -1; };
  for (int k = 2; k <= 3; k++) {
    REQUIRE(plan_shards(t.units.data(), t.units.size(), k, sh, asc) && asc && sh.size() == (size_t) k);
    size_t total = 0; for (auto &v : sh) total += v.size();
    REQUIRE(total == t.units.size());                                 // everybody once
    for (uint32_t x = 0; x < 16; x++) REQUIRE(where(x) >= 0);
    REQUIRE(where(5) == where(6) && where(12) == where(5));           // the barred cut was moved, the unit went along
    REQUIRE(where(3) == where(4) && where(4) == where(5) && where(13) == where(3));
    REQUIRE(where(14) == where(11) && where(15) == 0);
    REQUIRE(where(0) == 0 && where(11) == k - 1);                     // (still cut: the last shard has work)
    for (auto &v : sh) { uint64_t prev = 0; for (uint32_t x : v) if (t.units[x].kind != MSPACK_HIP_KIND_MD5) { REQUIRE(t.units[x].in_off >= prev); prev = t.units[x].in_off; } }
  }
  // one range over everything: no cut is left -- one shard holds all
  t.units.push_back(D5(1, 12 * 65536 - 2));
  REQUIRE(plan_shards(t.units.data(), t.units.size(), 3, sh, asc) && sh[0].size() == t.units.size() && sh[1].empty() && sh[2].empty());
  // outputs that interleave: with digest units the batch is not cut at all
  Table r = plain; for (size_t i = 0; i < n; i++) r.units[i].out_off = (n - 1 - i) * 65536;
  REQUIRE(plan_shards(r.units.data(), n, 2, sh, asc) && !asc);
  r.units.push_back(D5(0, 10));
  REQUIRE(!plan_shards(r.units.data(), r.units.size(), 2, sh, asc));
}

static void case_rejections()
{
  struct R { std::function<void(Table &)> make; const char *msg; };
  const R rs[] = {
    { [](Table &c) { c.units[2] = D5(4 * 65536 - 9, 10); }, "unit 2: a digest unit's range leaves the output arena" },
    { [](Table &c) { c.units[2] = D5(4 * 65536 + 1, 0); }, "unit 2: a digest unit's range leaves the output arena" },
    { [](Table &c) { c.units[2] = D5(0, 10); c.units[2].in_len = 1; }, "unit 2: a digest unit reads no input (in_len must be 0)" },
    { [](Table &c) { c.units[2] = D5(0, 10); c.units[2].flags = MSPACK_HIP_UF_CRC32; }, "unit 2: a digest unit decodes nothing to take a CRC-32 of" },
    { [](Table &c) { c.units[2].kind = 9; }, "unit 2: unknown kind 9" },
  };
  for (const R &r : rs) {
    Table c = lzx_row(4, 8192, 65536);
    r.make(c);
    BatchPlan p; char err[256];
    if (plan(c, K(4, 8u << 20, 256), p, err) != -1 || strcmp(err, r.msg) != 0) { printf("PLAN_FAIL rejection \"%s\": got \"%s\"\n", r.msg, err); exit(1); }
    for (size_t i = 0; i < c.units.size(); i++) REQUIRE(c.units[i].frame_base == 0xDEADu);
  }
  Table ok = lzx_row(4, 8192, 65536);
  ok.units[2] = D5(4 * 65536 - 10, 10); ok.units.push_back(D5(4 * 65536, 0));
  ok.units[2].flags = 0x7Fu;                                            // (every other flag is ignored)
  BatchPlan p; char err[256];
  REQUIRE(plan(ok, K(4, 8u << 20, 256), p, err) == 0 && p.n_md5 == 2);
}
#endif

int main(int argc, char **argv)
{
  const std::string which = argc > 1 ? argv[1] : "all";
  if (which == "dump") { dump_all(); return 0; }
#ifndef PLAN_PARENT
  const struct { const char *name; void (*run)(); } cases[] = {
    { "no_weight", case_no_weight }, { "longest_first", case_longest_first }, { "md5_only", case_md5_only }, { "shard_cuts", case_shard_cuts }, { "rejections", case_rejections },
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
#else
  return 2;
#endif
}
