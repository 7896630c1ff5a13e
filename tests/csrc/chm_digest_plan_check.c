/* tests/csrc/chm_digest_plan_check.c -- TEST INFRASTRUCTURE ONLY: the CHM driver's planner of a chunk's digest units
 * (libmspack_amd/csrc/host/host_digest.h: chm_digest_plan, a pure function of the sorted file table, the chunk's bounds, the
 * algorithm mask and the ratios) asked what units it makes.  Includes that header alone; tests/test_chm_digest.py builds it with
 * -fsanitize=address,undefined and runs one case per call:
 *
 *     chm_digest_plan_check list | CASE
 *
 * "PLAN_OK CASE" and exit 0 when every expectation holds. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "host_digest.h"

#define CHECK(c) do { if (!(c)) { printf("PLAN_FAIL line %d: %s\n", __LINE__, #c); exit(2); } } while (0)
#define LO 131072u                      /* the chunk: [LO, HI) of the stream, decoded to its buffer from 0 on */
#define HI (LO + 262144u)
#define ALL (MSPACK_DIGEST_MD5 | MSPACK_DIGEST_SHA1 | MSPACK_DIGEST_SHA256)

static const double generous[3] = { 1.0, 1.0, 1.0 };
static mspack_hip_unit units[64];

/* the units made for `files` with every slot of `units` poisoned first; also: counting alone gives the same number */
static size_t plan(const struct chm_digest_file *files, size_t n, uint64_t padded, int algs, const double *ratio)
{
  size_t made, counted;
  memset(units, 0xA5, sizeof(units));
  made = chm_digest_plan(files, n, LO, HI, padded, algs, ratio, units, 64);
  counted = chm_digest_plan(files, n, LO, HI, padded, algs, ratio, NULL, 0);
  CHECK(made == counted && made <= 64);
  return made;
}
static int is_head(const mspack_hip_unit *u, int kind, uint64_t off, uint32_t len)
{
  return u->kind == kind && u->out_off == off && u->out_len == len && u->in_len == 0 && u->flags == 0;
}
static int is_tail(const mspack_hip_unit *u) { return u->kind == MSPACK_HIP_KIND_DIGEST_MORE && u->out_len == 0 && u->in_len == 0; }

static void chunk_end(void)
{
  /* a file ending exactly at the chunk's end gets a unit, one a byte longer gets none; so at the chunk's start */
  const struct chm_digest_file f[4] = { { LO - 1, 10 }, { LO, 10 }, { HI - 100, 100 }, { HI - 100, 101 } };
  CHECK(plan(f, 4, 1u << 30, MSPACK_DIGEST_MD5, generous) == 2);
  CHECK(is_head(&units[0], MSPACK_HIP_KIND_MD5, 0, 10) && is_head(&units[1], MSPACK_HIP_KIND_MD5, HI - 100 - LO, 100));
  CHECK(plan(f + 3, 1, 1u << 30, ALL, generous) == 0);
  CHECK(plan(f, 1, 1u << 30, ALL, generous) == 0);
}
static void zero_length(void)
{
  const struct chm_digest_file f[3] = { { LO + 5, 0 }, { LO + 5, 7 }, { HI, 0 } };
  CHECK(plan(f, 3, 1u << 30, MSPACK_DIGEST_MD5, generous) == 1 && is_head(&units[0], MSPACK_HIP_KIND_MD5, 5, 7));
  CHECK(plan(f, 1, 1u << 30, ALL, generous) == 0);
}
static void padded_len(void)
{
  /* the stream ends inside the chunk: a file up to the end gets a unit, files that reach or lie past it get none */
  const uint64_t padded = LO + 65536u;
  const struct chm_digest_file f[4] = { { LO + 65536u - 64, 64 }, { LO + 65536u - 64, 65 }, { LO + 65536u, 16 }, { LO + 100000u, 16 } };
  CHECK(plan(f, 4, padded, MSPACK_DIGEST_MD5, generous) == 1 && is_head(&units[0], MSPACK_HIP_KIND_MD5, 65536u - 64, 64));
  CHECK(plan(f, 4, LO, ALL, generous) == 0 && plan(f, 4, 0, ALL, generous) == 0);        /* a chunk wholly behind the end */
}
static void ratio_rule(void)
{
  /* 1000 bytes of files in all: at 0.10 the file of 100 gets a unit, the file of 101 does not; per algorithm its own ratio */
  const struct chm_digest_file f[4] = { { LO, 100 }, { LO + 100, 101 }, { LO + 300, 700 }, { LO + 1000, 99 } };
  const double r[3] = { 0.10, 0.0995, 1.0 };
  CHECK(plan(f, 4, 1u << 30, MSPACK_DIGEST_MD5, r) == 2);
  CHECK(is_head(&units[0], MSPACK_HIP_KIND_MD5, 0, 100) && is_head(&units[1], MSPACK_HIP_KIND_MD5, 1000, 99));
  CHECK(plan(f, 4, 1u << 30, MSPACK_DIGEST_SHA1, r) == 2 && is_head(&units[0], MSPACK_HIP_KIND_SHA1, 1000, 99) && is_tail(&units[1]));
  CHECK(plan(f, 4, 1u << 30, MSPACK_DIGEST_SHA256, r) == 8);
  /* files outside the chunk do not count towards the sum */
  {
    const struct chm_digest_file g[3] = { { 0, 100000 }, { LO, 100 }, { LO + 100, 101 } };
    CHECK(plan(g, 3, 1u << 30, MSPACK_DIGEST_MD5, r) == 0);
  }
  { const double none[3] = { 0.0, 0.0, 0.0 }; CHECK(plan(f, 4, 1u << 30, ALL, none) == 0); }
}
static void wide_tails(void)
{
  /* per file its algorithms next to each other, every SHA head with its tail behind it; files in list order */
  const struct chm_digest_file f[2] = { { LO + 3, 55 }, { LO + 64, 56 } };
  size_t i;
  CHECK(plan(f, 2, 1u << 30, ALL, generous) == 10);
  for (i = 0; i < 2; i++) {
    const mspack_hip_unit *u = &units[5 * i];
    const uint64_t off = f[i].offset - LO;
    const uint32_t len = (uint32_t) f[i].length;
    CHECK(is_head(&u[0], MSPACK_HIP_KIND_MD5, off, len));
    CHECK(is_head(&u[1], MSPACK_HIP_KIND_SHA1, off, len) && is_tail(&u[2]));
    CHECK(is_head(&u[3], MSPACK_HIP_KIND_SHA256, off, len) && is_tail(&u[4]));
  }
  CHECK(plan(f, 2, 1u << 30, MSPACK_DIGEST_SHA1 | MSPACK_DIGEST_SHA256, generous) == 8 && units[0].kind == MSPACK_HIP_KIND_SHA1);
  CHECK(plan(f, 2, 1u << 30, 0, generous) == 0 && plan(f, 0, 1u << 30, ALL, generous) == 0);
  /* a table with less room than the plan: nothing is written past it, a head never without its tail; the count is the plan's */
  memset(units, 0xA5, sizeof(units));
  CHECK(chm_digest_plan(f, 2, LO, HI, 1u << 30, ALL, generous, units, 4) == 10);
  CHECK(units[0].kind == MSPACK_HIP_KIND_MD5 && units[1].kind == MSPACK_HIP_KIND_SHA1 && is_tail(&units[2]) && units[3].kind == 0xA5 && units[4].kind == 0xA5);
}

static const struct { const char *name; void (*run)(void); } cases[] = {
  { "chunk_end", chunk_end }, { "zero_length", zero_length }, { "padded_len", padded_len }, { "ratio_rule", ratio_rule }, { "wide_tails", wide_tails },
};

int main(int argc, char **argv)
{
  size_t i;
  if (argc == 2 && !strcmp(argv[1], "list")) { for (i = 0; i < sizeof(cases) / sizeof(cases[0]); i++) puts(cases[i].name); return 0; }
  for (i = 0; argc == 2 && i < sizeof(cases) / sizeof(cases[0]); i++)
    if (!strcmp(argv[1], cases[i].name)) { cases[i].run(); printf("PLAN_OK %s\n", cases[i].name); return 0; }
  puts("PLAN_FAIL unknown case");
  return 2;
}
