/* host_digest.h -- everything the drivers' digest calls share (cabd.c: mspack_cabd_digest, chmd.c: mspack_chmd_digest): the hash in
 * progress on the host; an algorithm's length / feature bit / unit kind and back; the rule that decides which files are worth a
 * digest unit; the emitter of one file's units (heads and MSPACK_HIP_KIND_DIGEST_MORE tails); the table of the digests a batch took,
 * its harvest from the batch's results and its lookup; the frame of a digest() call and its counters; and the CHM driver's planner
 * of a chunk's units.  All of it static inline over plain structs, the table and the planners pure functions:
 * tests/csrc/digest_table_check.c and tests/csrc/chm_digest_plan_check.c include this header alone. */
#ifndef MSPACK_AMD_HOST_DIGEST_H
#define MSPACK_AMD_HOST_DIGEST_H
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "mspack.h"
#include "mspack_hip.h"
#include "md5.h"
#include "sha.h"
#include "sha512.h"
#include "crc32.h"

/* CRC-32 (zlib's) rides in the drivers' masks of algorithms as a bit of its own, INTERNAL to the drivers: no MSPACK_DIGEST_* value (8 is
 * MSPACK_ERR_ARGS in the digest() calls and in *_PARAM_HIP_DIGESTS); mspack_cabd_crc32() / mspack_chmd_crc32() and *_PARAM_HIP_CRC32 set it.
 * Its unit is MSPACK_HIP_KIND_CRC32 -- any length: the ratio rule does not apply --, its kept record holds the checksum in d[0 .. 4),
 * little-endian, as the unit's result.out_len lies there */
#define DIGEST_ALG_CRC32 8

/* the algorithms of the drivers' masks, in the emitter's order, and how many of them there are: digest_index(alg) counts through them */
#define DIGEST_ALGS 5
static const int digest_alg_list[DIGEST_ALGS] = { MSPACK_DIGEST_MD5, MSPACK_DIGEST_SHA1, MSPACK_DIGEST_SHA256, MSPACK_DIGEST_SHA384, MSPACK_DIGEST_SHA512 };
static inline int digest_is_sha512(int alg) { return alg == MSPACK_DIGEST_SHA384 || alg == MSPACK_DIGEST_SHA512; }

/* a digest call's hash in progress: one of them */
struct digest_sink { int alg; struct mspack_md5 md5; struct mspack_sha sha; struct mspack_sha512 sha512; uint32_t crc; };
static inline void sink_init(struct digest_sink *k, int alg)
{
  k->alg = alg; k->crc = 0;
  if (alg == DIGEST_ALG_CRC32) return;
  if (alg == MSPACK_DIGEST_MD5) mspack_md5_init(&k->md5);
  else if (alg == MSPACK_DIGEST_SHA1) mspack_sha1_init(&k->sha);
  else if (alg == MSPACK_DIGEST_SHA384) mspack_sha384_init(&k->sha512);
  else if (alg == MSPACK_DIGEST_SHA512) mspack_sha512_init(&k->sha512);
  else mspack_sha256_init(&k->sha);
}
static inline void sink_update(struct digest_sink *k, const void *data, size_t n)
{
  if (k->alg == DIGEST_ALG_CRC32) { k->crc = mspack_crc32_step(k->crc, data, n); return; }
  if (k->alg == MSPACK_DIGEST_MD5) mspack_md5_update(&k->md5, data, n);
  else if (digest_is_sha512(k->alg)) mspack_sha512_update(&k->sha512, data, n);
  else mspack_sha_update(&k->sha, data, n);
}
static inline void sink_final(struct digest_sink *k, unsigned char *digest)
{
  if (k->alg == MSPACK_DIGEST_MD5) mspack_md5_final(&k->md5, digest);
  else if (digest_is_sha512(k->alg)) mspack_sha512_final(&k->sha512, digest);
  else mspack_sha_final(&k->sha, digest);
}
static inline int digest_bytes(int alg)
{
  return alg == MSPACK_DIGEST_MD5 ? 16 : alg == MSPACK_DIGEST_SHA1 ? 20 : alg == MSPACK_DIGEST_SHA256 ? 32 : alg == MSPACK_DIGEST_SHA384 ? 48 : alg == MSPACK_DIGEST_SHA512 ? 64 : 0;
}
static inline int digest_index(int alg) { return alg == MSPACK_DIGEST_MD5 ? 0 : alg == MSPACK_DIGEST_SHA1 ? 1 : alg == MSPACK_DIGEST_SHA384 ? 3 : alg == MSPACK_DIGEST_SHA512 ? 4 : 2; }
/* the feature bit and the unit kind of an algorithm */
static inline unsigned digest_feat(int alg)
{
  return alg == MSPACK_DIGEST_MD5 ? MSPACK_HIP_FEAT_MD5 : alg == MSPACK_DIGEST_SHA1 ? MSPACK_HIP_FEAT_SHA1 : alg == MSPACK_DIGEST_SHA384 ? MSPACK_HIP_FEAT_SHA384 :
         alg == MSPACK_DIGEST_SHA512 ? MSPACK_HIP_FEAT_SHA512 : MSPACK_HIP_FEAT_SHA256;
}
static inline uint8_t digest_kind(int alg)
{
  return (uint8_t)(alg == MSPACK_DIGEST_MD5 ? MSPACK_HIP_KIND_MD5 : alg == MSPACK_DIGEST_SHA1 ? MSPACK_HIP_KIND_SHA1 : alg == MSPACK_DIGEST_SHA384 ? MSPACK_HIP_KIND_SHA384 :
                   alg == MSPACK_DIGEST_SHA512 ? MSPACK_HIP_KIND_SHA512 : MSPACK_HIP_KIND_SHA256);
}
/* ... and back: the algorithm of a head's kind; 0 for every other kind (a tail's too) */
static inline int digest_alg_of_kind(unsigned kind)
{
  return kind == MSPACK_HIP_KIND_MD5 ? MSPACK_DIGEST_MD5 : kind == MSPACK_HIP_KIND_SHA1 ? MSPACK_DIGEST_SHA1 : kind == MSPACK_HIP_KIND_SHA256 ? MSPACK_DIGEST_SHA256 :
         kind == MSPACK_HIP_KIND_SHA384 ? MSPACK_DIGEST_SHA384 : kind == MSPACK_HIP_KIND_SHA512 ? MSPACK_DIGEST_SHA512 : 0;
}
/* a result has sixteen bytes to spare (mspack_hip.h): MD5 is one unit, a wide digest a head and its tails -- 2 units for SHA-1 and
 * SHA-256, 3 for SHA-384, 4 for SHA-512 */
static inline size_t digest_units(int alg) { const int nd = digest_bytes(alg); return nd > 16 ? (size_t)(nd + 15) / 16u : 1; }
/* the units one file needs at most for the algorithms of the mask `algs` */
static inline size_t digest_units_per_file(int algs)
{
  size_t n = 0; int a;
  for (a = 0; a < DIGEST_ALGS; a++) if (algs & digest_alg_list[a]) n += digest_units(digest_alg_list[a]);
  if (algs & DIGEST_ALG_CRC32) n++;
  return n;
}

/* Which files get a digest unit.  The device hashes one range per LANE (MD5 is one chain per message), so
 * one lane is much slower than a host core and the pass takes as long as its longest range; the host hashes everything at its
 * one-core rate.  A file longer than ratio x (all digest-range bytes of the batch), ratio = lane rate / host rate, would hold the
 * batch longer than the host takes for everything: it gets no unit and is hashed on the host.  The compiled default comes from the
 * two rates measured on an MI355X box -- one lane 67 MB/s, md5.c on one core 637 MB/s, three runs: 0.1051, 0.1052, 0.1055
 * (profiles/md5_digest.txt) --; MSPACK_HIP_MD5_RATIO overrides it (read once;
 * 0: no file gets a unit). */
#define MD5_RATIO_DEFAULT 0.10
/* SHA-1 and SHA-256 are chains too, so the same rule holds with their own rates, measured the same way on an MI355X box, three runs
 * each (profiles/sha_digest.txt): SHA-1 one lane 31.5 to 39.2 MB/s, csrc/host/sha.c on one core 617 MB/s --
 * 0.0582, 0.0511, 0.0636 --; SHA-256 one lane 15.5 to 19.0 MB/s, one core 413 to 416 MB/s -- 0.0373, 0.0460, 0.0409.  The
 * compiled defaults are the quotients rounded down; MSPACK_HIP_SHA1_RATIO / MSPACK_HIP_SHA256_RATIO override them in the same way. */
#define SHA1_RATIO_DEFAULT 0.05
#define SHA256_RATIO_DEFAULT 0.04
/* SHA-384 and SHA-512 share one kernel and one host function, so one ratio (MSPACK_HIP_SHA512_RATIO) serves both.  Measured the same
 * way on an MI355X box, three runs per algorithm (profiles/sha512_digest.txt; tools/sha512_digest_bench.py rates
 * 8 3): one lane 11.0 to 14.7 MB/s, csrc/host/sha512.c on one core 539 to 553 MB/s -- SHA-384 0.0234, 0.0199, 0.0257; SHA-512 0.0236,
 * 0.0272, 0.0239; mean 0.0240.  The compiled default is that quotient rounded down. */
#define SHA512_RATIO_DEFAULT 0.02
extern unsigned mspack_hip_features(void) __attribute__((weak));
static inline double digest_ratio(int alg)
{
  /* (read once per driver, in parts per million; plain C has no dynamic initialiser for a static: the first callers all compute
   * the same value, and it is published and read with atomic accesses, so two decompressors on two threads do not race) */
  static long long ppm[DIGEST_ALGS] = { -1, -1, -1, -1, -1 };
  static const char *const name[DIGEST_ALGS] = { "MSPACK_HIP_MD5_RATIO", "MSPACK_HIP_SHA1_RATIO", "MSPACK_HIP_SHA256_RATIO", "MSPACK_HIP_SHA512_RATIO", "MSPACK_HIP_SHA512_RATIO" };
  static const double dflt[DIGEST_ALGS] = { MD5_RATIO_DEFAULT, SHA1_RATIO_DEFAULT, SHA256_RATIO_DEFAULT, SHA512_RATIO_DEFAULT, SHA512_RATIO_DEFAULT };
  const int a = digest_index(alg);
  long long v = __atomic_load_n(&ppm[a], __ATOMIC_RELAXED);
  if (v < 0) {
    const char *e = getenv(name[a]);
    const double r = e ? atof(e) : dflt[a];
    v = r <= 0.0 ? 0 : (r >= 1e6 ? 1000000000000ll : (long long)(r * 1e6 + 0.5));
    __atomic_store_n(&ppm[a], v, __ATOMIC_RELAXED);
  }
  return (double) v * 1e-6;
}
/* the algorithms of `asked` (a mask of MSPACK_DIGEST_*) a batch may carry units for: the provider can (one without
 * mspack_hip_features cannot) and the ratio is above 0 */
static inline int digest_device_algs(int asked)
{
  int a, alg, algs = 0;
  for (a = 0; a < DIGEST_ALGS && (alg = digest_alg_list[a]) != 0; a++)
    if ((asked & alg) && mspack_hip_features && (mspack_hip_features() & digest_feat(alg)) && digest_ratio(alg) > 0.0) algs |= alg;
  /* (CRC-32 range units: no ratio -- the device takes them at any length) */
  if ((asked & DIGEST_ALG_CRC32) && mspack_hip_features && (mspack_hip_features() & MSPACK_HIP_FEAT_CRC32_RANGES)) algs |= DIGEST_ALG_CRC32;
  return algs;
}
static inline void digest_ratios(double ratio[DIGEST_ALGS]) { int a; for (a = 0; a < DIGEST_ALGS; a++) ratio[a] = digest_ratio(digest_alg_list[a]); }

/* ---- the digest units of one file --------------------------------------------------------------------------------------------------
 * The file's bytes lie at [out_off, out_off + len) of the batch's output arena; `sum`: the bytes of all files of the batch that may
 * get units.  Per algorithm of `algs` whose ratio[digest_index(alg)] x sum is not below len: the head (kind, out_off, out_len, every
 * other field 0) and, for a wide digest, its tails (the kind alone) behind it, MD5 / SHA-1 / SHA-256 / SHA-384 / SHA-512 in that order.
 * Written to units[n ..) as far as they fit below `cap`, a head never without all its tails (units == NULL: counts only).  Returns
 * the units the file needs, fitting or not.  (ratio[] is read at the indices of the algorithms of `algs` only: a caller that asks
 * for the first three may pass three.) */
static inline size_t digest_emit_file(uint64_t out_off, uint32_t len, double sum, int algs, const double *ratio,
                                      mspack_hip_unit *units, size_t n, size_t cap)
{
  size_t made = 0, j; int a;
  for (a = 0; a < DIGEST_ALGS; a++) {
    const int alg = digest_alg_list[a];
    const size_t need = digest_units(alg), at = n + made;
    if (!(algs & alg) || (double) len > ratio[a] * sum) continue;
    if (units && at + need <= cap) {
      memset(&units[at], 0, need * sizeof(*units));
      units[at].kind = digest_kind(alg);
      units[at].out_off = out_off; units[at].out_len = len;
      for (j = 1; j < need; j++) units[at + j].kind = MSPACK_HIP_KIND_DIGEST_MORE;
    }
    made += need;
  }
  if (algs & DIGEST_ALG_CRC32) {                          /* behind the hashes (the table's order), whatever the file's length */
    if (units && n + made + 1 <= cap) {
      memset(&units[n + made], 0, sizeof(*units));
      units[n + made].kind = MSPACK_HIP_KIND_CRC32;
      units[n + made].out_off = out_off; units[n + made].out_len = len;
    }
    made++;
  }
  return made;
}

/* ---- the digests a batch took, kept ------------------------------------------------------------------------------------------------
 * One record per head whose result -- and whose tail's -- came back MSPACK_ERR_OK, ascending by (offset, length, alg); d: the
 * algorithm's 16, 20, 32, 48 or 64 bytes, zeros behind them.  The owner allocates e[]; sorts: how often a harvest found its records out
 * of order and sorted (the planners emit ascending: normally never); next: the record behind the last one found. */
struct digest_kept { uint64_t offset; uint32_t length; int alg; unsigned char d[64]; };
struct digest_table { struct digest_kept *e; size_t n, next; unsigned sorts; };
static inline int digest_kept_order(const void *pa, const void *pb)
{
  const struct digest_kept *a = (const struct digest_kept *) pa, *b = (const struct digest_kept *) pb;
  if (a->offset != b->offset) return a->offset < b->offset ? -1 : 1;
  if (a->length != b->length) return a->length < b->length ? -1 : 1;
  return (a->alg > b->alg) - (a->alg < b->alg);
}
/* units[0 .. n) -- digest heads and tails -- and their results res[0 .. n) join the table, which has room for n more records; a
 * record's offset is its head's out_off - out_base + base (the owner's origin instead of the output arena's).  Bytes 0 to 15 of a digest
 * are the head's result from out_len on, bytes 16 k .. of a wide one those of the unit k places behind it (mspack_hip.h): a wide
 * head whose tails are not all there and MSPACK_ERR_OK is dropped. */
static inline void digest_table_harvest(struct digest_table *t, const mspack_hip_unit *units, const mspack_hip_result *res, size_t n,
                                        uint64_t out_base, uint64_t base)
{
  size_t j, k; int ascending = 1;
  for (j = 0; j < n; j++) {
    const int alg = units[j].kind == MSPACK_HIP_KIND_CRC32 ? DIGEST_ALG_CRC32 : digest_alg_of_kind(units[j].kind);
    const size_t tails = alg && alg != DIGEST_ALG_CRC32 ? digest_units(alg) - 1 : 0, nd = (size_t) digest_bytes(alg);
    struct digest_kept *e = &t->e[t->n];
    if (!alg || res[j].err != MSPACK_ERR_OK) continue;            /* (a tail is taken with its head) */
    for (k = 1; k <= tails; k++) if (j + k >= n || units[j + k].kind != MSPACK_HIP_KIND_DIGEST_MORE || res[j + k].err != MSPACK_ERR_OK) break;
    if (k <= tails) continue;
    e->offset = units[j].out_off - out_base + base; e->length = units[j].out_len; e->alg = alg;
    memset(e->d, 0, sizeof(e->d));
    memcpy(e->d, &res[j].out_len, 16);
    for (k = 1; k <= tails; k++) memcpy(e->d + 16 * k, &res[j + k].out_len, nd - 16 * k < 16 ? nd - 16 * k : 16);
    if (t->n && digest_kept_order(e - 1, e) > 0) ascending = 0;
    t->n++;
  }
  if (!ascending) { qsort(t->e, t->n, sizeof(*t->e), digest_kept_order); t->sorts++; }
}
/* the digest of algorithm alg that was taken of the bytes [offset, offset + length), or NULL.  Files are mostly asked for in list
 * order, one algorithm at a time: the record behind the last hit is looked at first, then a binary search */
static inline const unsigned char *digest_table_find(struct digest_table *t, uint64_t offset, uint64_t length, int alg)
{
  size_t lo = 0, hi = t->n;
  struct digest_kept want;
  if (length > 0xFFFFFFFFu) return NULL;
  want.offset = offset; want.length = (uint32_t) length; want.alg = alg;
  if (t->next < t->n && !digest_kept_order(&want, &t->e[t->next])) return t->e[t->next++].d;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    const int o = digest_kept_order(&want, &t->e[mid]);
    if (o == 0) { t->next = mid + 1; return t->e[mid].d; }
    if (o > 0) lo = mid + 1; else hi = mid;
  }
  return NULL;
}

/* ---- the frame of a digest() call (mspack.h) ---------------------------------------------------------------------------------------
 * the arguments: a buffer that can hold the algorithm's bytes is zeroed, whatever else is wrong; MSPACK_ERR_ARGS for no file, an
 * unknown algorithm, no buffer or one too small */
static inline int digest_call_args(const void *file, int alg, unsigned char *digest, size_t digest_cap)
{
  const size_t nd = (size_t) digest_bytes(alg);
  if (digest && nd && digest_cap >= nd) memset(digest, 0, nd); else return MSPACK_ERR_ARGS;
  return file ? MSPACK_ERR_OK : MSPACK_ERR_ARGS;
}
/* a call that succeeded: the digest the batch took of the file (`kept`) or else the one hashed on the way, and the driver's counter
 * of either -- counts[digest_index(alg)][0: from the device, 1: on the host], over all decompressors of the process */
static inline void digest_call_done(struct digest_sink *k, const unsigned char *kept, unsigned char *digest, unsigned long long counts[DIGEST_ALGS][2])
{
  if (kept) memcpy(digest, kept, (size_t) digest_bytes(k->alg)); else sink_final(k, digest);
  __atomic_fetch_add(&counts[digest_index(k->alg)][kept ? 0 : 1], 1ull, __ATOMIC_RELAXED);
}
/* the frame of a crc32() call: the same with a checksum for a digest -- counts[0: from the device, 1: on the host] */
static inline int crc32_call_args(const void *file, unsigned int *crc)
{
  if (!crc) return MSPACK_ERR_ARGS;
  *crc = 0;
  return file ? MSPACK_ERR_OK : MSPACK_ERR_ARGS;
}
static inline void crc32_call_done(const struct digest_sink *k, const unsigned char *kept, unsigned int *crc, unsigned long long counts[2])
{
  if (kept) *crc = (unsigned int) kept[0] | ((unsigned int) kept[1] << 8) | ((unsigned int) kept[2] << 16) | ((unsigned int) kept[3] << 24);
  else *crc = k->crc;
  __atomic_fetch_add(&counts[kept ? 0 : 1], 1ull, __ATOMIC_RELAXED);
}
static inline void crc32_counts_get(unsigned long long counts[2], unsigned long long out[2], int reset)
{
  int i;
  for (i = 0; i < 2; i++) {
    if (out) out[i] = __atomic_load_n(&counts[i], __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(&counts[i], 0ull, __ATOMIC_RELAXED);
  }
}
/* the *_digest_counts calls: the pair of one algorithm (an unknown one: zeros), optionally reset */
static inline void digest_counts_get(unsigned long long counts[DIGEST_ALGS][2], int alg, unsigned long long out[2], int reset)
{
  int i;
  if (!digest_bytes(alg)) { if (out) out[0] = out[1] = 0; return; }
  for (i = 0; i < 2; i++) {
    if (out) out[i] = __atomic_load_n(&counts[digest_index(alg)][i], __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(&counts[digest_index(alg)][i], 0ull, __ATOMIC_RELAXED);
  }
}

/* ---- CHM: the digest units of one chunk -------------------------------------------------------------------------------------------
 * files[0 .. n_files): the CHM's section-1 files with length > 0, ascending by offset.  The chunk decodes the stream's bytes
 * [chunk_lo, chunk_hi) into its output buffer from 0 on; the stream ends at padded_len.  Per algorithm of `algs` (a mask of
 * MSPACK_DIGEST_*) one unit -- a SHA head with its MSPACK_HIP_KIND_DIGEST_MORE tails behind it -- for every file that lies wholly in
 * [chunk_lo, min(chunk_hi, padded_len)) and is no longer than ratio[digest_index(alg)] x (the bytes of all such files), with
 * out_off = offset - chunk_lo and out_len = length (digest_emit_file); a file's algorithms next to each other, files in list order.  Files that
 * cross a chunk boundary, reach past padded_len, have length 0 or are above the ratio get none.  Returns the number of units
 * (heads and tails); writes them to units[0 .. cap) as far as they fit (units == NULL: counts only). */
struct chm_digest_file { uint64_t offset, length; };
static inline size_t chm_digest_plan(const struct chm_digest_file *files, size_t n_files, uint64_t chunk_lo, uint64_t chunk_hi,
                                     uint64_t padded_len, int algs, const double *ratio, mspack_hip_unit *units, size_t cap)
{
  const uint64_t hi = chunk_hi < padded_len ? chunk_hi : padded_len;
  size_t lo_i = 0, hi_i = n_files, i, n = 0;
  double sum = 0.0;
  int pass;
  if (!algs || hi <= chunk_lo) return 0;
  while (lo_i < hi_i) {                                   /* the first file at or behind chunk_lo */
    const size_t mid = lo_i + (hi_i - lo_i) / 2;
    if (files[mid].offset < chunk_lo) lo_i = mid + 1; else hi_i = mid;
  }
  for (pass = 0; pass < 2; pass++)
    for (i = lo_i; i < n_files && files[i].offset < hi; i++) {
      const uint64_t len = files[i].length;
      if (!len || len > hi - files[i].offset || len > 0xFFFFFFFFu) continue;
      if (!pass) sum += (double) len;
      else n += digest_emit_file(files[i].offset - chunk_lo, (uint32_t) len, sum, algs, ratio, units, n, cap);
    }
  return n;
}
#endif
