/* host_digest.h -- what the drivers' digest calls share (cabd.c: mspack_cabd_digest, chmd.c: mspack_chmd_digest): the hash in
 * progress on the host, an algorithm's length / feature bit / unit kind, the rule that decides which files are worth a digest
 * unit, and the CHM driver's planner of a chunk's digest units (a pure function: tests/csrc/chm_digest_plan_check.c includes this
 * header alone). */
#ifndef MSPACK_AMD_HOST_DIGEST_H
#define MSPACK_AMD_HOST_DIGEST_H
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "mspack.h"
#include "mspack_hip.h"
#include "md5.h"
#include "sha.h"

/* a digest call's hash in progress: one of the three */
struct digest_sink { int alg; struct mspack_md5 md5; struct mspack_sha sha; };
static inline void sink_init(struct digest_sink *k, int alg)
{
  k->alg = alg;
  if (alg == MSPACK_DIGEST_MD5) mspack_md5_init(&k->md5);
  else if (alg == MSPACK_DIGEST_SHA1) mspack_sha1_init(&k->sha);
  else mspack_sha256_init(&k->sha);
}
static inline void sink_update(struct digest_sink *k, const void *data, size_t n)
{
  if (k->alg == MSPACK_DIGEST_MD5) mspack_md5_update(&k->md5, data, n); else mspack_sha_update(&k->sha, data, n);
}
static inline void sink_final(struct digest_sink *k, unsigned char *digest)
{
  if (k->alg == MSPACK_DIGEST_MD5) mspack_md5_final(&k->md5, digest); else mspack_sha_final(&k->sha, digest);
}
static inline int digest_bytes(int alg) { return alg == MSPACK_DIGEST_MD5 ? 16 : alg == MSPACK_DIGEST_SHA1 ? 20 : alg == MSPACK_DIGEST_SHA256 ? 32 : 0; }
static inline int digest_index(int alg) { return alg == MSPACK_DIGEST_MD5 ? 0 : alg == MSPACK_DIGEST_SHA1 ? 1 : 2; }
/* the feature bit and the unit kind of an algorithm */
static inline unsigned digest_feat(int alg) { return alg == MSPACK_DIGEST_MD5 ? MSPACK_HIP_FEAT_MD5 : alg == MSPACK_DIGEST_SHA1 ? MSPACK_HIP_FEAT_SHA1 : MSPACK_HIP_FEAT_SHA256; }
static inline uint8_t digest_kind(int alg) { return (uint8_t)(alg == MSPACK_DIGEST_MD5 ? MSPACK_HIP_KIND_MD5 : alg == MSPACK_DIGEST_SHA1 ? MSPACK_HIP_KIND_SHA1 : MSPACK_HIP_KIND_SHA256); }

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
extern unsigned mspack_hip_features(void) __attribute__((weak));
static inline double digest_ratio(int alg)
{
  /* (read once per driver, in parts per million; plain C has no dynamic initialiser for a static: the first callers all compute
   * the same value, and it is published and read with atomic accesses, so two decompressors on two threads do not race) */
  static long long ppm[3] = { -1, -1, -1 };
  static const char *const name[3] = { "MSPACK_HIP_MD5_RATIO", "MSPACK_HIP_SHA1_RATIO", "MSPACK_HIP_SHA256_RATIO" };
  static const double dflt[3] = { MD5_RATIO_DEFAULT, SHA1_RATIO_DEFAULT, SHA256_RATIO_DEFAULT };
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
  int alg, algs = 0;
  for (alg = MSPACK_DIGEST_MD5; alg <= MSPACK_DIGEST_SHA256; alg <<= 1)
    if ((asked & alg) && mspack_hip_features && (mspack_hip_features() & digest_feat(alg)) && digest_ratio(alg) > 0.0) algs |= alg;
  return algs;
}

/* ---- CHM: the digest units of one chunk -------------------------------------------------------------------------------------------
 * files[0 .. n_files): the CHM's section-1 files with length > 0, ascending by offset.  The chunk decodes the stream's bytes
 * [chunk_lo, chunk_hi) into its output buffer from 0 on; the stream ends at padded_len.  Per algorithm of `algs` (a mask of
 * MSPACK_DIGEST_*) one unit -- a SHA head with its MSPACK_HIP_KIND_DIGEST_MORE tail behind it -- for every file that lies wholly in
 * [chunk_lo, min(chunk_hi, padded_len)) and is no longer than ratio[digest_index(alg)] x (the bytes of all such files), with
 * out_off = offset - chunk_lo and out_len = length; a file's algorithms next to each other, files in list order.  Files that
 * cross a chunk boundary, reach past padded_len, have length 0 or are above the ratio get none.  Returns the number of units
 * (heads and tails); writes them to units[0 .. cap) as far as they fit (units == NULL: counts only). */
struct chm_digest_file { uint64_t offset, length; };
static inline size_t chm_digest_plan(const struct chm_digest_file *files, size_t n_files, uint64_t chunk_lo, uint64_t chunk_hi,
                                     uint64_t padded_len, int algs, const double ratio[3], mspack_hip_unit *units, size_t cap)
{
  const uint64_t hi = chunk_hi < padded_len ? chunk_hi : padded_len;
  size_t lo_i = 0, hi_i = n_files, i, n = 0;
  double sum = 0.0;
  int pass, alg;
  if (!algs || hi <= chunk_lo) return 0;
  while (lo_i < hi_i) {                                   /* the first file at or behind chunk_lo */
    const size_t mid = lo_i + (hi_i - lo_i) / 2;
    if (files[mid].offset < chunk_lo) lo_i = mid + 1; else hi_i = mid;
  }
  for (pass = 0; pass < 2; pass++)
    for (i = lo_i; i < n_files && files[i].offset < hi; i++) {
      const uint64_t len = files[i].length;
      if (!len || len > hi - files[i].offset || len > 0xFFFFFFFFu) continue;
      if (!pass) { sum += (double) len; continue; }
      for (alg = MSPACK_DIGEST_MD5; alg <= MSPACK_DIGEST_SHA256; alg <<= 1) {
        const size_t need = alg == MSPACK_DIGEST_MD5 ? 1 : 2;
        if (!(algs & alg) || (double) len > ratio[digest_index(alg)] * sum) continue;
        if (units && n + need <= cap) {
          memset(&units[n], 0, need * sizeof(*units));
          units[n].kind = digest_kind(alg);
          units[n].out_off = files[i].offset - chunk_lo; units[n].out_len = (uint32_t) len;
          if (need == 2) units[n + 1].kind = MSPACK_HIP_KIND_DIGEST_MORE;
        }
        n += need;
      }
    }
  return n;
}
#endif
