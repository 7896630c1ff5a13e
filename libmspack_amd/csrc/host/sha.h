/* sha.h -- SHA-1 and SHA-256 (FIPS 180-4) in plain C for the drivers' host side: mspack_cabd_digest() hashes with them whatever the
 * device did not (include/mspack.h).  Written from the standard's description; incremental: init, any number of updates, final.
 * One context serves both: the algorithms share the block size, the padding and the big-endian byte order. */
#ifndef MSPACK_HOST_SHA_H
#define MSPACK_HOST_SHA_H
#include <stddef.h>
#include <stdint.h>

struct mspack_sha {
  uint32_t st[8];               /* H0 .. H4 (SHA-1) or H0 .. H7 (SHA-256) */
  uint64_t bytes;               /* message bytes taken so far */
  unsigned char buf[64];        /* the block that is not full yet: bytes % 64 of it are in use */
  int words;                    /* 5: SHA-1, 8: SHA-256 */
};
void mspack_sha1_init(struct mspack_sha *m);
void mspack_sha256_init(struct mspack_sha *m);
void mspack_sha_update(struct mspack_sha *m, const void *data, size_t n);
void mspack_sha_final(struct mspack_sha *m, unsigned char *digest);      /* 20 bytes (SHA-1) or 32 (SHA-256) */
#endif
