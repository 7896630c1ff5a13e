/* sha512.h -- SHA-384 and SHA-512 (FIPS 180-4) in plain C for the drivers' host side: the digest() calls hash with them whatever the
 * device did not (include/mspack.h).  Written from the standard's description; incremental: init, any number of updates, final.
 * One context serves both: the algorithms share the compression function, the 128-byte block, the padding with its 128-bit length
 * and the big-endian byte order, and differ in the initial state and in how many bytes of the state are the digest. */
#ifndef MSPACK_HOST_SHA512_H
#define MSPACK_HOST_SHA512_H
#include <stddef.h>
#include <stdint.h>

struct mspack_sha512 {
  uint64_t st[8];               /* H0 .. H7 */
  uint64_t bytes;               /* message bytes taken so far (below 2^61: the length's upper 64 bits are 0) */
  unsigned char buf[128];       /* the block that is not full yet: bytes % 128 of it are in use */
  int out;                      /* 48: SHA-384, 64: SHA-512 */
};
void mspack_sha384_init(struct mspack_sha512 *m);
void mspack_sha512_init(struct mspack_sha512 *m);
void mspack_sha512_update(struct mspack_sha512 *m, const void *data, size_t n);
void mspack_sha512_final(struct mspack_sha512 *m, unsigned char *digest);      /* 48 bytes (SHA-384) or 64 (SHA-512) */
#endif
