/* md5.h -- MD5 (RFC 1321) in plain C for the drivers' host side: mspack_cabd_md5() hashes with it whatever the device did not
 * (include/mspack.h).  Written from the RFC's description; incremental: init, any number of updates, final. */
#ifndef MSPACK_HOST_MD5_H
#define MSPACK_HOST_MD5_H
#include <stddef.h>
#include <stdint.h>

struct mspack_md5 {
  uint32_t st[4];               /* A, B, C, D */
  uint64_t bytes;               /* message bytes taken so far */
  unsigned char buf[64];        /* the block that is not full yet: bytes % 64 of it are in use */
};
void mspack_md5_init(struct mspack_md5 *m);
void mspack_md5_update(struct mspack_md5 *m, const void *data, size_t n);
void mspack_md5_final(struct mspack_md5 *m, unsigned char digest[16]);
#endif
