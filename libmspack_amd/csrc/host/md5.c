/* md5.c -- MD5 (RFC 1321), plain C.  The four rounds follow the RFC's tables: round r, step i uses message word
 * (mul[r] * i + add[r]) mod 16, rotation rot[r][i mod 4] and the constant floor(2^32 * |sin(i + 1)|) (spelled out below, so
 * that nothing depends on a math library). */
#include <string.h>
#include "md5.h"

static const uint32_t md5_t[64] = {
  0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
  0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
  0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
  0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
  0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
  0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
  0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
  0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u };
static const unsigned char md5_rot[4][4] = { { 7, 12, 17, 22 }, { 5, 9, 14, 20 }, { 4, 11, 16, 23 }, { 6, 10, 15, 21 } };
static const unsigned char md5_mul[4] = { 1, 5, 3, 7 }, md5_add[4] = { 0, 1, 5, 0 };

static void md5_block(uint32_t st[4], const unsigned char *p)
{
  uint32_t w[16], a = st[0], b = st[1], c = st[2], d = st[3];
  unsigned int i;
  for (i = 0; i < 16; i++)
    w[i] = (uint32_t) p[4 * i] | ((uint32_t) p[4 * i + 1] << 8) | ((uint32_t) p[4 * i + 2] << 16) | ((uint32_t) p[4 * i + 3] << 24);
  for (i = 0; i < 64; i++) {
    const unsigned int r = i >> 4, s = md5_rot[r][i & 3];
    uint32_t f, t;
    switch (r) {
    case 0:  f = d ^ (b & (c ^ d)); break;
    case 1:  f = c ^ (d & (b ^ c)); break;
    case 2:  f = b ^ c ^ d; break;
    default: f = c ^ (b | ~d); break;
    }
    t = a + f + w[(md5_mul[r] * i + md5_add[r]) & 15u] + md5_t[i];
    a = d; d = c; c = b;
    b += (t << s) | (t >> (32u - s));
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}

void mspack_md5_init(struct mspack_md5 *m)
{
  m->st[0] = 0x67452301u; m->st[1] = 0xefcdab89u; m->st[2] = 0x98badcfeu; m->st[3] = 0x10325476u;
  m->bytes = 0;
}

void mspack_md5_update(struct mspack_md5 *m, const void *data, size_t n)
{
  const unsigned char *p = (const unsigned char *) data;
  size_t have = (size_t)(m->bytes & 63u);
  m->bytes += n;
  if (have) {
    size_t take = 64u - have;
    if (take > n) take = n;
    memcpy(m->buf + have, p, take);
    p += take; n -= take; have += take;
    if (have < 64u) return;
    md5_block(m->st, m->buf);
  }
  for (; n >= 64u; p += 64, n -= 64u) md5_block(m->st, p);
  if (n) memcpy(m->buf, p, n);
}

void mspack_md5_final(struct mspack_md5 *m, unsigned char digest[16])
{
  const uint64_t bits = m->bytes << 3;
  size_t have = (size_t)(m->bytes & 63u);
  unsigned int i;
  m->buf[have++] = 0x80u;
  if (have > 56u) { memset(m->buf + have, 0, 64u - have); md5_block(m->st, m->buf); have = 0; }
  memset(m->buf + have, 0, 56u - have);
  for (i = 0; i < 8; i++) m->buf[56 + i] = (unsigned char)(bits >> (8 * i));
  md5_block(m->st, m->buf);
  for (i = 0; i < 16; i++) digest[i] = (unsigned char)(m->st[i >> 2] >> (8 * (i & 3)));
}
