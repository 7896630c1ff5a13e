/* sha.c -- SHA-1 and SHA-256 (FIPS 180-4), plain C.  The message schedule is kept as sixteen rolling words (word t replaces word
 * t - 16); SHA-256's constants are the first 32 bits of the fractional parts of the cube roots of the first 64 primes, spelled
 * out below so that nothing depends on a math library. */
#include <string.h>
#include "sha.h"

static const uint32_t sha256_k[64] = {
  0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
  0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
  0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
  0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
  0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
  0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
  0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
  0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u };

static uint32_t rotr(uint32_t x, unsigned int s) { return (x >> s) | (x << (32u - s)); }
static void load_be(uint32_t w[16], const unsigned char *p)
{
  unsigned int i;
  for (i = 0; i < 16; i++)
    w[i] = ((uint32_t) p[4 * i] << 24) | ((uint32_t) p[4 * i + 1] << 16) | ((uint32_t) p[4 * i + 2] << 8) | (uint32_t) p[4 * i + 3];
}

static void sha256_block(uint32_t st[8], const unsigned char *p)
{
  uint32_t w[16], v[8];
  unsigned int t;
  load_be(w, p);
  memcpy(v, st, sizeof(v));
  for (t = 0; t < 64; t++) {
    uint32_t t1, t2;
    if (t >= 16) {
      const uint32_t x = w[(t - 15) & 15u], y = w[(t - 2) & 15u];
      w[t & 15u] += (rotr(y, 17) ^ rotr(y, 19) ^ (y >> 10)) + w[(t - 7) & 15u] + (rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3));
    }
    t1 = v[7] + (rotr(v[4], 6) ^ rotr(v[4], 11) ^ rotr(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) + sha256_k[t] + w[t & 15u];
    t2 = (rotr(v[0], 2) ^ rotr(v[0], 13) ^ rotr(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
    v[7] = v[6]; v[6] = v[5]; v[5] = v[4]; v[4] = v[3] + t1; v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = t1 + t2;
  }
  for (t = 0; t < 8; t++) st[t] += v[t];
}

static void sha1_block(uint32_t st[8], const unsigned char *p)
{
  uint32_t w[16], a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
  unsigned int t;
  load_be(w, p);
  for (t = 0; t < 80; t++) {
    uint32_t f, k, tmp;
    if (t >= 16) w[t & 15u] = rotr(w[(t - 3) & 15u] ^ w[(t - 8) & 15u] ^ w[(t - 14) & 15u] ^ w[t & 15u], 31);
    if (t < 20)      { f = (b & c) ^ (~b & d);          k = 0x5a827999u; }
    else if (t < 40) { f = b ^ c ^ d;                   k = 0x6ed9eba1u; }
    else if (t < 60) { f = (b & c) ^ (b & d) ^ (c & d); k = 0x8f1bbcdcu; }
    else             { f = b ^ c ^ d;                   k = 0xca62c1d6u; }
    tmp = rotr(a, 27) + f + e + k + w[t & 15u];
    e = d; d = c; c = rotr(b, 2); b = a; a = tmp;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e;
}

void mspack_sha1_init(struct mspack_sha *m)
{
  memset(m, 0, sizeof(*m));
  m->st[0] = 0x67452301u; m->st[1] = 0xefcdab89u; m->st[2] = 0x98badcfeu; m->st[3] = 0x10325476u; m->st[4] = 0xc3d2e1f0u;
  m->words = 5;
}

void mspack_sha256_init(struct mspack_sha *m)
{
  memset(m, 0, sizeof(*m));
  m->st[0] = 0x6a09e667u; m->st[1] = 0xbb67ae85u; m->st[2] = 0x3c6ef372u; m->st[3] = 0xa54ff53au;
  m->st[4] = 0x510e527fu; m->st[5] = 0x9b05688cu; m->st[6] = 0x1f83d9abu; m->st[7] = 0x5be0cd19u;
  m->words = 8;
}

static void sha_block(struct mspack_sha *m, const unsigned char *p)
{
  if (m->words == 5) sha1_block(m->st, p); else sha256_block(m->st, p);
}

void mspack_sha_update(struct mspack_sha *m, const void *data, size_t n)
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
    sha_block(m, m->buf);
  }
  for (; n >= 64u; p += 64, n -= 64u) sha_block(m, p);
  if (n) memcpy(m->buf, p, n);
}

void mspack_sha_final(struct mspack_sha *m, unsigned char *digest)
{
  const uint64_t bits = m->bytes << 3;
  size_t have = (size_t)(m->bytes & 63u);
  int i;
  m->buf[have++] = 0x80u;
  if (have > 56u) { memset(m->buf + have, 0, 64u - have); sha_block(m, m->buf); have = 0; }
  memset(m->buf + have, 0, 56u - have);
  for (i = 0; i < 8; i++) m->buf[56 + i] = (unsigned char)(bits >> (8 * (7 - i)));
  sha_block(m, m->buf);
  for (i = 0; i < 4 * m->words; i++) digest[i] = (unsigned char)(m->st[i >> 2] >> (8 * (3 - (i & 3))));
}
