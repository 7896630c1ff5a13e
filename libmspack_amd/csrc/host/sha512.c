/* sha512.c -- SHA-384 and SHA-512 (FIPS 180-4), plain C.  The message schedule is kept as sixteen rolling 64-bit words (word t replaces
 * word t - 16), the eight working variables rotate through an array; the round constants are the standard's table 4.2.3. */
#include <string.h>
#include "sha512.h"

static uint64_t rotr64(uint64_t x, unsigned s) { return (x >> s) | (x << (64u - s)); }

static const uint64_t sha512_k[80] = {
  0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
  0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
  0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
  0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
  0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
  0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
  0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
  0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
  0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
  0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
  0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
  0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
  0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
  0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
  0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
  0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
  0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
  0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
  0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
  0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull,
};

static void sha512_block(uint64_t st[8], const unsigned char *p)
{
  uint64_t w[16], v[8], t1, t2;
  unsigned t, i;
  for (t = 0; t < 16; t++) {
    w[t] = 0;
    for (i = 0; i < 8; i++) w[t] = (w[t] << 8) | p[8 * t + i];
  }
  for (i = 0; i < 8; i++) v[i] = st[i];
  for (t = 0; t < 80; t++) {
    if (t >= 16) {
      const uint64_t a = w[(t - 15) & 15u], b = w[(t - 2) & 15u];
      w[t & 15u] += (rotr64(a, 1) ^ rotr64(a, 8) ^ (a >> 7)) + w[(t - 7) & 15u] + (rotr64(b, 19) ^ rotr64(b, 61) ^ (b >> 6));
    }
    t1 = v[7] + (rotr64(v[4], 14) ^ rotr64(v[4], 18) ^ rotr64(v[4], 41)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) + sha512_k[t] + w[t & 15u];
    t2 = (rotr64(v[0], 28) ^ rotr64(v[0], 34) ^ rotr64(v[0], 39)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
    v[7] = v[6]; v[6] = v[5]; v[5] = v[4]; v[4] = v[3] + t1; v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = t1 + t2;
  }
  for (i = 0; i < 8; i++) st[i] += v[i];
}

void mspack_sha384_init(struct mspack_sha512 *m)
{
  memset(m, 0, sizeof(*m));
  m->st[0] = 0xcbbb9d5dc1059ed8ull; m->st[1] = 0x629a292a367cd507ull; m->st[2] = 0x9159015a3070dd17ull; m->st[3] = 0x152fecd8f70e5939ull;
  m->st[4] = 0x67332667ffc00b31ull; m->st[5] = 0x8eb44a8768581511ull; m->st[6] = 0xdb0c2e0d64f98fa7ull; m->st[7] = 0x47b5481dbefa4fa4ull;
  m->out = 48;
}

void mspack_sha512_init(struct mspack_sha512 *m)
{
  memset(m, 0, sizeof(*m));
  m->st[0] = 0x6a09e667f3bcc908ull; m->st[1] = 0xbb67ae8584caa73bull; m->st[2] = 0x3c6ef372fe94f82bull; m->st[3] = 0xa54ff53a5f1d36f1ull;
  m->st[4] = 0x510e527fade682d1ull; m->st[5] = 0x9b05688c2b3e6c1full; m->st[6] = 0x1f83d9abfb41bd6bull; m->st[7] = 0x5be0cd19137e2179ull;
  m->out = 64;
}

void mspack_sha512_update(struct mspack_sha512 *m, const void *data, size_t n)
{
  const unsigned char *p = (const unsigned char *) data;
  size_t have = (size_t)(m->bytes & 127u);
  m->bytes += n;
  if (have) {
    size_t take = 128u - have;
    if (take > n) take = n;
    memcpy(m->buf + have, p, take);
    p += take; n -= take; have += take;
    if (have < 128u) return;
    sha512_block(m->st, m->buf);
  }
  for (; n >= 128u; p += 128, n -= 128u) sha512_block(m->st, p);
  if (n) memcpy(m->buf, p, n);
}

void mspack_sha512_final(struct mspack_sha512 *m, unsigned char *digest)
{
  const uint64_t bits = m->bytes << 3;
  size_t have = (size_t)(m->bytes & 127u);
  int i;
  m->buf[have++] = 0x80u;
  if (have > 112u) { memset(m->buf + have, 0, 128u - have); sha512_block(m->st, m->buf); have = 0; }
  memset(m->buf + have, 0, 120u - have);                  /* (with the upper 64 bits of the 128-bit length) */
  for (i = 0; i < 8; i++) m->buf[120 + i] = (unsigned char)(bits >> (8 * (7 - i)));
  sha512_block(m->st, m->buf);
  for (i = 0; i < m->out; i++) digest[i] = (unsigned char)(m->st[i >> 3] >> (8 * (7 - (i & 7))));
}
