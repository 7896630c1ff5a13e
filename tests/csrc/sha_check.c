/* tests/csrc/sha_check.c -- TEST INFRASTRUCTURE ONLY.  The drivers' plain-C SHA-1 / SHA-256 (libmspack_amd/csrc/host/sha.c) on their own,
 * built with -fsanitize=address,undefined by tests/test_sha_host.py:   sha_check <vectors file>
 * The vectors file holds one line per case, "<algorithm: 1 | 256> <length> <hex digest> [<split>]": the digest of the first <length>
 * bytes of the message m[i] = (i * 131 + (i >> 8) * 17 + 7) & 0xFF, written by the test from hashlib.  Without <split> the case is
 * hashed in one piece and fed in pieces of 1, 7, 64 and 1000 bytes; with it in two updates cut at byte <split>.  The FIPS 180-4
 * example messages are checked first. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sha.h"

static void hex(const unsigned char *d, int n, char *out) { int i; for (i = 0; i < n; i++) sprintf(out + 2 * i, "%02x", d[i]); }

/* (every update out of a buffer of exactly the piece's size: a read beyond it is the sanitizer's to see) */
static void feed(struct mspack_sha *c, const unsigned char *m, size_t k)
{
  unsigned char *tmp = (unsigned char *) malloc(k ? k : 1);
  memcpy(tmp, m, k);
  mspack_sha_update(c, tmp, k);
  free(tmp);
}

static void digest_in_pieces(int alg, const unsigned char *m, size_t n, size_t piece, long split, char *out)
{
  struct mspack_sha c;
  unsigned char d[32];
  size_t at = 0;
  if (alg == 1) mspack_sha1_init(&c); else mspack_sha256_init(&c);
  if (split >= 0) { feed(&c, m, (size_t) split); feed(&c, m + split, n - (size_t) split); }
  else if (!piece) feed(&c, m, n);
  else for (; at < n; at += piece) feed(&c, m + at, n - at < piece ? n - at : piece);
  mspack_sha_final(&c, d);
  hex(d, alg == 1 ? 20 : 32, out);
}

int main(int argc, char **argv)
{
  static const char *msg[4] = { "", "abc", "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq",
    "abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu" };
  static const char *want1[4] = { "da39a3ee5e6b4b0d3255bfef95601890afd80709", "a9993e364706816aba3e25717850c26c9cd0d89d",
    "84983e441c3bd26ebaae4aa1f95129e5e54670f1", "a49b2446a02c645bf419f995b67091253a04a259" };
  static const char *want256[4] = { "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad",
    "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1",
    "cf5b16a778af8380036ce59e7b0492370b249b11e8f07a51afac45037afee9d1" };
  static const size_t pieces[] = { 0, 1, 7, 64, 1000 };
  char got[65], want[80], line[256];
  size_t i, p, cases = 0;
  FILE *f;
  for (i = 0; i < 4; i++)
    for (p = 0; p < 5; p++) {
      digest_in_pieces(1, (const unsigned char *) msg[i], strlen(msg[i]), pieces[p], -1, got);
      if (strcmp(got, want1[i])) { printf("SHA_FAIL SHA-1 fips %zu pieces of %zu: %s\n", i, pieces[p], got); return 1; }
      digest_in_pieces(256, (const unsigned char *) msg[i], strlen(msg[i]), pieces[p], -1, got);
      if (strcmp(got, want256[i])) { printf("SHA_FAIL SHA-256 fips %zu pieces of %zu: %s\n", i, pieces[p], got); return 1; }
    }
  if (argc < 2 || !(f = fopen(argv[1], "r"))) { printf("SHA_FAIL no vectors file\n"); return 2; }
  while (fgets(line, sizeof(line), f)) {
    int alg; unsigned long n; long split = -1;
    unsigned char *m;
    const int got_n = sscanf(line, "%d %lu %79s %ld", &alg, &n, want, &split);
    if (got_n < 3 || (alg != 1 && alg != 256) || (got_n == 4 && (split < 0 || (unsigned long) split > n))) { printf("SHA_FAIL bad line: %s", line); return 2; }
    m = (unsigned char *) malloc(n ? n : 1);
    for (i = 0; i < n; i++) m[i] = (unsigned char)((i * 131u + (i >> 8) * 17u + 7u) & 0xFFu);
    for (p = 0; p < (split >= 0 ? 1u : 5u); p++) {
      digest_in_pieces(alg, m, n, pieces[p], split, got);
      if (strcmp(got, want)) { printf("SHA_FAIL SHA-%d length %lu pieces of %zu split %ld: %s, not %s\n", alg, n, pieces[p], split, got, want); free(m); fclose(f); return 1; }
    }
    free(m);
    cases++;
  }
  fclose(f);
  printf("SHA_OK %zu cases\n", cases);
  return 0;
}
