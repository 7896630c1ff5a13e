/* tests/csrc/sha512_check.c -- TEST INFRASTRUCTURE ONLY.  The drivers' plain-C SHA-384 / SHA-512 (libmspack_amd/csrc/host/sha512.c) on
 * their own, built with -fsanitize=address,undefined by tests/test_sha512_host.py:   sha512_check <vectors file>
 * The vectors file holds one line per case, "<algorithm: 384 | 512> <length> <hex digest>": the digest of the first <length> bytes of
 * the message m[i] = (i * 131 + (i >> 8) * 17 + 7) & 0xFF, written by the test from hashlib.  Every case is hashed in one piece, in
 * pieces of 1, 7, 128 and 1000 bytes, and in uneven pieces of 1, 2, 3, ... bytes.  The FIPS 180-4 example messages are checked
 * first. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sha512.h"

static void hex(const unsigned char *d, int n, char *out) { int i; for (i = 0; i < n; i++) sprintf(out + 2 * i, "%02x", d[i]); }

/* (every update out of a buffer of exactly the piece's size: a read beyond it is the sanitizer's to see) */
static void feed(struct mspack_sha512 *c, const unsigned char *m, size_t k)
{
  unsigned char *tmp = (unsigned char *) malloc(k ? k : 1);
  memcpy(tmp, m, k);
  mspack_sha512_update(c, tmp, k);
  free(tmp);
}

/* piece 0: one update; (size_t) -1: pieces of 1, 2, 3, ... bytes; else pieces of that size */
static void digest_in_pieces(int alg, const unsigned char *m, size_t n, size_t piece, char *out)
{
  struct mspack_sha512 c;
  unsigned char *d = (unsigned char *) malloc(alg / 8);     /* (exactly the digest's room) */
  size_t at = 0, step = 1;
  if (alg == 384) mspack_sha384_init(&c); else mspack_sha512_init(&c);
  if (!piece) feed(&c, m, n);
  else if (piece == (size_t) -1) for (; at < n; at += step, step++) feed(&c, m + at, n - at < step ? n - at : step);
  else for (; at < n; at += piece) feed(&c, m + at, n - at < piece ? n - at : piece);
  mspack_sha512_final(&c, d);
  hex(d, alg / 8, out);
  free(d);
}

int main(int argc, char **argv)
{
  static const char *msg[3] = { "", "abc",
    "abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu" };
  static const char *want384[3] = {
    "38b060a751ac96384cd9327eb1b1e36a21fdb71114be07434c0cc7bf63f6e1da274edebfe76f65fbd51ad2f14898b95b",
    "cb00753f45a35e8bb5a03d699ac65007272c32ab0eded1631a8b605a43ff5bed8086072ba1e7cc2358baeca134c825a7",
    "09330c33f71147e83d192fc782cd1b4753111b173b3b05d22fa08086e3b0f712fcc7c71a557e2db966c3e9fa91746039" };
  static const char *want512[3] = {
    "cf83e1357eefb8bdf1542850d66d8007d620e4050b5715dc83f4a921d36ce9ce47d0d13c5d85f2b0ff8318d2877eec2f63b931bd47417a81a538327af927da3e",
    "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
    "8e959b75dae313da8cf4f72814fc143f8f7779c6eb9f7fa17299aeadb6889018501d289e4900f7e4331b99dec4b5433ac7d329eeb6dd26545e96e55b874be909" };
  static const size_t pieces[] = { 0, 1, 7, 128, 1000, (size_t) -1 };
  char got[129], want[160], line[256];
  size_t i, p, cases = 0;
  FILE *f;
  for (i = 0; i < 3; i++)
    for (p = 0; p < 6; p++) {
      digest_in_pieces(384, (const unsigned char *) msg[i], strlen(msg[i]), pieces[p], got);
      if (strcmp(got, want384[i])) { printf("SHA512_FAIL SHA-384 fips %zu pieces %zu: %s\n", i, p, got); return 1; }
      digest_in_pieces(512, (const unsigned char *) msg[i], strlen(msg[i]), pieces[p], got);
      if (strcmp(got, want512[i])) { printf("SHA512_FAIL SHA-512 fips %zu pieces %zu: %s\n", i, p, got); return 1; }
    }
  if (argc < 2 || !(f = fopen(argv[1], "r"))) { printf("SHA512_FAIL no vectors file\n"); return 2; }
  while (fgets(line, sizeof(line), f)) {
    int alg; unsigned long n;
    unsigned char *m;
    if (sscanf(line, "%d %lu %159s", &alg, &n, want) != 3 || (alg != 384 && alg != 512)) { printf("SHA512_FAIL bad line: %s", line); return 2; }
    m = (unsigned char *) malloc(n ? n : 1);
    for (i = 0; i < n; i++) m[i] = (unsigned char)((i * 131u + (i >> 8) * 17u + 7u) & 0xFFu);
    for (p = 0; p < 6; p++) {
      digest_in_pieces(alg, m, n, pieces[p], got);
      if (strcmp(got, want)) { printf("SHA512_FAIL SHA-%d length %lu pieces %zu: %s, not %s\n", alg, n, p, got, want); free(m); fclose(f); return 1; }
    }
    free(m);
    cases++;
  }
  fclose(f);
  printf("SHA512_OK %zu cases\n", cases);
  return 0;
}
