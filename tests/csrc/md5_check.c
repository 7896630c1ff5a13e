/* tests/csrc/md5_check.c -- TEST INFRASTRUCTURE ONLY.  The drivers' plain-C MD5 (libmspack_amd/csrc/host/md5.c) on its own, built with
 * -fsanitize=address,undefined by tests/test_md5_host.py:   md5_check <vectors file>
 * The vectors file holds one line per case, "<length> <32 hex digits>": the digest of the first <length> bytes of the message
 * m[i] = (i * 131 + (i >> 8) * 17 + 7) & 0xFF (recorded from hashlib into tests/golden/md5_vectors.json).  Every case is hashed in
 * one piece and fed in pieces of 1, 7, 64 and 1000 bytes; the RFC 1321 strings are checked first. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "md5.h"

static void hex(const unsigned char d[16], char out[33]) { int i; for (i = 0; i < 16; i++) sprintf(out + 2 * i, "%02x", d[i]); }

static void digest_in_pieces(const unsigned char *m, size_t n, size_t piece, char out[33])
{
  struct mspack_md5 c;
  unsigned char d[16];
  size_t at = 0;
  mspack_md5_init(&c);
  if (!piece) mspack_md5_update(&c, m, n);
  else for (; at < n; at += piece) {
    /* (out of a buffer of exactly the piece's size: a read beyond it is the sanitizer's to see) */
    const size_t k = n - at < piece ? n - at : piece;
    unsigned char *tmp = (unsigned char *) malloc(k ? k : 1);
    memcpy(tmp, m + at, k);
    mspack_md5_update(&c, tmp, k);
    free(tmp);
  }
  mspack_md5_final(&c, d);
  hex(d, out);
}

int main(int argc, char **argv)
{
  static const char *rfc[][2] = {
    { "", "d41d8cd98f00b204e9800998ecf8427e" }, { "a", "0cc175b9c0f1b6a831c399e269772661" }, { "abc", "900150983cd24fb0d6963f7d28e17f72" },
    { "message digest", "f96b697d7cb7938d525a2f31aaf161d0" }, { "abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b" },
    { "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f" },
    { "12345678901234567890123456789012345678901234567890123456789012345678901234567890", "57edf4a22be3c955ac49da2e2107b67a" } };
  static const size_t pieces[] = { 0, 1, 7, 64, 1000 };
  char got[33], want[64];
  unsigned long n;
  size_t i, p, cases = 0;
  FILE *f;
  for (i = 0; i < sizeof(rfc) / sizeof(rfc[0]); i++)
    for (p = 0; p < 5; p++) {
      digest_in_pieces((const unsigned char *) rfc[i][0], strlen(rfc[i][0]), pieces[p], got);
      if (strcmp(got, rfc[i][1])) { printf("MD5_FAIL rfc \"%s\" pieces of %zu: %s\n", rfc[i][0], pieces[p], got); return 1; }
    }
  if (argc < 2 || !(f = fopen(argv[1], "r"))) { printf("MD5_FAIL no vectors file\n"); return 2; }
  while (fscanf(f, "%lu %63s", &n, want) == 2) {
    unsigned char *m = (unsigned char *) malloc(n ? n : 1);
    for (i = 0; i < n; i++) m[i] = (unsigned char)((i * 131u + (i >> 8) * 17u + 7u) & 0xFFu);
    for (p = 0; p < 5; p++) {
      digest_in_pieces(m, n, pieces[p], got);
      if (strcmp(got, want)) { printf("MD5_FAIL length %lu pieces of %zu: %s, not %s\n", n, pieces[p], got, want); return 1; }
    }
    free(m);
    cases++;
  }
  fclose(f);
  printf("MD5_OK %zu lengths\n", cases);
  return 0;
}
