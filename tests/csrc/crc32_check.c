/* tests/csrc/crc32_check.c -- TEST INFRASTRUCTURE ONLY.  The drivers' plain-C CRC-32 (libmspack_amd/csrc/host/crc32.c / .h) stand-alone,
 * built with -fsanitize=address,undefined by tests/test_crc32_host.py.  Reads no input: prints, for a fixed pseudo-random buffer,
 * "len off crc" for every edge length at sixteen alignments, then "split len crc" where the same bytes were fed in pieces. */
#include <stdio.h>
#include <stdlib.h>
#include "crc32.h"

int main(void)
{
  static const size_t lens[] = { 0, 1, 3, 15, 16, 17, 1023, 1024, 65535, 65536, 65537, 131072 + 5, 196608 - 1 };
  const size_t cap = 196608 + 64;
  unsigned char *buf = (unsigned char *) malloc(cap);
  uint32_t x = 0x12345678u;
  size_t i, k, off;
  if (!buf) return 2;
  for (i = 0; i < cap; i++) { x = x * 1664525u + 1013904223u; buf[i] = (unsigned char)(x >> 24); }
  for (k = 0; k < sizeof(lens) / sizeof(lens[0]); k++)
    for (off = 0; off < 16; off++) {
      /* an exact-size copy: a read past the end is the sanitizer's to see */
      unsigned char *p = (unsigned char *) malloc(lens[k] ? lens[k] : 1);
      uint32_t whole, parts = 0;
      size_t at = 0, step = 1;
      if (!p) return 2;
      for (i = 0; i < lens[k]; i++) p[i] = buf[off + i];
      whole = mspack_crc32_update(0, p, lens[k]);
      printf("%zu %zu %u\n", lens[k], off, (unsigned) whole);
      while (at < lens[k]) {                                   /* pieces of 1, 2, 4, ... 4096, 1, ... bytes, and empty ones between */
        const size_t n = step < lens[k] - at ? step : lens[k] - at;
        parts = mspack_crc32_update(parts, p + at, n);
        parts = mspack_crc32_update(parts, p + at + n, 0);
        at += n; step = step >= 4096 ? 1 : step * 2;
      }
      if (parts != whole || mspack_crc32_step(0, p, lens[k]) != whole) { printf("CRC_FAIL split %zu %zu\n", lens[k], off); return 1; }
      free(p);
    }
  free(buf);
  printf("CRC_OK\n");
  return 0;
}
