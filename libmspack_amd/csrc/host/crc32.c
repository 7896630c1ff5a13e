/* crc32.c -- the exported form of crc32.h's table-driven CRC-32 (zlib's convention) */
#include "crc32.h"

uint32_t mspack_crc32_update(uint32_t crc, const void *data, size_t n) { return mspack_crc32_step(crc, data, n); }
