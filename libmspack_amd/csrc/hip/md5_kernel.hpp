// md5_kernel.hpp -- MSPACK_HIP_KIND_MD5: the MD5 (RFC 1321) of a byte range of the output arena, computed where the bytes lie.
//
// MD5 is one chain per message: block k's compression starts from the state block k - 1 left, and inside a block every one of the
// 64 steps needs the step before it.  Nothing of one range can be spread over lanes (CRC-32, crc32_kernel.hpp, is linear and can),
// so the work split is ONE LANE PER RANGE, 64 ranges per wavefront: a lane keeps the state (4 words) and the sixteen message words
// of its current block in VGPRs, the 64 steps are unrolled with their constants as literals, a rotation is one v_alignbit_b32, F,
// G, H and I are one v_bitop3_b32 each (gfx950's three-operand bit operation: what the compiler makes of the bit-selects below,
// where older targets take v_bfi_b32).  No table, no LDS, no atomics, no cross-lane traffic, no wait on another wave: a lane runs
// `blocks` iterations of a counted loop and leaves; lanes of one wave have different counts, the loop runs to the longest and the
// lanes that are through are masked -- which is why the host hands the units over longest first (host_plan.hpp).
//
// Loading.  A range begins at any byte.  Block offsets are multiples of 64, so a lane's alignment is the same for all its blocks:
//   * p % 16 == 0: four aligned 16-byte rows per block;
//   * p % 4 == 0:  sixteen aligned dwords;
//   * otherwise:   seventeen aligned dwords, neighbours funnelled together with v_alignbyte_b32.  Both end dwords of the seventeen
//                  hold at least one byte of the block, so no dword wholly outside the range is touched.
// That is the path of the whole blocks.  The last one or two blocks (the message's tail, 0x80, zeros, the 64-bit bit length) are
// built word by word: an aligned dword is loaded only if it holds a byte of the range, bytes of it beyond the range are masked
// before the pad goes in, and the words behind the message are made in registers.
// The next block's words are loaded before the current block is compressed (sixteen more VGPRs), so the loads' latency hides
// behind the ~300 dependent VALU operations of a block.
#pragma once
#include "wave_common.hpp"
#include "digest_load.hpp"

__device__ __forceinline__ u32 md5_rotl(u32 x, u32 s) { return __builtin_amdgcn_alignbit(x, x, 32u - s); }
// bit-selects: where the mask bit is set take a's bit, else b's
__device__ __forceinline__ u32 md5_sel(u32 mask, u32 a, u32 b) { return (mask & a) | (~mask & b); }

#define MD5_F(b, c, d) md5_sel((b), (c), (d))
#define MD5_G(b, c, d) md5_sel((d), (b), (c))
#define MD5_H(b, c, d) ((b) ^ (c) ^ (d))
#define MD5_I(b, c, d) ((c) ^ ((b) | ~(d)))
#define MD5_STEP(f, a, b, c, d, x, t, s) do { (a) += f((b), (c), (d)) + (x) + (t); (a) = md5_rotl((a), (s)) + (b); } while (0)

// one block: st[4] += compress(st, w[16])
__device__ __forceinline__ void md5_block(u32 st[4], const u32 w[16])
{
  u32 a = st[0], b = st[1], c = st[2], d = st[3];
  MD5_STEP(MD5_F, a, b, c, d, w[ 0], 0xd76aa478u,  7); MD5_STEP(MD5_F, d, a, b, c, w[ 1], 0xe8c7b756u, 12);
  MD5_STEP(MD5_F, c, d, a, b, w[ 2], 0x242070dbu, 17); MD5_STEP(MD5_F, b, c, d, a, w[ 3], 0xc1bdceeeu, 22);
  MD5_STEP(MD5_F, a, b, c, d, w[ 4], 0xf57c0fafu,  7); MD5_STEP(MD5_F, d, a, b, c, w[ 5], 0x4787c62au, 12);
  MD5_STEP(MD5_F, c, d, a, b, w[ 6], 0xa8304613u, 17); MD5_STEP(MD5_F, b, c, d, a, w[ 7], 0xfd469501u, 22);
  MD5_STEP(MD5_F, a, b, c, d, w[ 8], 0x698098d8u,  7); MD5_STEP(MD5_F, d, a, b, c, w[ 9], 0x8b44f7afu, 12);
  MD5_STEP(MD5_F, c, d, a, b, w[10], 0xffff5bb1u, 17); MD5_STEP(MD5_F, b, c, d, a, w[11], 0x895cd7beu, 22);
  MD5_STEP(MD5_F, a, b, c, d, w[12], 0x6b901122u,  7); MD5_STEP(MD5_F, d, a, b, c, w[13], 0xfd987193u, 12);
  MD5_STEP(MD5_F, c, d, a, b, w[14], 0xa679438eu, 17); MD5_STEP(MD5_F, b, c, d, a, w[15], 0x49b40821u, 22);

  MD5_STEP(MD5_G, a, b, c, d, w[ 1], 0xf61e2562u,  5); MD5_STEP(MD5_G, d, a, b, c, w[ 6], 0xc040b340u,  9);
  MD5_STEP(MD5_G, c, d, a, b, w[11], 0x265e5a51u, 14); MD5_STEP(MD5_G, b, c, d, a, w[ 0], 0xe9b6c7aau, 20);
  MD5_STEP(MD5_G, a, b, c, d, w[ 5], 0xd62f105du,  5); MD5_STEP(MD5_G, d, a, b, c, w[10], 0x02441453u,  9);
  MD5_STEP(MD5_G, c, d, a, b, w[15], 0xd8a1e681u, 14); MD5_STEP(MD5_G, b, c, d, a, w[ 4], 0xe7d3fbc8u, 20);
  MD5_STEP(MD5_G, a, b, c, d, w[ 9], 0x21e1cde6u,  5); MD5_STEP(MD5_G, d, a, b, c, w[14], 0xc33707d6u,  9);
  MD5_STEP(MD5_G, c, d, a, b, w[ 3], 0xf4d50d87u, 14); MD5_STEP(MD5_G, b, c, d, a, w[ 8], 0x455a14edu, 20);
  MD5_STEP(MD5_G, a, b, c, d, w[13], 0xa9e3e905u,  5); MD5_STEP(MD5_G, d, a, b, c, w[ 2], 0xfcefa3f8u,  9);
  MD5_STEP(MD5_G, c, d, a, b, w[ 7], 0x676f02d9u, 14); MD5_STEP(MD5_G, b, c, d, a, w[12], 0x8d2a4c8au, 20);

  MD5_STEP(MD5_H, a, b, c, d, w[ 5], 0xfffa3942u,  4); MD5_STEP(MD5_H, d, a, b, c, w[ 8], 0x8771f681u, 11);
  MD5_STEP(MD5_H, c, d, a, b, w[11], 0x6d9d6122u, 16); MD5_STEP(MD5_H, b, c, d, a, w[14], 0xfde5380cu, 23);
  MD5_STEP(MD5_H, a, b, c, d, w[ 1], 0xa4beea44u,  4); MD5_STEP(MD5_H, d, a, b, c, w[ 4], 0x4bdecfa9u, 11);
  MD5_STEP(MD5_H, c, d, a, b, w[ 7], 0xf6bb4b60u, 16); MD5_STEP(MD5_H, b, c, d, a, w[10], 0xbebfbc70u, 23);
  MD5_STEP(MD5_H, a, b, c, d, w[13], 0x289b7ec6u,  4); MD5_STEP(MD5_H, d, a, b, c, w[ 0], 0xeaa127fau, 11);
  MD5_STEP(MD5_H, c, d, a, b, w[ 3], 0xd4ef3085u, 16); MD5_STEP(MD5_H, b, c, d, a, w[ 6], 0x04881d05u, 23);
  MD5_STEP(MD5_H, a, b, c, d, w[ 9], 0xd9d4d039u,  4); MD5_STEP(MD5_H, d, a, b, c, w[12], 0xe6db99e5u, 11);
  MD5_STEP(MD5_H, c, d, a, b, w[15], 0x1fa27cf8u, 16); MD5_STEP(MD5_H, b, c, d, a, w[ 2], 0xc4ac5665u, 23);

  MD5_STEP(MD5_I, a, b, c, d, w[ 0], 0xf4292244u,  6); MD5_STEP(MD5_I, d, a, b, c, w[ 7], 0x432aff97u, 10);
  MD5_STEP(MD5_I, c, d, a, b, w[14], 0xab9423a7u, 15); MD5_STEP(MD5_I, b, c, d, a, w[ 5], 0xfc93a039u, 21);
  MD5_STEP(MD5_I, a, b, c, d, w[12], 0x655b59c3u,  6); MD5_STEP(MD5_I, d, a, b, c, w[ 3], 0x8f0ccc92u, 10);
  MD5_STEP(MD5_I, c, d, a, b, w[10], 0xffeff47du, 15); MD5_STEP(MD5_I, b, c, d, a, w[ 1], 0x85845dd1u, 21);
  MD5_STEP(MD5_I, a, b, c, d, w[ 8], 0x6fa87e4fu,  6); MD5_STEP(MD5_I, d, a, b, c, w[15], 0xfe2ce6e0u, 10);
  MD5_STEP(MD5_I, c, d, a, b, w[ 6], 0xa3014314u, 15); MD5_STEP(MD5_I, b, c, d, a, w[13], 0x4e0811a1u, 21);
  MD5_STEP(MD5_I, a, b, c, d, w[ 4], 0xf7537e82u,  6); MD5_STEP(MD5_I, d, a, b, c, w[11], 0xbd3af235u, 10);
  MD5_STEP(MD5_I, c, d, a, b, w[ 2], 0x2ad7d2bbu, 15); MD5_STEP(MD5_I, b, c, d, a, w[ 9], 0xeb86d391u, 21);
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}

// the loader (three alignment paths, the tail rule, the pad) is digest_load.hpp's, shared with SHA-1 and SHA-256: MD5 takes its
// words little-endian, as they lie, and the bit length little-endian in words 14 and 15
__device__ __forceinline__ u64 md5_blocks(u32 n) { return digest_blocks(n); }
__device__ __forceinline__ void md5_load_block(const u8 *p, const u32 n, const u64 k, u32 w[16]) { digest_load_block<false>(p, n, k, w); }

// one lane, one range: the digest of out_arena[out_off .. out_off + out_len) -> the sixteen bytes of res->out_len .. in_next
__device__ __forceinline__ void md5_unit(const mspack_hip_unit &u, const u8 *out_arena, const u64 out_bytes, mspack_hip_result *res)
{
  mspack_hip_result r;
  r.err = ERR_OK; r.flags = 0u; r.out_len = 0u; r.in_used = 0u; r.good_len = 0u; r.in_next = 0u;
  if (u.out_off > out_bytes || (u64) u.out_len > out_bytes - u.out_off) { r.err = ERR_ARGS; gst(res, r); return; }      // (the host entry points refuse these)
  const u8 *p = out_arena + u.out_off;
  const u32 n = u.out_len;
  const u64 nb = md5_blocks(n);
  u32 st[4] = { 0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u };
  u32 w[16], nx[16];
  md5_load_block(p, n, 0u, w);
  for (u64 k = 0; k < nb; k++) {
    const bool more = k + 1u < nb;
    if (more) md5_load_block(p, n, k + 1u, nx);            // the next block's loads are in flight while this one is compressed
    md5_block(st, w);
    if (more) {
#pragma unroll
      for (int j = 0; j < 16; j++) w[j] = nx[j];
    }
  }
  r.out_len = st[0]; r.in_used = st[1]; r.good_len = st[2]; r.in_next = st[3];
  gst(res, r);
}
