// digest_load.hpp -- the message loader of the digest kernels (md5_kernel.hpp, sha_kernel.hpp, sha512_kernel.hpp): block k of the
// padded message of a byte range, NW 32-bit words in VGPRs.  MD5, SHA-1 and SHA-256 (NW = 16: 64-byte blocks) pad alike (0x80,
// zeros, the 64-bit bit length in the last block's words 14 and 15) and differ in two things only: the byte order of a word (SHA:
// big-endian, one v_perm_b32 per loaded dword) and the order of the length's two words.  SHA-384 / SHA-512 (NW = 32: 128-byte
// blocks) pad the same way with a 128-bit big-endian bit length -- out_len is 32-bit, so its upper three words are the zeros the
// padding left there and the lower 64 bits lie in words 30 and 31 --; a 64-bit message word i is the pair (w[2 i], w[2 i + 1]),
// high half first.  The three alignment paths and the tail rule are described in md5_kernel.hpp.
#pragma once
#include "wave_common.hpp"

// a dword as it was loaded (little-endian) -> the message word
template <bool BE> __device__ __forceinline__ u32 digest_word(u32 v) { return BE ? __builtin_amdgcn_perm(0u, v, 0x00010203u) : v; }

// blocks of the padded message of n bytes: n + 1 (0x80) + 8 (the bit length), rounded up to 64 (NW = 32: + 16, to 128)
template <int NW> __device__ __forceinline__ u64 digest_blocks_of(u32 n) { return ((u64) n + (u32)(NW / 2)) / (u32)(4 * NW) + 1u; }
__device__ __forceinline__ u64 digest_blocks(u32 n) { return digest_blocks_of<16>(n); }

// block k (of digest_blocks_of<NW>(n)) of the message p[0 .. n) into w[NW]; BE: the words big-endian
template <bool BE, int NW = 16>
__device__ __forceinline__ void digest_load_block(const u8 *p, const u32 n, const u64 k, u32 w[NW])
{
  constexpr u32 BB = 4u * (u32) NW;                        // the block's bytes
  const u64 o = k * BB;                                    // the block's first byte in the message
  const u8 *b = p + o;
  const u32 sh = (u32)((size_t) p & 3u);
  if (o + BB <= (u64) n) {                                // a whole block of message bytes
    if (((size_t) p & 15u) == 0u) {
      const uint4 *r = (const uint4 *) b;
#pragma unroll
      for (int j = 0; j < NW / 4; j++) { const uint4 v = gld(r + j); w[4 * j] = digest_word<BE>(v.x); w[4 * j + 1] = digest_word<BE>(v.y); w[4 * j + 2] = digest_word<BE>(v.z); w[4 * j + 3] = digest_word<BE>(v.w); }
    }
    else if (sh == 0u) {
      const u32 *q = (const u32 *) b;
#pragma unroll
      for (int j = 0; j < NW; j++) w[j] = digest_word<BE>(gld(q + j));
    }
    else {
      const u32 *q = (const u32 *)(b - sh);               // q[0] holds the block's first 4 - sh bytes, q[NW] its last sh
      u32 lo = gld(q);
#pragma unroll
      for (int j = 0; j < NW; j++) { const u32 hi = gld(q + j + 1); w[j] = digest_word<BE>(__builtin_amdgcn_alignbyte(hi, lo, sh)); lo = hi; }
    }
    return;
  }
  // the tail: what is left of the message, 0x80, zeros; the bit length ends the last block
  const u32 rem = (u64) n > o ? (u32)((u64) n - o) : 0u;   // message bytes in this block (< BB)
  const bool pad_here = (u64) n >= o;                      // the 0x80 lies in this block (else it lay in the block before)
#pragma unroll
  for (int j = 0; j < NW; j++) {
    const u32 at = 4u * (u32) j;                           // the word's first byte in the block
    u32 v = 0u;
    if (at < rem) {
      const u32 have = rem - at;                           // message bytes from here on: 1 ..
      const u32 *q = (const u32 *)(b + at - sh);           // the aligned dword that holds byte `at`
      const u32 lo = gld(q);
      const u32 hi = (sh != 0u && have > 4u - sh) ? gld(q + 1) : 0u;      // (the next one only if a byte of the range is in it)
      v = __builtin_amdgcn_alignbyte(hi, lo, sh);
      if (have < 4u) v = (v & ((1u << (8u * have)) - 1u)) | (0x80u << (8u * have));
    }
    else if (at == rem && pad_here) v = 0x80u;
    w[j] = digest_word<BE>(v);
  }
  if (k + 1u == digest_blocks_of<NW>(n)) { w[NW - 2] = BE ? n >> 29 : n << 3; w[NW - 1] = BE ? n << 3 : n >> 29; }
}
