// sha_kernel.hpp -- MSPACK_HIP_KIND_SHA1 and MSPACK_HIP_KIND_SHA256: the SHA-1 / SHA-256 (FIPS 180-4) of a byte range of the output
// arena, computed where the bytes lie.  The shape is md5_kernel.hpp's: both hashes are one chain per message, so ONE LANE PER RANGE,
// 64 ranges per wavefront, one launch per algorithm over that algorithm's own list (lanes of one wave never run different hash
// functions), longest range first.  A lane keeps the state (5 / 8 words) and the SIXTEEN-word rolling message schedule in VGPRs:
// word t of the schedule (t >= 16) replaces word t - 16 in place, so there is no 80- or 64-word W array; the rounds are unrolled
// with their constants as literals, so every schedule index is a constant and a register.  A rotation is one v_alignbit_b32; Ch and
// Maj are bit-selects, Parity and the sigmas three-way xors: what the compiler makes v_bitop3_b32 of.  No table, no LDS, no
// atomics, no cross-lane traffic, no wait on another wave.
//
// Loading is digest_load.hpp's (the three alignment paths and the tail rule of md5_kernel.hpp), with the words big-endian -- one
// v_perm_b32 per loaded dword -- and the bit length big-endian in words 14 and 15.  The next block's words are loaded before the
// current block is compressed.
//
// A digest of 20 / 32 bytes does not fit the 16 bytes a result has to spare: bytes 0 .. 15 go into the unit's own result
// (out_len .. in_next), the rest into out_len .. of the NEXT unit's result, which must be an MSPACK_HIP_KIND_DIGEST_MORE unit
// (mspack_hip.h).  The head's lane writes both results; nothing else writes a tail's.
#pragma once
#include "wave_common.hpp"
#include "digest_load.hpp"

__device__ __forceinline__ u32 sha_rotr(u32 x, u32 s) { return __builtin_amdgcn_alignbit(x, x, s); }
__device__ __forceinline__ u32 sha_rotl(u32 x, u32 s) { return __builtin_amdgcn_alignbit(x, x, 32u - s); }
// bit-select: where the mask bit is set take a's bit, else b's
__device__ __forceinline__ u32 sha_sel(u32 mask, u32 a, u32 b) { return (mask & a) | (~mask & b); }
// the word as its bytes lie in the digest (big-endian), read as the little-endian word a result field is
__device__ __forceinline__ u32 sha_out(u32 v) { return __builtin_amdgcn_perm(0u, v, 0x00010203u); }

#define SHA_CH(x, y, z)     sha_sel((x), (y), (z))
#define SHA_MAJ(x, y, z)    sha_sel((x) ^ (y), (z), (y))              /* where x and y differ z decides, else they do */
#define SHA_PARITY(x, y, z) ((x) ^ (y) ^ (z))

// ---- SHA-256 ----
#define SHA256_S0(x) (sha_rotr((x), 2) ^ sha_rotr((x), 13) ^ sha_rotr((x), 22))
#define SHA256_S1(x) (sha_rotr((x), 6) ^ sha_rotr((x), 11) ^ sha_rotr((x), 25))
#define SHA256_s0(x) (sha_rotr((x), 7) ^ sha_rotr((x), 18) ^ ((x) >> 3))
#define SHA256_s1(x) (sha_rotr((x), 17) ^ sha_rotr((x), 19) ^ ((x) >> 10))
// round t: from t = 16 on the schedule word is made in place of word t - 16
#define SHA256_ROUND(a, b, c, d, e, f, g, h, t, k) do { \
    if ((t) >= 16) w[(t) & 15] += SHA256_s1(w[((t) - 2) & 15]) + w[((t) - 7) & 15] + SHA256_s0(w[((t) - 15) & 15]); \
    (h) += SHA256_S1(e) + SHA_CH((e), (f), (g)) + (k) + w[(t) & 15]; \
    (d) += (h); \
    (h) += SHA256_S0(a) + SHA_MAJ((a), (b), (c)); } while (0)

// one block: st[8] += compress(st, w[16]); w is used up (it holds the schedule's last sixteen words afterwards)
__device__ __forceinline__ void sha256_block(u32 st[8], u32 w[16])
{
  u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  SHA256_ROUND(a, b, c, d, e, f, g, h,  0, 0x428a2f98u); SHA256_ROUND(h, a, b, c, d, e, f, g,  1, 0x71374491u);
  SHA256_ROUND(g, h, a, b, c, d, e, f,  2, 0xb5c0fbcfu); SHA256_ROUND(f, g, h, a, b, c, d, e,  3, 0xe9b5dba5u);
  SHA256_ROUND(e, f, g, h, a, b, c, d,  4, 0x3956c25bu); SHA256_ROUND(d, e, f, g, h, a, b, c,  5, 0x59f111f1u);
  SHA256_ROUND(c, d, e, f, g, h, a, b,  6, 0x923f82a4u); SHA256_ROUND(b, c, d, e, f, g, h, a,  7, 0xab1c5ed5u);
  SHA256_ROUND(a, b, c, d, e, f, g, h,  8, 0xd807aa98u); SHA256_ROUND(h, a, b, c, d, e, f, g,  9, 0x12835b01u);
  SHA256_ROUND(g, h, a, b, c, d, e, f, 10, 0x243185beu); SHA256_ROUND(f, g, h, a, b, c, d, e, 11, 0x550c7dc3u);
  SHA256_ROUND(e, f, g, h, a, b, c, d, 12, 0x72be5d74u); SHA256_ROUND(d, e, f, g, h, a, b, c, 13, 0x80deb1feu);
  SHA256_ROUND(c, d, e, f, g, h, a, b, 14, 0x9bdc06a7u); SHA256_ROUND(b, c, d, e, f, g, h, a, 15, 0xc19bf174u);
  SHA256_ROUND(a, b, c, d, e, f, g, h, 16, 0xe49b69c1u); SHA256_ROUND(h, a, b, c, d, e, f, g, 17, 0xefbe4786u);
  SHA256_ROUND(g, h, a, b, c, d, e, f, 18, 0x0fc19dc6u); SHA256_ROUND(f, g, h, a, b, c, d, e, 19, 0x240ca1ccu);
  SHA256_ROUND(e, f, g, h, a, b, c, d, 20, 0x2de92c6fu); SHA256_ROUND(d, e, f, g, h, a, b, c, 21, 0x4a7484aau);
  SHA256_ROUND(c, d, e, f, g, h, a, b, 22, 0x5cb0a9dcu); SHA256_ROUND(b, c, d, e, f, g, h, a, 23, 0x76f988dau);
  SHA256_ROUND(a, b, c, d, e, f, g, h, 24, 0x983e5152u); SHA256_ROUND(h, a, b, c, d, e, f, g, 25, 0xa831c66du);
  SHA256_ROUND(g, h, a, b, c, d, e, f, 26, 0xb00327c8u); SHA256_ROUND(f, g, h, a, b, c, d, e, 27, 0xbf597fc7u);
  SHA256_ROUND(e, f, g, h, a, b, c, d, 28, 0xc6e00bf3u); SHA256_ROUND(d, e, f, g, h, a, b, c, 29, 0xd5a79147u);
  SHA256_ROUND(c, d, e, f, g, h, a, b, 30, 0x06ca6351u); SHA256_ROUND(b, c, d, e, f, g, h, a, 31, 0x14292967u);
  SHA256_ROUND(a, b, c, d, e, f, g, h, 32, 0x27b70a85u); SHA256_ROUND(h, a, b, c, d, e, f, g, 33, 0x2e1b2138u);
  SHA256_ROUND(g, h, a, b, c, d, e, f, 34, 0x4d2c6dfcu); SHA256_ROUND(f, g, h, a, b, c, d, e, 35, 0x53380d13u);
  SHA256_ROUND(e, f, g, h, a, b, c, d, 36, 0x650a7354u); SHA256_ROUND(d, e, f, g, h, a, b, c, 37, 0x766a0abbu);
  SHA256_ROUND(c, d, e, f, g, h, a, b, 38, 0x81c2c92eu); SHA256_ROUND(b, c, d, e, f, g, h, a, 39, 0x92722c85u);
  SHA256_ROUND(a, b, c, d, e, f, g, h, 40, 0xa2bfe8a1u); SHA256_ROUND(h, a, b, c, d, e, f, g, 41, 0xa81a664bu);
  SHA256_ROUND(g, h, a, b, c, d, e, f, 42, 0xc24b8b70u); SHA256_ROUND(f, g, h, a, b, c, d, e, 43, 0xc76c51a3u);
  SHA256_ROUND(e, f, g, h, a, b, c, d, 44, 0xd192e819u); SHA256_ROUND(d, e, f, g, h, a, b, c, 45, 0xd6990624u);
  SHA256_ROUND(c, d, e, f, g, h, a, b, 46, 0xf40e3585u); SHA256_ROUND(b, c, d, e, f, g, h, a, 47, 0x106aa070u);
  SHA256_ROUND(a, b, c, d, e, f, g, h, 48, 0x19a4c116u); SHA256_ROUND(h, a, b, c, d, e, f, g, 49, 0x1e376c08u);
  SHA256_ROUND(g, h, a, b, c, d, e, f, 50, 0x2748774cu); SHA256_ROUND(f, g, h, a, b, c, d, e, 51, 0x34b0bcb5u);
  SHA256_ROUND(e, f, g, h, a, b, c, d, 52, 0x391c0cb3u); SHA256_ROUND(d, e, f, g, h, a, b, c, 53, 0x4ed8aa4au);
  SHA256_ROUND(c, d, e, f, g, h, a, b, 54, 0x5b9cca4fu); SHA256_ROUND(b, c, d, e, f, g, h, a, 55, 0x682e6ff3u);
  SHA256_ROUND(a, b, c, d, e, f, g, h, 56, 0x748f82eeu); SHA256_ROUND(h, a, b, c, d, e, f, g, 57, 0x78a5636fu);
  SHA256_ROUND(g, h, a, b, c, d, e, f, 58, 0x84c87814u); SHA256_ROUND(f, g, h, a, b, c, d, e, 59, 0x8cc70208u);
  SHA256_ROUND(e, f, g, h, a, b, c, d, 60, 0x90befffau); SHA256_ROUND(d, e, f, g, h, a, b, c, 61, 0xa4506cebu);
  SHA256_ROUND(c, d, e, f, g, h, a, b, 62, 0xbef9a3f7u); SHA256_ROUND(b, c, d, e, f, g, h, a, 63, 0xc67178f2u);
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// ---- SHA-1 ----
#define SHA1_ROUND(fn, a, b, c, d, e, t, k) do { \
    if ((t) >= 16) w[(t) & 15] = sha_rotl(w[((t) - 3) & 15] ^ w[((t) - 8) & 15] ^ w[((t) - 14) & 15] ^ w[(t) & 15], 1); \
    (e) += sha_rotl((a), 5) + fn((b), (c), (d)) + (k) + w[(t) & 15]; \
    (b) = sha_rotl((b), 30); } while (0)

__device__ __forceinline__ void sha1_block(u32 st[5], u32 w[16])
{
  u32 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4];
  SHA1_ROUND(SHA_CH    , a, b, c, d, e,  0, 0x5a827999u); SHA1_ROUND(SHA_CH    , e, a, b, c, d,  1, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , d, e, a, b, c,  2, 0x5a827999u); SHA1_ROUND(SHA_CH    , c, d, e, a, b,  3, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , b, c, d, e, a,  4, 0x5a827999u); SHA1_ROUND(SHA_CH    , a, b, c, d, e,  5, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , e, a, b, c, d,  6, 0x5a827999u); SHA1_ROUND(SHA_CH    , d, e, a, b, c,  7, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , c, d, e, a, b,  8, 0x5a827999u); SHA1_ROUND(SHA_CH    , b, c, d, e, a,  9, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , a, b, c, d, e, 10, 0x5a827999u); SHA1_ROUND(SHA_CH    , e, a, b, c, d, 11, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , d, e, a, b, c, 12, 0x5a827999u); SHA1_ROUND(SHA_CH    , c, d, e, a, b, 13, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , b, c, d, e, a, 14, 0x5a827999u); SHA1_ROUND(SHA_CH    , a, b, c, d, e, 15, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , e, a, b, c, d, 16, 0x5a827999u); SHA1_ROUND(SHA_CH    , d, e, a, b, c, 17, 0x5a827999u);
  SHA1_ROUND(SHA_CH    , c, d, e, a, b, 18, 0x5a827999u); SHA1_ROUND(SHA_CH    , b, c, d, e, a, 19, 0x5a827999u);

  SHA1_ROUND(SHA_PARITY, a, b, c, d, e, 20, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, e, a, b, c, d, 21, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, d, e, a, b, c, 22, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, c, d, e, a, b, 23, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, b, c, d, e, a, 24, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, a, b, c, d, e, 25, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, e, a, b, c, d, 26, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, d, e, a, b, c, 27, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, c, d, e, a, b, 28, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, b, c, d, e, a, 29, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, a, b, c, d, e, 30, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, e, a, b, c, d, 31, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, d, e, a, b, c, 32, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, c, d, e, a, b, 33, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, b, c, d, e, a, 34, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, a, b, c, d, e, 35, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, e, a, b, c, d, 36, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, d, e, a, b, c, 37, 0x6ed9eba1u);
  SHA1_ROUND(SHA_PARITY, c, d, e, a, b, 38, 0x6ed9eba1u); SHA1_ROUND(SHA_PARITY, b, c, d, e, a, 39, 0x6ed9eba1u);

  SHA1_ROUND(SHA_MAJ   , a, b, c, d, e, 40, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , e, a, b, c, d, 41, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , d, e, a, b, c, 42, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , c, d, e, a, b, 43, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , b, c, d, e, a, 44, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , a, b, c, d, e, 45, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , e, a, b, c, d, 46, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , d, e, a, b, c, 47, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , c, d, e, a, b, 48, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , b, c, d, e, a, 49, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , a, b, c, d, e, 50, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , e, a, b, c, d, 51, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , d, e, a, b, c, 52, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , c, d, e, a, b, 53, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , b, c, d, e, a, 54, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , a, b, c, d, e, 55, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , e, a, b, c, d, 56, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , d, e, a, b, c, 57, 0x8f1bbcdcu);
  SHA1_ROUND(SHA_MAJ   , c, d, e, a, b, 58, 0x8f1bbcdcu); SHA1_ROUND(SHA_MAJ   , b, c, d, e, a, 59, 0x8f1bbcdcu);

  SHA1_ROUND(SHA_PARITY, a, b, c, d, e, 60, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, e, a, b, c, d, 61, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, d, e, a, b, c, 62, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, c, d, e, a, b, 63, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, b, c, d, e, a, 64, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, a, b, c, d, e, 65, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, e, a, b, c, d, 66, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, d, e, a, b, c, 67, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, c, d, e, a, b, 68, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, b, c, d, e, a, 69, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, a, b, c, d, e, 70, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, e, a, b, c, d, 71, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, d, e, a, b, c, 72, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, c, d, e, a, b, 73, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, b, c, d, e, a, 74, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, a, b, c, d, e, 75, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, e, a, b, c, d, 76, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, d, e, a, b, c, 77, 0xca62c1d6u);
  SHA1_ROUND(SHA_PARITY, c, d, e, a, b, 78, 0xca62c1d6u); SHA1_ROUND(SHA_PARITY, b, c, d, e, a, 79, 0xca62c1d6u);
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e;
}

template <int KIND> struct ShaAlg;
template <> struct ShaAlg<MSPACK_HIP_KIND_SHA1> {
  static constexpr int WORDS = 5;
  static __device__ __forceinline__ void init(u32 *st) { st[0] = 0x67452301u; st[1] = 0xefcdab89u; st[2] = 0x98badcfeu; st[3] = 0x10325476u; st[4] = 0xc3d2e1f0u; }
  static __device__ __forceinline__ void block(u32 *st, u32 *w) { sha1_block(st, w); }
};
template <> struct ShaAlg<MSPACK_HIP_KIND_SHA256> {
  static constexpr int WORDS = 8;
  static __device__ __forceinline__ void init(u32 *st) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au; st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
  }
  static __device__ __forceinline__ void block(u32 *st, u32 *w) { sha256_block(st, w); }
};

__device__ __forceinline__ bool sha_is_head(u32 kind) { return kind == MSPACK_HIP_KIND_SHA1 || kind == MSPACK_HIP_KIND_SHA256; }
// the tails a head of this kind needs (mspack_hip.h: ceil(digest bytes / 16) - 1); 0: no wide head
__device__ __forceinline__ u32 sha_tails_of(u32 kind)
{
  return sha_is_head(kind) ? 1u : kind == MSPACK_HIP_KIND_SHA384 ? 2u : kind == MSPACK_HIP_KIND_SHA512 ? 3u : 0u;
}

// a lane that met an MSPACK_HIP_KIND_DIGEST_MORE unit (the device-resident entry only: the host entry points list heads alone): a
// tail is its head's lane's to write when the first unit in front of it that is no tail is a head that needs as many tails as
// stand between them (itself included); every other tail -- no head, or more tails than the head needs -- answers MSPACK_ERR_ARGS
__device__ __forceinline__ void sha_tail_unit(const mspack_hip_unit *units, const u32 ui, mspack_hip_result *results)
{
  u32 k = 1u;
  while (k < 3u && k < ui && units[ui - k].kind == MSPACK_HIP_KIND_DIGEST_MORE) k++;
  if (k <= ui && sha_tails_of(units[ui - k].kind) >= k) return;
  mspack_hip_result r;
  r.err = ERR_ARGS; r.flags = 0u; r.out_len = 0u; r.in_used = 0u; r.good_len = 0u; r.in_next = 0u;
  gst(&results[ui], r);
}

// one lane, one range: the digest of out_arena[out_off .. out_off + out_len) of unit ui (a head of this algorithm) -> bytes 0 .. 15
// in results[ui].out_len .. in_next, the rest in results[ui + 1].out_len ..
template <int KIND>
__device__ __forceinline__ void sha_unit(const mspack_hip_unit *units, const u32 ui, const u32 n_table, const mspack_hip_unit &u,
                                         const u8 *out_arena, const u64 out_bytes, mspack_hip_result *results)
{
  typedef ShaAlg<KIND> A;
  mspack_hip_result r, t;
  r.err = ERR_OK; r.flags = 0u; r.out_len = 0u; r.in_used = 0u; r.good_len = 0u; r.in_next = 0u;
  t = r;
  // the tail: units[ui + 1], an MSPACK_HIP_KIND_DIGEST_MORE unit that names nothing (the host entry points refuse the rest)
  bool tail = ui + 1u < n_table;
  if (tail) { const mspack_hip_unit m = units[ui + 1u]; tail = m.kind == MSPACK_HIP_KIND_DIGEST_MORE && m.in_len == 0u && m.out_len == 0u; }
  if (!tail) { r.err = ERR_ARGS; gst(&results[ui], r); return; }
  if (u.out_off > out_bytes || (u64) u.out_len > out_bytes - u.out_off) { r.err = ERR_ARGS; gst(&results[ui], r); gst(&results[ui + 1u], t); return; }
  const u8 *p = out_arena + u.out_off;
  const u32 n = u.out_len;
  const u64 nb = digest_blocks(n);
  u32 st[A::WORDS];
  A::init(st);
  u32 w[16], nx[16];
  digest_load_block<true>(p, n, 0u, w);
  for (u64 k = 0; k < nb; k++) {
    const bool more = k + 1u < nb;
    if (more) digest_load_block<true>(p, n, k + 1u, nx);   // the next block's loads are in flight while this one is compressed
    A::block(st, w);
    if (more) {
#pragma unroll
      for (int j = 0; j < 16; j++) w[j] = nx[j];
    }
  }
  r.out_len = sha_out(st[0]); r.in_used = sha_out(st[1]); r.good_len = sha_out(st[2]); r.in_next = sha_out(st[3]);
  t.out_len = sha_out(st[4]);
  if (A::WORDS == 8) { t.in_used = sha_out(st[5]); t.good_len = sha_out(st[6]); t.in_next = sha_out(st[7]); }
  gst(&results[ui], r);
  gst(&results[ui + 1u], t);
}
