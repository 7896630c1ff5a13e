// sha512_kernel.hpp -- MSPACK_HIP_KIND_SHA384 and MSPACK_HIP_KIND_SHA512: the SHA-384 / SHA-512 (FIPS 180-4) of a byte range of the
// output arena, computed where the bytes lie.  The shape is sha_kernel.hpp's: ONE LANE PER RANGE, 64 ranges per wavefront, longest
// range first, no table, no LDS, no atomics, no cross-lane traffic, no wait on another wave.  The two algorithms share the
// compression function and differ in the initial state and in how many words of the state are the digest, so they share ONE list
// and ONE launch: a lane picks its initial state by its unit's kind (eight selects), and lanes of one wave still never run
// different hash functions.
//
// This is not SHA-256 with other constants: the words are 64 bits wide, a block has 128 bytes, there are 80 rounds and the length
// field has 128 bits.  A lane keeps eight 64-bit state words and the SIXTEEN-word rolling 64-bit schedule in VGPR pairs; word t
// (t >= 16) replaces word t - 16 in place and the 80 rounds are unrolled, so every schedule index is a constant and a register.
// gfx950 has no 64-bit rotate: a rotate by s < 32 is two v_alignbit_b32 over the (hi, lo) pair -- lo' = (hi:lo) >> s, hi' =
// (lo:hi) >> s --, one by s >= 32 the same with the halves swapped and s - 32; the sigmas' plain shifts are one v_alignbit_b32 and
// one v_lshrrev_b32.  Ch and Maj are bit-selects, the sigmas three-way xors, each applied per half (v_bitop3_b32 / v_bfi_b32).
// The 64-bit adds are left to the compiler as uint64_t sums: gfx950 has v_lshl_add_u64, one instruction per add with a shift
// count of 0, so there is no v_add_co_u32 / v_addc_co_u32 chain through VCC.  The eighty 64-bit round constants are literals
// in the source; where the compiler puts them is said in DESIGN.md section 4.7b.
//
// Loading is digest_load.hpp's with NW = 32 (the three alignment paths and the tail rule of md5_kernel.hpp): thirty-two big-endian
// dwords, message word i the pair (2 i, 2 i + 1), the bit length big-endian in the last block's last sixteen bytes.  The next
// block's dwords are loaded before the current block is compressed.
//
// A digest of 48 / 64 bytes continues in the results of the TWO / THREE MSPACK_HIP_KIND_DIGEST_MORE units behind the head
// (mspack_hip.h): bytes 16 k .. 16 k + 15 in results[ui + k] from out_len on.  The head's lane writes all of them; nothing else
// writes a tail's.
#pragma once
#include "wave_common.hpp"
#include "digest_load.hpp"
#include "sha_kernel.hpp"

// (hi:lo) >> s for 0 < s < 32, the low word: what a funnel shift gives
__device__ __forceinline__ u64 sha512_pair(u32 hi, u32 lo) { return ((u64) hi << 32) | lo; }
template <int S> __device__ __forceinline__ u64 sha512_rotr(u64 x)
{
  const u32 lo = (u32) x, hi = (u32)(x >> 32);
  if (S < 32) return sha512_pair(__builtin_amdgcn_alignbit(lo, hi, S), __builtin_amdgcn_alignbit(hi, lo, S));
  if (S == 32) return sha512_pair(lo, hi);
  return sha512_pair(__builtin_amdgcn_alignbit(hi, lo, S - 32), __builtin_amdgcn_alignbit(lo, hi, S - 32));
}
template <int S> __device__ __forceinline__ u64 sha512_shr(u64 x)       // 0 < S < 32
{
  const u32 lo = (u32) x, hi = (u32)(x >> 32);
  return sha512_pair(hi >> S, __builtin_amdgcn_alignbit(hi, lo, S));
}
// bit-select per half: where the mask bit is set take a's bit, else b's
__device__ __forceinline__ u64 sha512_sel(u64 mask, u64 a, u64 b)
{
  return sha512_pair(sha_sel((u32)(mask >> 32), (u32)(a >> 32), (u32)(b >> 32)), sha_sel((u32) mask, (u32) a, (u32) b));
}
#define SHA512_CH(x, y, z)  sha512_sel((x), (y), (z))
#define SHA512_MAJ(x, y, z) sha512_sel((x) ^ (y), (z), (y))           /* where x and y differ z decides, else they do */
#define SHA512_S0(x) (sha512_rotr<28>(x) ^ sha512_rotr<34>(x) ^ sha512_rotr<39>(x))
#define SHA512_S1(x) (sha512_rotr<14>(x) ^ sha512_rotr<18>(x) ^ sha512_rotr<41>(x))
#define SHA512_s0(x) (sha512_rotr<1>(x) ^ sha512_rotr<8>(x) ^ sha512_shr<7>(x))
#define SHA512_s1(x) (sha512_rotr<19>(x) ^ sha512_rotr<61>(x) ^ sha512_shr<6>(x))
// round t: from t = 16 on the schedule word is made in place of word t - 16
#define SHA512_ROUND(a, b, c, d, e, f, g, h, t, k) do { \
    if ((t) >= 16) w[(t) & 15] += SHA512_s1(w[((t) - 2) & 15]) + w[((t) - 7) & 15] + SHA512_s0(w[((t) - 15) & 15]); \
    (h) += SHA512_S1(e) + SHA512_CH((e), (f), (g)) + (k) + w[(t) & 15]; \
    (d) += (h); \
    (h) += SHA512_S0(a) + SHA512_MAJ((a), (b), (c)); } while (0)

// one block: st[8] += compress(st, w[16]); w is used up (it holds the schedule's last sixteen words afterwards)
__device__ __forceinline__ void sha512_block(u64 st[8], u64 w[16])
{
  u64 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  SHA512_ROUND(a, b, c, d, e, f, g, h,  0, 0x428a2f98d728ae22ull); SHA512_ROUND(h, a, b, c, d, e, f, g,  1, 0x7137449123ef65cdull);
  SHA512_ROUND(g, h, a, b, c, d, e, f,  2, 0xb5c0fbcfec4d3b2full); SHA512_ROUND(f, g, h, a, b, c, d, e,  3, 0xe9b5dba58189dbbcull);
  SHA512_ROUND(e, f, g, h, a, b, c, d,  4, 0x3956c25bf348b538ull); SHA512_ROUND(d, e, f, g, h, a, b, c,  5, 0x59f111f1b605d019ull);
  SHA512_ROUND(c, d, e, f, g, h, a, b,  6, 0x923f82a4af194f9bull); SHA512_ROUND(b, c, d, e, f, g, h, a,  7, 0xab1c5ed5da6d8118ull);
  SHA512_ROUND(a, b, c, d, e, f, g, h,  8, 0xd807aa98a3030242ull); SHA512_ROUND(h, a, b, c, d, e, f, g,  9, 0x12835b0145706fbeull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 10, 0x243185be4ee4b28cull); SHA512_ROUND(f, g, h, a, b, c, d, e, 11, 0x550c7dc3d5ffb4e2ull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 12, 0x72be5d74f27b896full); SHA512_ROUND(d, e, f, g, h, a, b, c, 13, 0x80deb1fe3b1696b1ull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 14, 0x9bdc06a725c71235ull); SHA512_ROUND(b, c, d, e, f, g, h, a, 15, 0xc19bf174cf692694ull);
  SHA512_ROUND(a, b, c, d, e, f, g, h, 16, 0xe49b69c19ef14ad2ull); SHA512_ROUND(h, a, b, c, d, e, f, g, 17, 0xefbe4786384f25e3ull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 18, 0x0fc19dc68b8cd5b5ull); SHA512_ROUND(f, g, h, a, b, c, d, e, 19, 0x240ca1cc77ac9c65ull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 20, 0x2de92c6f592b0275ull); SHA512_ROUND(d, e, f, g, h, a, b, c, 21, 0x4a7484aa6ea6e483ull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 22, 0x5cb0a9dcbd41fbd4ull); SHA512_ROUND(b, c, d, e, f, g, h, a, 23, 0x76f988da831153b5ull);
  SHA512_ROUND(a, b, c, d, e, f, g, h, 24, 0x983e5152ee66dfabull); SHA512_ROUND(h, a, b, c, d, e, f, g, 25, 0xa831c66d2db43210ull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 26, 0xb00327c898fb213full); SHA512_ROUND(f, g, h, a, b, c, d, e, 27, 0xbf597fc7beef0ee4ull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 28, 0xc6e00bf33da88fc2ull); SHA512_ROUND(d, e, f, g, h, a, b, c, 29, 0xd5a79147930aa725ull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 30, 0x06ca6351e003826full); SHA512_ROUND(b, c, d, e, f, g, h, a, 31, 0x142929670a0e6e70ull);
  SHA512_ROUND(a, b, c, d, e, f, g, h, 32, 0x27b70a8546d22ffcull); SHA512_ROUND(h, a, b, c, d, e, f, g, 33, 0x2e1b21385c26c926ull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 34, 0x4d2c6dfc5ac42aedull); SHA512_ROUND(f, g, h, a, b, c, d, e, 35, 0x53380d139d95b3dfull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 36, 0x650a73548baf63deull); SHA512_ROUND(d, e, f, g, h, a, b, c, 37, 0x766a0abb3c77b2a8ull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 38, 0x81c2c92e47edaee6ull); SHA512_ROUND(b, c, d, e, f, g, h, a, 39, 0x92722c851482353bull);
  SHA512_ROUND(a, b, c, d, e, f, g, h, 40, 0xa2bfe8a14cf10364ull); SHA512_ROUND(h, a, b, c, d, e, f, g, 41, 0xa81a664bbc423001ull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 42, 0xc24b8b70d0f89791ull); SHA512_ROUND(f, g, h, a, b, c, d, e, 43, 0xc76c51a30654be30ull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 44, 0xd192e819d6ef5218ull); SHA512_ROUND(d, e, f, g, h, a, b, c, 45, 0xd69906245565a910ull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 46, 0xf40e35855771202aull); SHA512_ROUND(b, c, d, e, f, g, h, a, 47, 0x106aa07032bbd1b8ull);
  SHA512_ROUND(a, b, c, d, e, f, g, h, 48, 0x19a4c116b8d2d0c8ull); SHA512_ROUND(h, a, b, c, d, e, f, g, 49, 0x1e376c085141ab53ull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 50, 0x2748774cdf8eeb99ull); SHA512_ROUND(f, g, h, a, b, c, d, e, 51, 0x34b0bcb5e19b48a8ull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 52, 0x391c0cb3c5c95a63ull); SHA512_ROUND(d, e, f, g, h, a, b, c, 53, 0x4ed8aa4ae3418acbull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 54, 0x5b9cca4f7763e373ull); SHA512_ROUND(b, c, d, e, f, g, h, a, 55, 0x682e6ff3d6b2b8a3ull);
  SHA512_ROUND(a, b, c, d, e, f, g, h, 56, 0x748f82ee5defb2fcull); SHA512_ROUND(h, a, b, c, d, e, f, g, 57, 0x78a5636f43172f60ull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 58, 0x84c87814a1f0ab72ull); SHA512_ROUND(f, g, h, a, b, c, d, e, 59, 0x8cc702081a6439ecull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 60, 0x90befffa23631e28ull); SHA512_ROUND(d, e, f, g, h, a, b, c, 61, 0xa4506cebde82bde9ull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 62, 0xbef9a3f7b2c67915ull); SHA512_ROUND(b, c, d, e, f, g, h, a, 63, 0xc67178f2e372532bull);
  SHA512_ROUND(a, b, c, d, e, f, g, h, 64, 0xca273eceea26619cull); SHA512_ROUND(h, a, b, c, d, e, f, g, 65, 0xd186b8c721c0c207ull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 66, 0xeada7dd6cde0eb1eull); SHA512_ROUND(f, g, h, a, b, c, d, e, 67, 0xf57d4f7fee6ed178ull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 68, 0x06f067aa72176fbaull); SHA512_ROUND(d, e, f, g, h, a, b, c, 69, 0x0a637dc5a2c898a6ull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 70, 0x113f9804bef90daeull); SHA512_ROUND(b, c, d, e, f, g, h, a, 71, 0x1b710b35131c471bull);
  SHA512_ROUND(a, b, c, d, e, f, g, h, 72, 0x28db77f523047d84ull); SHA512_ROUND(h, a, b, c, d, e, f, g, 73, 0x32caab7b40c72493ull);
  SHA512_ROUND(g, h, a, b, c, d, e, f, 74, 0x3c9ebe0a15c9bebcull); SHA512_ROUND(f, g, h, a, b, c, d, e, 75, 0x431d67c49c100d4cull);
  SHA512_ROUND(e, f, g, h, a, b, c, d, 76, 0x4cc5d4becb3e42b6ull); SHA512_ROUND(d, e, f, g, h, a, b, c, 77, 0x597f299cfc657e2aull);
  SHA512_ROUND(c, d, e, f, g, h, a, b, 78, 0x5fcb6fab3ad6faecull); SHA512_ROUND(b, c, d, e, f, g, h, a, 79, 0x6c44198c4a475817ull);
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// the sixteen bytes 16 k .. 16 k + 15 of the digest -- state words 2 k and 2 k + 1, big-endian -- as a result's four spare words
__device__ __forceinline__ void sha512_out(mspack_hip_result &r, u64 x, u64 y)
{
  r.out_len = sha_out((u32)(x >> 32)); r.in_used = sha_out((u32) x); r.good_len = sha_out((u32)(y >> 32)); r.in_next = sha_out((u32) y);
}

// one lane, one range: the digest of out_arena[out_off .. out_off + out_len) of unit ui (an MSPACK_HIP_KIND_SHA384 or _SHA512 head) ->
// bytes 0 .. 15 in results[ui].out_len .. in_next, bytes 16 k .. in results[ui + k].out_len .. of its two / three tails
__device__ __forceinline__ void sha512_unit(const mspack_hip_unit *units, const u32 ui, const u32 n_table, const mspack_hip_unit &u,
                                            const u8 *out_arena, const u64 out_bytes, mspack_hip_result *results)
{
  const bool is384 = u.kind == MSPACK_HIP_KIND_SHA384;
  const u32 n_tails = is384 ? 2u : 3u;
  mspack_hip_result r, t;
  r.err = ERR_OK; r.flags = 0u; r.out_len = 0u; r.in_used = 0u; r.good_len = 0u; r.in_next = 0u;
  t = r;
  // the tails: units[ui + 1 .. ui + n_tails], MSPACK_HIP_KIND_DIGEST_MORE units that name nothing (the host entry points refuse the rest)
  bool tails = (u64) ui + n_tails < (u64) n_table;
  if (tails)
    for (u32 j = 1u; j <= n_tails; j++) { const mspack_hip_unit m = units[ui + j]; tails = tails && m.kind == MSPACK_HIP_KIND_DIGEST_MORE && m.in_len == 0u && m.out_len == 0u; }
  if (!tails) { r.err = ERR_ARGS; gst(&results[ui], r); return; }
  if (u.out_off > out_bytes || (u64) u.out_len > out_bytes - u.out_off) {
    r.err = ERR_ARGS; gst(&results[ui], r);
    for (u32 j = 1u; j <= n_tails; j++) gst(&results[ui + j], t);
    return;
  }
  const u8 *p = out_arena + u.out_off;
  const u32 n = u.out_len;
  const u64 nb = digest_blocks_of<32>(n);
  u64 st[8];
  st[0] = is384 ? 0xcbbb9d5dc1059ed8ull : 0x6a09e667f3bcc908ull; st[1] = is384 ? 0x629a292a367cd507ull : 0xbb67ae8584caa73bull;
  st[2] = is384 ? 0x9159015a3070dd17ull : 0x3c6ef372fe94f82bull; st[3] = is384 ? 0x152fecd8f70e5939ull : 0xa54ff53a5f1d36f1ull;
  st[4] = is384 ? 0x67332667ffc00b31ull : 0x510e527fade682d1ull; st[5] = is384 ? 0x8eb44a8768581511ull : 0x9b05688c2b3e6c1full;
  st[6] = is384 ? 0xdb0c2e0d64f98fa7ull : 0x1f83d9abfb41bd6bull; st[7] = is384 ? 0x47b5481dbefa4fa4ull : 0x5be0cd19137e2179ull;
  u32 nx[32];
  u64 w[16];
  digest_load_block<true, 32>(p, n, 0u, nx);
  for (u64 k = 0; k < nb; k++) {
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = sha512_pair(nx[2 * j], nx[2 * j + 1]);
    if (k + 1u < nb) digest_load_block<true, 32>(p, n, k + 1u, nx);   // the next block's loads are in flight while this one is compressed
    sha512_block(st, w);
  }
  sha512_out(r, st[0], st[1]);
  gst(&results[ui], r);
  sha512_out(t, st[2], st[3]);
  gst(&results[ui + 1u], t);
  sha512_out(t, st[4], st[5]);
  gst(&results[ui + 2u], t);
  if (!is384) { sha512_out(t, st[6], st[7]); gst(&results[ui + 3u], t); }
}
