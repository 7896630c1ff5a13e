// crc32_kernel.hpp -- MSPACK_HIP_UF_CRC32: the CRC-32 of a unit's decoded bytes, computed where they lie.
//
// The digest is the OAB block check (reflected polynomial 0xEDB88320, register started at 0xFFFFFFFF, not inverted at the
// end), i.e. zlib.crc32(bytes) ^ 0xFFFFFFFF; it replaces the diagnostic result.in_used of a flagged unit.
//
// CRC is linear over GF(2), and that is the whole design.  Read a message M of n bytes as a polynomial; the register after
// it, started at R, is  R * x^(8n) + M * x^32  (mod P).  So
//   raw(M)            the register started at 0: linear in M, and blind to zero bytes IN FRONT of M;
//   raw(A || B)     = raw(A) * x^(8|B|) + raw(B);
//   digest(M)       = raw(M) + 0xFFFFFFFF * x^(8n)            (the start value is an affine term of its own).
// Registers are bit-reflected: bit 31 is the coefficient of x^0, multiplying by x is a shift to the right.
//
// Work split.  The unit's bytes are read as ALIGNED 16-byte rows: the `head` = out_off & 15 bytes below the unit that share
// its first row count as zeros in front (masked after the load), which raw() does not see.  That stream is cut into
// segments of CRC_SEG bytes, one wavefront each; within a segment every lane runs slice-by-4 (four 256-entry tables in LDS)
// over its own contiguous slice -- all slices of a segment have one length L, a short segment is padded with zero rows IN
// FRONT --, then six levels of ds_bpermute + mulmod fold the 64 lanes with one multiplier x^(8 L 2^k) per level; the up to 15
// bytes behind the last whole row are taken one by one.  A segment's value times x^(8 * bytes behind it) is its share of
// raw(M); a wave XORs its segments' shares into result.in_used with a compare-and-swap loop (XOR commutes: the order of
// arrival does not matter).  mspack_crc32_init, launched in front, has put the affine term there.
//
// CRC_SEG = 64 KiB: a lane's slice of a whole segment is 1 KiB = 64 rows, against which the ~13 multiplications a segment
// ends with (32 shift-and-xor steps each) cost about as many VALU operations as the slices themselves -- half that size
// would spend more on folding than on bytes --, while the units this is for still spread: a 256 KiB OAB block is four
// waves, a CHM reset interval or a CAB folder of two frames one, and a 2 GiB folder 32768.
//
// LDS: t[4][256] u32 = 4 KiB.  ds_read_b32 has 32 banks per group of 32 lanes (bank = dword address mod 32); the index is a
// data byte, so conflicts are the data's -- what the layout can do is keep each table contiguous, so that its 256 entries
// lie on all 32 banks evenly (interleaving the four tables would put a table on 8 of them).
#pragma once
#include "wave_common.hpp"

#define CRC_POLY 0xEDB88320u
#define CRC_ONE  0x80000000u           /* x^0 */
#define CRC_SEG  65536u
#define CRC_ROWS_FULL (CRC_SEG / 1024u) /* rows per lane in a whole segment */

struct CrcShared { u32 t[4][256]; };

// a * b mod P (reflected): shift-and-xor, 32 steps, no branches
__host__ __device__ constexpr u32 crc_mulmod(u32 a, u32 b)
{
  u32 p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}
// x^(8 * 2^k) mod P, k = 0..31: the squares of x^8
static __device__ const u32 crc_x2n8[32] = {
  0x00800000u, 0x00008000u, 0xEDB88320u, 0xB1E6B092u, 0xA06A2517u, 0xED627DAEu, 0x88D14467u, 0xD7BBFE6Au,
  0xEC447F11u, 0x8E7EA170u, 0x6427800Eu, 0x4D47BAE0u, 0x09FE548Fu, 0x83852D0Fu, 0x30362F1Au, 0x7B5A9CC3u,
  0x31FEC169u, 0x9FEC022Au, 0x6C8DEDC4u, 0x15D6874Du, 0x5FDE7A4Eu, 0xBAD90E37u, 0x2E4E5EEFu, 0x4EABA214u,
  0xA8A472C0u, 0x429A969Eu, 0x148D302Au, 0xC40BA6D0u, 0xC4E22C3Cu, 0x40000000u, 0x20000000u, 0x08000000u };
constexpr u32 crc_sq_n(u32 v, int n) { for (int i = 0; i < n; i++) v = crc_mulmod(v, v); return v; }
static_assert(crc_sq_n(CRC_ONE >> 8, 1) == 0x00008000u && crc_sq_n(CRC_ONE >> 8, 2) == 0xEDB88320u &&
              crc_sq_n(CRC_ONE >> 8, 10) == 0x6427800Eu && crc_sq_n(CRC_ONE >> 8, 31) == 0x08000000u, "crc_x2n8");

__device__ __forceinline__ u32 crc_lane(u32 v, u32 l) { return (u32) __builtin_amdgcn_ds_bpermute((int)((l & 63u) << 2), (int) v); }

// x^(8m) mod P, wave-uniform: lane k holds the factor of bit k of m, five levels multiply them up
__device__ __forceinline__ u32 crc_xpow8(u32 m, u32 lane)
{
  u32 v = (lane < 32u && ((m >> (lane & 31u)) & 1u)) ? crc_x2n8[lane & 31u] : CRC_ONE;
  for (u32 o = 16; o >= 1; o >>= 1) v = crc_mulmod(v, crc_lane(v, lane ^ o));
  return rfl(v);
}

__device__ __forceinline__ void crc_build_tables(CrcShared *sh, u32 lane)
{
  for (u32 i = lane; i < 256u; i += WAVE) {
    u32 c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
    sh->t[0][i] = c;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  for (u32 k = 1; k < 4u; k++) {
    for (u32 i = lane; i < 256u; i += WAVE) {
      const u32 v = sh->t[k - 1u][i];
      sh->t[k][i] = (v >> 8) ^ sh->t[0][v & 0xFFu];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
}
// four more bytes (a little-endian dword) into a register
__device__ __forceinline__ u32 crc_dword(const CrcShared *sh, u32 c, u32 w)
{
  c ^= w;
  return sh->t[3][c & 0xFFu] ^ sh->t[2][(c >> 8) & 0xFFu] ^ sh->t[1][(c >> 16) & 0xFFu] ^ sh->t[0][c >> 24];
}

// the bytes the digest covers: what the unit produced, never more than the room it owns
__device__ __forceinline__ u32 crc_unit_len(const mspack_hip_unit &u, const mspack_hip_result *res)
{
  const u32 n = gld(&res->out_len);
  return n < u.out_len ? n : u.out_len;
}
__device__ __forceinline__ bool crc_unit_wanted(const mspack_hip_unit &u)
{
  return (u.flags & MSPACK_HIP_UF_CRC32) != 0u && ((u.kind >= MSPACK_HIP_KIND_MSZIP && u.kind <= MSPACK_HIP_KIND_KWAJ_LZH) || u.kind == MSPACK_HIP_KIND_STORED);
}

// one unit per lane: in_used = 0xFFFFFFFF * x^(8n), the start value's share (all of the digest when n == 0)
__device__ __forceinline__ void crc_init_unit(const mspack_hip_unit &u, mspack_hip_result *res)
{
  const u32 n = crc_unit_len(u, res);
  u32 r = 0xFFFFFFFFu;
  for (u32 k = 0; k < 32u && (n >> k) != 0u; k++)
    if ((n >> k) & 1u) r = crc_mulmod(r, crc_x2n8[k]);
  gst(&res->in_used, r);
}

// raw CRC of bytes [vlo, vhi) of the unit's row-aligned stream (row0 = its first row, `head` masked bytes in front); vlo is
// a multiple of CRC_SEG, vhi - vlo <= CRC_SEG.  Wave-uniform result.
__device__ __forceinline__ u32 crc_segment(const u8 *row0, const u32 head, const u64 vlo, const u64 vhi, const CrcShared *sh, const u32 lane)
{
  const u32 len = (u32)(vhi - vlo), body = len & ~15u, tail = len & 15u;
  u32 c = 0;
  if (body) {
    const bool full = body == CRC_SEG;
    const u32 rows = (body + 1023u) >> 10;                       // 16-byte rows per lane
    const u32 L = rows << 4;
    const int32_t first = (int32_t)(lane * L) - (int32_t)(64u * L - body);      // this lane's first byte; < 0: zero rows in front
    const u8 *seg = row0 + vlo;
    for (u32 r = 0; r < rows; r++) {
      const int32_t off = first + (int32_t)(r << 4);
      uint4 w = make_uint4(0u, 0u, 0u, 0u);
      if (off >= 0) {
        w = gld((const uint4 *)(seg + off));
        if (head != 0u && vlo == 0u && off == 0) {               // the unit's first row: the bytes below out_off count as zeros
          u32 d[4] = { w.x, w.y, w.z, w.w };
          for (u32 k = 0; k < 4u; k++) {
            const u32 lo = 4u * k;
            d[k] = head >= lo + 4u ? 0u : (head > lo ? d[k] & (0xFFFFFFFFu << (8u * (head - lo))) : d[k]);
          }
          w = make_uint4(d[0], d[1], d[2], d[3]);
        }
      }
      c = crc_dword(sh, c, w.x); c = crc_dword(sh, c, w.y); c = crc_dword(sh, c, w.z); c = crc_dword(sh, c, w.w);
    }
    // lanes j and j + 2^k: crc(A || B) = crc(A) * x^(8|B|) + crc(B), |B| = L * 2^k
    u32 m = full ? crc_x2n8[10] : crc_xpow8(L, lane);
    for (u32 k = 0; k < 6u; k++) {
      const u32 hi = crc_lane(c, lane + (1u << k));
      c = crc_mulmod(c, m) ^ hi;
      if (k < 5u) m = full ? crc_x2n8[11u + k] : crc_mulmod(m, m);
    }
    c = rfl(c);
  }
  for (u32 i = 0; i < tail; i++) {                               // behind the last whole row (wave-uniform)
    const u64 pos = vlo + body + i;
    const u32 b = pos >= head ? (u32) gld(row0 + pos) : 0u;
    c = sh->t[0][(c ^ b) & 0xFFu] ^ (c >> 8);
  }
  return c;
}

// wave y of a unit's Y waves: segments y, y + Y, ... -> XORed into in_used
__device__ __forceinline__ void crc_unit_segments(const mspack_hip_unit &u, const u8 *out_arena, mspack_hip_result *res, const u32 y, const u32 Y,
                                                  CrcShared *sh)
{
  const u32 lane = threadIdx.x;
  const u32 n = rfl(crc_unit_len(u, res));
  if (n == 0u) return;
  const u8 *p = out_arena + u.out_off;
  const u32 head = (u32)((size_t) p & 15u);
  const u8 *row0 = p - head;
  const u64 nv = (u64) n + head;
  const u64 nseg = (nv + CRC_SEG - 1u) / CRC_SEG;
  if (y >= nseg) return;
  crc_build_tables(sh, lane);
  u32 acc = 0;
  for (u64 s = y; s < nseg; s += Y) {
    const u64 vlo = s * CRC_SEG, vhi = vlo + CRC_SEG < nv ? vlo + CRC_SEG : nv;
    u32 c = crc_segment(row0, head, vlo, vhi, sh, lane);
    const u32 behind = (u32)(nv - vhi);
    if (behind) c = crc_mulmod(c, crc_xpow8(behind, lane));
    acc ^= c;
  }
  if (lane == 0 && acc != 0u) {
    u32 *w = &res->in_used;
    u32 old = gld(w);
    for (;;) {
      const u32 seen = atomicCAS(w, old, old ^ acc);
      if (seen == old) break;
      old = seen;
    }
  }
}
