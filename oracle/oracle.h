/* oracle/oracle.h -- TEST INFRASTRUCTURE ONLY.  Not part of the product; only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load liboracle.so.
 *
 * A clean-room, buffer-to-buffer CPU restatement of the reference's three stream codecs
 *   lzxd_decompress   (libmspack/mspack/lzxd.c:388-771)
 *   mszipd_decompress (libmspack/mspack/mszipd.c:377-460, inflate :154-316)
 *   qtmd_decompress   (libmspack/mspack/qtmd.c:257-479)
 * including their bit readers (readbits.h:133-214) and the accept/reject behaviour of the
 * canonical-Huffman table builder (readhuff.h:83-176).
 *
 * PARITY PINNING: every function here is checked (tests/test_oracle_vs_ref.py) against the real
 * reference compiled into oracle/_ref/ by oracle/Makefile, on the reference's own known-answer
 * cabinets (libmspack/test/cabd_test.c:405-520 vectors) and on synthetic corpora, and against
 * the committed golden fixtures under tests/golden/.
 */
#ifndef MSPACK_AMD_ORACLE_H
#define MSPACK_AMD_ORACLE_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes: identical values to mspack.h:485-507 */
#define ORC_OK        0
#define ORC_ARGS      1
#define ORC_READ      3
#define ORC_DATAFORMAT 8
#define ORC_DECRUNCH 11

/* result flags */
#define ORC_F_E8_APPLIED      1u  /* at least one frame went through the E8 translation      */
#define ORC_F_LOOKAHEAD_READ  2u  /* LZX: all requested bytes were produced, but the one-frame
                                     look-ahead (lzxd.c:419) then ran out of input (ERR_READ)  */
#define ORC_F_INTEL_HEADER    4u  /* LZX: an interval header carried intel_filesize != 0      */
#define ORC_F_BLOCK_OPEN     16u  /* LZX: the last decoded frame ended inside a block (block_remaining != 0;
                                     at a reset point the reference warns and goes on, lzxd.c:424-431)   */

#define ORC_F_OUT_FULL        8u  /* KWAJ-framed MSZIP: the next block did not fit the room (MSPACK_HIP_F_OUT_FULL)          */

typedef struct oracle_result {
  int32_t  err;       /* MSPACK_ERR_* the reference would return from the decompress call      */
  uint32_t flags;
  uint64_t out_len;   /* bytes the codec handed to sys->write                                   */
  uint64_t in_used;   /* the reference's i_ptr position (bytes pulled into the bit buffer)      */
  uint64_t in_next;   /* LZX: input byte position right after the 16-bit realignment that follows the
                         last completely decoded non-empty frame (lzxd.c:695-697) = where the next frame's
                         bits start; 0 if no frame was completed.
                         Quantum (err 0): bytes decoded beyond the request -- what qtmd keeps in its window (o_end - o_ptr)
                         and hands to the NEXT call's output before it decodes anything (qtmd.c:268-276)          */
} oracle_result;

/* LZX: equivalent to lzxd_init(window_bits, reset_frames, bufsize, length, is_delta=0) followed
 * by one lzxd_decompress(out_bytes).  `e8_base` is the value lzx->offset would have had at the
 * start of this unit if the reference had been decoding since an earlier point (it only shifts
 * the E8 `curpos`, lzxd.c:712).  `out` receives what sys->write would have received. */
int oracle_lzx_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                      uint64_t out_bytes, uint64_t length, int window_bits, int reset_frames,
                      int32_t e8_base, oracle_result *res);
/* the same with LZX DELTA (is_delta: window 2^17..2^25, per-frame chunk size, extended match lengths)
 * and its reference data (lzxd_set_reference_data, lzxd.c:348-382) */
/* For the NEXT decode calls of this thread: the feeder's read fails at in_len (sys->read returns < 0 -- a bad CFDATA block, cabd.c:1322-1324)
 * instead of reporting the end of the input: MSPACK_ERR_READ at once, without the two zero bytes read_input fabricates at a clean end
 * (readbits.h:192-208).  What MSPACK_HIP_UF_HARD_EOF tells the kernels.  0 switches it off again. */
void oracle_set_hard_eof(int on);
/* for the next oracle_qtm_decode() of the calling thread: see qtm_oracle.c */
void oracle_qtm_set_marks(const uint32_t *marks, uint32_t n, uint32_t *log);
/* the reset points (frame indices) at which the last oracle_lzx_decode / oracle_lzxd_decode of THIS thread found a block still
 * open -- lzxd.c:423-431, where the reference warns through sys->message.  Returns how many there were (also beyond cap). */
uint32_t oracle_lzx_open_resets(uint32_t *frames, uint32_t cap);
int oracle_lzxd_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                       uint64_t out_bytes, uint64_t length, int window_bits, int reset_frames,
                       int32_t e8_base, int is_delta, const uint8_t *ref, size_t ref_len, oracle_result *res);

/* MSZIP: mszipd_init(repair_mode) + one mszipd_decompress(out_bytes) over a whole folder stream
 * (concatenated CFDATA payloads).  block_lens (optional, cap entries) receives each block's
 * bytes_output; *n_blocks the number of blocks inflated. */
int oracle_mszip_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                        uint64_t out_bytes, int repair_mode, uint32_t *block_lens, int cap,
                        int *n_blocks, oracle_result *res);

/* MSZIP as KWAJ files frame it: mszipd_init + mszipd_decompress_kwaj (mszipd.c:462-495) over the bytes behind the KWAJ header.
 * `room`: a block is started only with 32768 bytes of it left, else ORC_F_OUT_FULL (the batch ABI's MSPACK_HIP_F_OUT_FULL). */
int oracle_mszip_kwaj_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                             uint64_t room, oracle_result *res);

/* Quantum: qtmd_init(window_bits) + one qtmd_decompress(out_bytes) over a whole folder stream
 * (CFDATA payloads, each followed by the 0xFF trailer cabd.c:1330-1332 injects). */
int oracle_qtm_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                      uint64_t out_bytes, int window_bits, oracle_result *res);

/* make_decode_table accept/reject (readhuff.h:83-176): returns 0 if the reference would accept
 * this set of code lengths for a table with `tablebits` direct bits, 1 if it would reject. */
/* LZSS of SZDD / KWAJ method 2 / MS Help (lzssd.c:36-91); mode 0 EXPAND, 1 MSHELP, 2 QBASIC.  Decoding ends
 * where the input ends; out_len = bytes produced (may exceed out_cap: the excess is dropped). */
int oracle_lzss_decode(const uint8_t *in, size_t in_len, int mode, uint8_t *out, size_t out_cap, oracle_result *res);
/* KWAJ method 3, LZH (kwajd.c:432-563) */
int oracle_kwaj_lzh_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap, oracle_result *res);

int oracle_huff_accepts(const uint8_t *lens, int nsyms, int tablebits);
/* cabd_checksum (cabd.c:1462-1479): the CFDATA checksum of `bytes` bytes with seed `cksum` (cab_oracle.c) */
uint32_t oracle_cab_checksum(const uint8_t *data, size_t bytes, uint32_t cksum);

#ifdef __cplusplus
}
#endif
#endif
