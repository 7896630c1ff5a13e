/* mspack.h -- the libmspack-compatible object API served by the MI355X batch decoder.
 *
 * This is the drop-in surface for programs written against the reference's public header
 * (libmspack/mspack/mspack.h): the same type names, member order and constants for the parts of
 * the API that sit on the LZX / LZX DELTA / Quantum / MSZIP hot path --
 *     struct mspack_system / mspack_file ............ reference mspack.h:285-480
 *     MSPACK_ERR_* ................................... reference mspack.h:485-507
 *     struct mscabd_cabinet / folder / file ......... reference mspack.h:699-916
 *     struct mscab_decompressor (8 methods) ......... reference mspack.h:957-1180
 *     struct mschmd_* / struct mschm_decompressor ... reference mspack.h:1218-1391, 1577-1724
 *     mspack_create/destroy_{cab,chm}_decompressor .. reference mspack.h:522-558
 *     struct msszdd_* / mskwaj_* (5 methods each) ... reference mspack.h:1750-2250
 *     struct msoab_decompressor (3 methods) ......... reference mspack.h:2300-2380
 *     mspack_version, MSPACK_SYS_SELFTEST ........... reference mspack.h:191-262
 * Structure layouts are kept identical so that objects can be exchanged with code compiled
 * against the reference header.  Everything else in the reference header (LIT, HLP and all
 * compressors) is outside this library's scope: the creators for those are not
 * provided.  Behavioural difference, by design: extract() decodes a whole folder / compressed
 * section on the GPU in one batch on first use and serves later extract() calls from that
 * result; outputs and error codes are those of the reference.
 */
#ifndef LIB_MSPACK_H
#define LIB_MSPACK_H 1

#ifdef __cplusplus
extern "C" {
#endif

#include <sys/types.h>
#include <stdlib.h>

/* ---- versioning / self test ---------------------------------------------------------------------- */
#define MSPACK_SYS_SELFTEST(result)  do { \
    (result) = mspack_sys_selftest_internal(sizeof(off_t)); \
} while (0)
extern int mspack_sys_selftest_internal(int);
extern int mspack_version(int entity);

#define MSPACK_VER_LIBRARY   (0)
#define MSPACK_VER_SYSTEM    (1)
#define MSPACK_VER_MSCABD    (2)
#define MSPACK_VER_MSCABC    (3)
#define MSPACK_VER_MSCHMD    (4)
#define MSPACK_VER_MSCHMC    (5)
#define MSPACK_VER_MSLITD    (6)
#define MSPACK_VER_MSLITC    (7)
#define MSPACK_VER_MSHLPD    (8)
#define MSPACK_VER_MSHLPC    (9)
#define MSPACK_VER_MSSZDDD   (10)
#define MSPACK_VER_MSSZDDC   (11)
#define MSPACK_VER_MSKWAJD   (12)
#define MSPACK_VER_MSKWAJC   (13)
#define MSPACK_VER_MSOABD    (14)
#define MSPACK_VER_MSOABC    (15)

/* ---- I/O and memory abstraction -------------------------------------------------------------------- */
struct mspack_file;

struct mspack_system {
  struct mspack_file * (*open)(struct mspack_system *self, const char *filename, int mode);
  void (*close)(struct mspack_file *file);
  int (*read)(struct mspack_file *file, void *buffer, int bytes);
  int (*write)(struct mspack_file *file, void *buffer, int bytes);
  int (*seek)(struct mspack_file *file, off_t offset, int mode);
  off_t (*tell)(struct mspack_file *file);
  void (*message)(struct mspack_file *file, const char *format, ...);
  void * (*alloc)(struct mspack_system *self, size_t bytes);
  void (*free)(void *ptr);
  void (*copy)(void *src, void *dest, size_t bytes);      /* NB: source first */
  void *null_ptr;                                          /* must be NULL */
};

#define MSPACK_SYS_OPEN_READ   (0)
#define MSPACK_SYS_OPEN_WRITE  (1)
#define MSPACK_SYS_OPEN_UPDATE (2)
#define MSPACK_SYS_OPEN_APPEND (3)

#define MSPACK_SYS_SEEK_START  (0)
#define MSPACK_SYS_SEEK_CUR    (1)
#define MSPACK_SYS_SEEK_END    (2)

struct mspack_file { int dummy; };

#define MSPACK_ERR_OK          (0)
#define MSPACK_ERR_ARGS        (1)
#define MSPACK_ERR_OPEN        (2)
#define MSPACK_ERR_READ        (3)
#define MSPACK_ERR_WRITE       (4)
#define MSPACK_ERR_SEEK        (5)
#define MSPACK_ERR_NOMEMORY    (6)
#define MSPACK_ERR_SIGNATURE   (7)
#define MSPACK_ERR_DATAFORMAT  (8)
#define MSPACK_ERR_CHECKSUM    (9)
#define MSPACK_ERR_CRUNCH      (10)
#define MSPACK_ERR_DECRUNCH    (11)

/* ---- CAB ---------------------------------------------------------------------------------------------- */
struct mscab_decompressor;
struct mscabd_folder;
struct mscabd_file;

extern struct mscab_decompressor *mspack_create_cab_decompressor(struct mspack_system *sys);
extern void mspack_destroy_cab_decompressor(struct mscab_decompressor *self);

struct mscabd_cabinet {
  struct mscabd_cabinet *next;
  const char *filename;
  off_t base_offset;
  unsigned int length;
  struct mscabd_cabinet *prevcab;
  struct mscabd_cabinet *nextcab;
  char *prevname;
  char *nextname;
  char *previnfo;
  char *nextinfo;
  struct mscabd_file *files;
  struct mscabd_folder *folders;
  unsigned short set_id;
  unsigned short set_index;
  unsigned short header_resv;
  int flags;
};

#define MSCAB_HDR_RESV_OFFSET (0x28)
#define MSCAB_HDR_PREVCAB (0x01)
#define MSCAB_HDR_NEXTCAB (0x02)
#define MSCAB_HDR_RESV    (0x04)

struct mscabd_folder {
  struct mscabd_folder *next;
  int comp_type;
  unsigned int num_blocks;
};

#define MSCABD_COMP_METHOD(comp_type) ((comp_type) & 0x0F)
#define MSCABD_COMP_LEVEL(comp_type) (((comp_type) >> 8) & 0x1F)
#define MSCAB_COMP_NONE       (0)
#define MSCAB_COMP_MSZIP      (1)
#define MSCAB_COMP_QUANTUM    (2)
#define MSCAB_COMP_LZX        (3)

struct mscabd_file {
  struct mscabd_file *next;
  char *filename;
  unsigned int length;
  int attribs;
  char time_h;
  char time_m;
  char time_s;
  char date_d;
  char date_m;
  int date_y;
  struct mscabd_folder *folder;
  unsigned int offset;
};

#define MSCAB_ATTRIB_RDONLY   (0x01)
#define MSCAB_ATTRIB_HIDDEN   (0x02)
#define MSCAB_ATTRIB_SYSTEM   (0x04)
#define MSCAB_ATTRIB_ARCH     (0x20)
#define MSCAB_ATTRIB_EXEC     (0x40)
#define MSCAB_ATTRIB_UTF_NAME (0x80)

#define MSCABD_PARAM_SEARCHBUF (0)
#define MSCABD_PARAM_FIXMSZIP  (1)
#define MSCABD_PARAM_DECOMPBUF (2)
#define MSCABD_PARAM_SALVAGE   (3)
/* extensions of this library (ids >= 100; the reference answers MSPACK_ERR_ARGS to them) */
#define MSCABD_PARAM_HIP_DEVICES  (100)  /* GPUs to shard a batch over (default 1)               */
#define MSCABD_PARAM_HIP_CACHE_MB (101)  /* decoded-folder cache budget in MiB (default 2048)    */
#define MSCABD_PARAM_HIP_MD5      (102)  /* 1: batches carry one MD5 digest unit per file, for mspack_cabd_md5() (default 0); bit 1
                                            (MSPACK_DIGEST_MD5) of MSCABD_PARAM_HIP_DIGESTS: either one reads and writes it */
#define MSCABD_PARAM_HIP_DIGESTS  (103)  /* a mask of MSPACK_DIGEST_*: the algorithms the batches carry digest units for, per file, for
                                            mspack_cabd_digest() (0 to 7, default 0; other values: MSPACK_ERR_ARGS) */
#define MSCABD_PARAM_HIP_CRC32    (105)  /* 1: batches carry one CRC-32 unit per file, for mspack_cabd_crc32() (0 or 1, default 0; other
                                            values: MSPACK_ERR_ARGS).  104 is not a parameter */
#define MSCABD_PARAM_HIP_DIGESTS64 (106) /* a mask of MSPACK_DIGEST_SHA384 | MSPACK_DIGEST_SHA512: the 64-bit-word algorithms the batches carry
                                            digest units for, per file, for mspack_cabd_digest() (0, 16, 32 or 48, default 0; other
                                            values: MSPACK_ERR_ARGS).  Read where MSCABD_PARAM_HIP_DIGESTS is read; that one keeps
                                            taking 0 to 7 only */
#define MSCABD_PARAM_HIP_STORED   (107)  /* 1: stored ("not compressed") folders are gathered into the batches like compressed ones -- one
                                            MSPACK_HIP_KIND_STORED unit each, their CFDATA checksums verified on the device, their files
                                            in the digest plan -- and served from them (0 or 1, default 0; other values:
                                            MSPACK_ERR_ARGS).  Read when a batch is built.  See mspack_cabd_stored_counts() */
/* digest algorithms (mspack_cabd_digest, MSCABD_PARAM_HIP_DIGESTS, MSCABD_PARAM_HIP_DIGESTS64) */
#define MSPACK_DIGEST_MD5     (1)        /* RFC 1321, 16 bytes */
#define MSPACK_DIGEST_SHA1    (2)        /* FIPS 180-4, 20 bytes */
#define MSPACK_DIGEST_SHA256  (4)        /* FIPS 180-4, 32 bytes */
/* (8 is no algorithm: MSPACK_ERR_ARGS) */
#define MSPACK_DIGEST_SHA384  (16)       /* FIPS 180-4, 48 bytes; its bit belongs to MSCABD_PARAM_HIP_DIGESTS64 / MSCHMD_PARAM_HIP_DIGESTS64 */
#define MSPACK_DIGEST_SHA512  (32)       /* FIPS 180-4, 64 bytes; likewise */

struct mscab_decompressor {
  struct mscabd_cabinet * (*open) (struct mscab_decompressor *self, const char *filename);
  void (*close)(struct mscab_decompressor *self, struct mscabd_cabinet *cab);
  struct mscabd_cabinet * (*search) (struct mscab_decompressor *self, const char *filename);
  int (*append) (struct mscab_decompressor *self, struct mscabd_cabinet *cab, struct mscabd_cabinet *nextcab);
  int (*prepend) (struct mscab_decompressor *self, struct mscabd_cabinet *cab, struct mscabd_cabinet *prevcab);
  int (*extract)(struct mscab_decompressor *self, struct mscabd_file *file, const char *filename);
  int (*set_param)(struct mscab_decompressor *self, int param, int value);
  int (*last_error)(struct mscab_decompressor *self);
};

/* extension of this library (a plain function: struct mscab_decompressor keeps the reference's layout).
 *
 * Gather every not-yet-decoded folder of the given cabinets into ONE GPU batch, so that the extract() calls
 * that follow are slices of it.  Advice: what extract() returns, writes and says is the same with and without it.
 *
 * Without it a batch is formed by the first extract() that touches a cabinet, of that cabinet's folders (or its set's):
 * a directory of thousands of small cabinets is then thousands of batches of one or two folders each.
 *   cabs[i]   cabinets this decompressor opened or found with search().  A member of a set joined with append() / prepend()
 *             stands for the set's folder list; an entry given twice, or two members of one set, are harmless, and so are
 *             folders that are decoded already or part of a batch that is still running.
 *   folders   stored folders are streamed as ever and are left out (unless MSCABD_PARAM_HIP_STORED is 1), as are folders continued from a cabinet that is not
 *             joined; a folder whose cabinet file cannot be opened stays undecoded, and its extract() reports that.
 *             Folders are taken in argument order, then in list order, while their estimated decoded size (32 KiB per CFDATA
 *             block) fits MSCABD_PARAM_HIP_CACHE_MB; the others are decoded on demand by extract().
 *   params    MSCABD_PARAM_FIXMSZIP, _SALVAGE, _DECOMPBUF and _HIP_DEVICES are read when the batch is built, i.e. here (as
 *             a cabinet's first extract() reads them): set them first.
 *   returns   MSPACK_ERR_OK (also for n_cabs == 0 and when nothing is left to decode: no batch is started then);
 *             MSPACK_ERR_ARGS for self == NULL, n_cabs < 0, cabs == NULL with n_cabs > 0 or a NULL entry (nothing is gathered);
 *             MSPACK_ERR_NOMEMORY; MSPACK_ERR_DECRUNCH when the batch call itself failed.  last_error() answers the same.
 * With at least two folders on one device the batch runs as a job: the call returns at once and each extract() waits for
 * its own folder only.  Closing a cabinet while the batch runs takes its folders out of it; the other cabinets' stay. */
extern int mspack_cabd_prefetch(struct mscab_decompressor *self, struct mscabd_cabinet **cabs, int n_cabs);

/* The MD5 of a file: extract() with the writes replaced by a hash -- what `cabextract -t` and package verifiers do with the bytes.
 *   returns   the code extract(file, ...) would return at this point of this decompressor's life, and it COUNTS as that call for
 *             everything that follows: the decompressor's sticky state (a later extract() of the same folder sees what it would
 *             see after an extract() here), Quantum's held-back bytes, the salvage rules, and the lines said through
 *             sys->message -- the same lines, in this call.  It opens no output file and never calls sys->write.
 *   digest    with MSPACK_ERR_OK the MD5 (RFC 1321) of exactly the bytes extract() would have handed to sys->write; with any
 *             other code sixteen zero bytes.  last_error() answers the same.  A NULL argument: MSPACK_ERR_ARGS.
 * With MSCABD_PARAM_HIP_MD5 set to 1 (before the batch is built: the cabinet's first extract() / md5() / mspack_cabd_prefetch())
 * and a batch provider that reports MSPACK_HIP_FEAT_MD5, the batch that decodes the folders carries one digest unit per file and
 * the digests are kept with the folders: md5() of a file that is good as a whole answers from there.  Everything else is hashed
 * on the host: the param off, stored folders (hashed as they stream), files whose call hands over something other than their
 * plain range (a failing call, what Quantum held back), and files too long for one lane of the device (DESIGN.md section 5;
 * MSPACK_HIP_MD5_RATIO).  The digests are the same either way.
 * The price of the param: digest units are through only when the whole batch is, so a batch that carries some does not run as a
 * job -- mspack_cabd_prefetch() and a cabinet's first extract() / md5() then return when every folder of the batch is decoded and
 * its slowest digest lane has ended, instead of at once / when their own folder is through.  Leave the param off for callers
 * that extract. */
extern int mspack_cabd_md5(struct mscab_decompressor *self, struct mscabd_file *file, unsigned char digest[16]);
/* diagnostics: how many successful mspack_cabd_md5() calls of this process were answered from a digest taken on the device
 * (counts[0]) and how many were hashed on the host (counts[1]); counts may be NULL; reset != 0 clears them after reading. */
extern void mspack_cabd_md5_counts(unsigned long long counts[2], int reset);

/* A digest of a file, by algorithm: mspack_cabd_md5() for MD5, SHA-1 and SHA-256 -- what package verifiers of cabinets check today
 * (Authenticode catalogs, update manifests, driver packages).  Everything said of mspack_cabd_md5() holds: the return codes, what the
 * call counts as for the decompressor's sticky state, the lines said through sys->message, no output file, no sys->write.
 *   alg         MSPACK_DIGEST_MD5, _SHA1, _SHA256, _SHA384 or _SHA512 -- one of them; anything else: MSPACK_ERR_ARGS
 *   digest      with MSPACK_ERR_OK the algorithm's 16, 20, 32, 48 or 64 bytes in the standard's byte order; with any other code that many
 *               zero bytes (if they fit)
 *   digest_cap  the room at digest; below the algorithm's length: MSPACK_ERR_ARGS, nothing written
 * With the algorithm's bit set in MSCABD_PARAM_HIP_DIGESTS (before the batch is built, as for MSCABD_PARAM_HIP_MD5) and a batch provider
 * that reports the algorithm's feature bit (MSPACK_HIP_FEAT_MD5 / _SHA1 / _SHA256), the batch carries one digest unit per file and
 * algorithm -- for SHA-1 and SHA-256 with the unit that takes the digest's bytes beyond sixteen behind it (mspack_hip.h:
 * MSPACK_HIP_KIND_DIGEST_MORE) -- and the digests are kept with the folders.  Everything else is hashed on the host by plain-C
 * SHA-1 / SHA-256 with identical results: the bit off, stored folders, failing or partial files, a provider without the feature bit
 * (or without mspack_hip_features() at all), and files too long for one lane of the device -- per algorithm, by that algorithm's
 * own ratio (MSPACK_HIP_SHA1_RATIO, MSPACK_HIP_SHA256_RATIO beside MSPACK_HIP_MD5_RATIO).
 * SHA-384 and SHA-512 work the same way with their bits in MSCABD_PARAM_HIP_DIGESTS64, MSPACK_HIP_FEAT_SHA384 / _SHA512, two / three
 * MSPACK_HIP_KIND_DIGEST_MORE units behind each head, plain-C SHA-384 / SHA-512 on the host and one ratio for both
 * (MSPACK_HIP_SHA512_RATIO: they share a kernel).
 * As with MSCABD_PARAM_HIP_MD5, a batch that carries digest units of any algorithm does not run as a job: it is waited for as a
 * whole.  Leave the bits off for callers that extract. */
extern int mspack_cabd_digest(struct mscab_decompressor *self, struct mscabd_file *file, int alg, unsigned char *digest, size_t digest_cap);
/* mspack_cabd_md5_counts() per algorithm (an unknown alg: zeros) */
extern void mspack_cabd_digest_counts(int alg, unsigned long long counts[2], int reset);
/* The CRC-32 of a file in zlib's convention (zlib.crc32(bytes): polynomial 0xEDB88320 reflected, started at 0xFFFFFFFF, inverted at the
 * end; 0 for no bytes) -- the per-file checksum ZIP, gzip, 7z and PNG store, what a caller who repacks or indexes a cabinet's members
 * needs.  The contract of mspack_cabd_digest(), word for word: the return code is the one extract(file, ...) would give now, the call
 * COUNTS as that extract() (the sticky state, what Quantum held back, the decoder's lifetime, the lines said through sys->message), no
 * output file is opened and sys->write is never called; *crc is the checksum of exactly the bytes extract() would have written when
 * the call succeeds and 0 otherwise; a NULL argument is MSPACK_ERR_ARGS.  CRC-32 is not a fourth MSPACK_DIGEST_* value.
 * With MSCABD_PARAM_HIP_CRC32 set to 1 (before the batch is built, as for MSCABD_PARAM_HIP_MD5) and a batch provider that reports
 * MSPACK_HIP_FEAT_CRC32_RANGES, the batch carries one MSPACK_HIP_KIND_CRC32 unit per file that lies inside its folder -- at ANY
 * length: there is no "too long for one lane" rule, the device spreads a range over the chip (mspack_hip.h) -- and the checksums are
 * kept with the folders beside the digests.  Everything else is computed on the host by a plain-C CRC-32 with the same answers: the
 * param off, stored folders (as they stream), failing or partial calls, what Quantum held back, a provider without the feature bit.
 * As with the other digest units, a batch that carries CRC-32 units does not run as a job. */
extern int mspack_cabd_crc32(struct mscab_decompressor *self, struct mscabd_file *file, unsigned int *crc);
/* diagnostics: successful mspack_cabd_crc32() calls of this process answered from the device (counts[0]) / computed on the host
 * (counts[1]); counts may be NULL; reset != 0 clears them after reading */
extern void mspack_cabd_crc32_counts(unsigned long long counts[2], int reset);
/* Stored folders (CAB method 0) in the batches: MSCABD_PARAM_HIP_STORED.  With 0 -- or a batch provider without
 * mspack_hip_features() / MSPACK_HIP_FEAT_STORED -- a stored folder is streamed as the reference streams it: one sys->seek + sys->read
 * stream per extract(), its checksums verified and its files hashed on the host, no part in mspack_cabd_prefetch().  With 1 a stored
 * folder is gathered like a compressed one by its cabinet's first extract() / md5() / digest() / crc32() and by mspack_cabd_prefetch():
 * its CFDATA payloads are read into the batch's input arena, one MSPACK_HIP_KIND_STORED unit puts them into the folder's place in the
 * output arena, its block parts get the checksum units compressed folders get, its files are counted into the digest plan
 * (MSCABD_PARAM_HIP_MD5 / _DIGESTS / _DIGESTS64 / _HIP_CRC32), it counts against MSCABD_PARAM_HIP_CACHE_MB by its bytes, and the batch
 * runs as a job under the usual conditions.
 * The streamed state machine stays the authority on everything that is not a clean folder: a stored folder is served from the batch
 * only if its unit answered 0, every block read succeeded, every block has cbData == cbUncomp, every checksum matched (or was 0 in the
 * header: the reference skips those), the folder is one the gather takes (not continued from a cabinet that is not joined) and
 * MSCABD_PARAM_SALVAGE is off.  Otherwise its bytes are dropped and every call on it is streamed as with 0 -- also a call for a file
 * in front of the folder's only bad block -- so codes, partial writes and messages of damaged folders are those of the streamed path,
 * not restatements of them.  A file that reaches past the folder's bytes is streamed too.  A served extract() writes the file's slice
 * with the open / write / close calls of the compressed path (runs of 32 KiB); what it returns, what a later call returns and what
 * last_error() says are what they are with 0.
 * The bytes take a detour through the device: extract() of one cabinet is not faster with 1 (README: the measurements).  The param
 * is for callers that want digests or checksums of stored files from the device, and for mspack_cabd_prefetch() over many small
 * cabinets.
 * diagnostics: stored folders of this process that were served from a batch (counts[0]) / that were streamed while the param was 1
 * (counts[1]), each folder once per way; counts may be NULL; reset != 0 clears them after reading. */
extern void mspack_cabd_stored_counts(unsigned long long counts[2], int reset);
/* the value set_param() last stored for a parameter (the defaults before that); MSCABD_PARAM_HIP_MD5 answers bit 1 of
 * MSCABD_PARAM_HIP_DIGESTS.  MSPACK_ERR_ARGS for an unknown parameter or a NULL argument. */
extern int mspack_cabd_get_param(struct mscab_decompressor *self, int param, int *value);

/* ---- CHM ---------------------------------------------------------------------------------------------- */
struct mschm_decompressor;
struct mschmd_header;
struct mschmd_file;

extern struct mschm_decompressor *mspack_create_chm_decompressor(struct mspack_system *sys);
extern void mspack_destroy_chm_decompressor(struct mschm_decompressor *self);

struct mschmd_section {
  struct mschmd_header *chm;
  unsigned int id;
};

struct mschmd_sec_uncompressed {
  struct mschmd_section base;
  off_t offset;
};

struct mschmd_sec_mscompressed {
  struct mschmd_section base;
  struct mschmd_file *content;
  struct mschmd_file *control;
  struct mschmd_file *rtable;
  struct mschmd_file *spaninfo;
};

struct mschmd_header {
  unsigned int version;
  unsigned int timestamp;
  unsigned int language;
  const char *filename;
  off_t length;
  struct mschmd_file *files;
  struct mschmd_file *sysfiles;
  struct mschmd_sec_uncompressed sec0;
  struct mschmd_sec_mscompressed sec1;
  off_t dir_offset;
  unsigned int num_chunks;
  unsigned int chunk_size;
  unsigned int density;
  unsigned int depth;
  unsigned int index_root;
  unsigned int first_pmgl;
  unsigned int last_pmgl;
  unsigned char **chunk_cache;
};

struct mschmd_file {
  struct mschmd_file *next;
  struct mschmd_section *section;
  off_t offset;
  off_t length;
  char *filename;
};

struct mschm_decompressor {
  struct mschmd_header *(*open)(struct mschm_decompressor *self, const char *filename);
  void (*close)(struct mschm_decompressor *self, struct mschmd_header *chm);
  int (*extract)(struct mschm_decompressor *self, struct mschmd_file *file, const char *filename);
  int (*last_error)(struct mschm_decompressor *self);
  struct mschmd_header *(*fast_open)(struct mschm_decompressor *self, const char *filename);
  int (*fast_find)(struct mschm_decompressor *self, struct mschmd_header *chm, const char *filename,
                   struct mschmd_file *f_ptr, int f_size);
};

/* extensions of this library (plain functions: the reference's mschm_decompressor has no set_param and keeps its layout) */
#define MSCHMD_PARAM_HIP_DIGESTS (103)   /* a mask of MSPACK_DIGEST_*: the algorithms a chunk's batch carries digest units for, per file,
                                            for mspack_chmd_digest() (0 to 7, default 0; other values: MSPACK_ERR_ARGS) */
#define MSCHMD_PARAM_HIP_CRC32   (105)   /* 1: a chunk's batch carries one CRC-32 unit per file, for mspack_chmd_crc32() (0 or 1, default 0;
                                            other values: MSPACK_ERR_ARGS).  104 is not a parameter */
#define MSCHMD_PARAM_HIP_DIGESTS64 (106) /* a mask of MSPACK_DIGEST_SHA384 | MSPACK_DIGEST_SHA512: the 64-bit-word algorithms a chunk's batch
                                            carries digest units for (0, 16, 32 or 48, default 0; other values: MSPACK_ERR_ARGS).  Read
                                            where MSCHMD_PARAM_HIP_DIGESTS is read, mspack_chmd_prefetch() included */
/* MSPACK_ERR_ARGS for an unknown parameter or a NULL argument; get_param answers what set_param last stored (the default before that) */
extern int mspack_chmd_set_param(struct mschm_decompressor *self, int param, int value);
extern int mspack_chmd_get_param(struct mschm_decompressor *self, int param, int *value);
/* A digest of a file: extract() with the writes replaced by a hash, the contract of mspack_cabd_digest() above.
 *   returns     the code extract(file, ...) would return at this point of this decompressor's life, and it COUNTS as that call for
 *               everything that follows: the LZX decoder the reference keeps between calls is created, advanced or dropped as by
 *               extract(), the lines said through sys->message ("file is ... bytes longer than ...", the LZX reset warning) are
 *               said in this call, the cache of decoded chunks is used and aged.  It opens no output file and never calls
 *               sys->write.  last_error() answers the same.
 *   alg         MSPACK_DIGEST_MD5, _SHA1, _SHA256, _SHA384 or _SHA512 -- one of them; anything else: MSPACK_ERR_ARGS, nothing written
 *   digest      with MSPACK_ERR_OK the algorithm's 16, 20, 32, 48 or 64 bytes over exactly the bytes extract() would have handed to
 *               sys->write (a file of length 0: the digest of the empty message; files of section 0 are hashed as they are read);
 *               with any other code that many zero bytes (if they fit)
 *   digest_cap  the room at digest; below the algorithm's length: MSPACK_ERR_ARGS, nothing written
 * With the algorithm's bit set in MSCHMD_PARAM_HIP_DIGESTS (SHA-384, SHA-512: in MSCHMD_PARAM_HIP_DIGESTS64) when a chunk of the compressed section is decoded (up to 64 MiB of reset
 * intervals, one GPU batch) and a batch provider that reports the algorithm's feature bit, that batch carries one digest unit per
 * algorithm for every file that lies wholly inside the chunk, and the digests are kept with the chunk, also when its bytes leave
 * the cache.  A call is answered from there when it succeeds and hands over exactly the file's plain range as the chunk holds it.
 * Everything else is hashed on the host with identical results: the bit off, a provider without the feature bit, failing or
 * partial calls, damaged or table-less files (decoded serially), intervals decoded again for another E8 origin, files that cross a
 * chunk boundary or reach past the stream's stated length, and files too long for one lane of the device (the ratios of
 * mspack_cabd_digest: DESIGN.md section 5, MSPACK_HIP_MD5_RATIO / _SHA1_RATIO / _SHA256_RATIO).
 * A chunk batch that carries digest units does not run as a job (as the cabinet driver's): the call that decodes the chunk returns
 * when all of it is decoded and its slowest digest lane has ended.  Leave the bits off for callers that extract. */
extern int mspack_chmd_digest(struct mschm_decompressor *self, struct mschmd_file *file, int alg, unsigned char *digest, size_t digest_cap);
/* diagnostics: how many successful mspack_chmd_digest() calls of this process, of algorithm alg, were answered from a digest taken
 * on the device (counts[0]) and how many were hashed on the host (counts[1]); counts may be NULL; reset != 0 clears them after
 * reading; an unknown alg: zeros */
extern void mspack_chmd_digest_counts(int alg, unsigned long long counts[2], int reset);
/* The CRC-32 of a file in zlib's convention: mspack_cabd_crc32() for CHM files, under the contract of mspack_chmd_digest() word for
 * word (return code, what the call counts as, no output file, no sys->write); *crc is zlib.crc32 of exactly the bytes extract() would
 * have written when the call succeeds and 0 otherwise; a NULL argument is MSPACK_ERR_ARGS.
 * With MSCHMD_PARAM_HIP_CRC32 set to 1 when a chunk is decoded (or gathered by mspack_chmd_prefetch()) and a provider that reports
 * MSPACK_HIP_FEAT_CRC32_RANGES, the chunk's batch carries one MSPACK_HIP_KIND_CRC32 unit for every file that lies wholly inside the
 * chunk, whatever its length; the checksums are kept with the chunk in the table of its digests.  Computed on the host, with the
 * same answers: the param off, a provider without the feature bit, failing or partial calls, damaged (serially decoded) files,
 * shifted E8 origins, files across a chunk boundary.  A batch that carries CRC-32 units does not run as a job. */
extern int mspack_chmd_crc32(struct mschm_decompressor *self, struct mschmd_file *file, unsigned int *crc);
extern void mspack_chmd_crc32_counts(unsigned long long counts[2], int reset);

/* Gather the not-yet-decoded reset intervals of the given CHMs into ONE GPU batch, so that the extract() / mspack_chmd_digest()
 * calls that follow are slices of it.  Advice: what every later extract(), fast_find() + extract() and mspack_chmd_digest() returns,
 * writes, hashes and says through sys->message is the same with and without it -- the LZX decoder the reference keeps between
 * calls, intervals decoded again for a shifted E8 origin, damaged or table-less streams (decoded serially) and files of section 0
 * included.  The call itself says nothing through sys->message and opens no output file.
 *
 * Without it a CHM's compressed section is decoded by the first call that touches it, in batches of that CHM's intervals alone: a
 * collection of thousands of small CHMs is then thousands of batches of two to ten units each.
 *   chms[i]   CHMs this decompressor opened with open() or fast_open(); an entry given twice is harmless.
 *   chunks    The CHMs are taken in argument order, within a CHM its chunks (up to 64 MiB of reset intervals) in stream order:
 *             every chunk whose intervals have reset-table entries, except those that are decoded already or part of a batch that
 *             is still running -- while the decoded bytes gathered by this call plus those the listed CHMs hold already fit
 *             mspack_hip_cache_mb(), and while the batch's input (the CHMs' compressed sections behind one another) stays below
 *             2^34 bytes.  Everything left out is decoded on demand as ever.
 *   setup     A CHM whose compressed section has not been looked at gets that done here (ControlData, ResetTable, SpanInfo and
 *             Content are read).  A CHM for which that fails is left exactly as it was -- no failure is remembered, nothing is said;
 *             its next extract() does it again and reports as ever -- and does not make the call fail.
 *   digests   MSCHMD_PARAM_HIP_DIGESTS is read here: when it is non-zero the batch carries the digest units of every gathered
 *             chunk, kept with that chunk as after a chunk's own batch.
 *   returns   MSPACK_ERR_OK (also for n_chms == 0, when nothing is left to decode and when every CHM was skipped: no batch is
 *             started then); MSPACK_ERR_ARGS for self == NULL, n_chms < 0, chms == NULL with n_chms > 0 or a NULL entry (nothing
 *             is gathered); MSPACK_ERR_NOMEMORY; MSPACK_ERR_DECRUNCH when the batch call itself failed ("GPU batch decode failed:
 *             ..." is said then, and nothing of the batch is kept).  last_error() answers the same.
 * With at least two intervals, one device (mspack_hip_default_devices() <= 1) and no digest units the batch runs as a job: the call
 * returns at once and each later call waits only for the intervals it needs.  Otherwise -- also with MSPACK_HIP_JOBS=0 -- it returns
 * when the batch is through.  A chunk's decoded bytes stay valid until that chunk leaves the cache or its CHM is closed, whatever
 * happens to the other CHMs of the batch.  Closing a CHM while the batch runs takes its intervals out of it; the other CHMs' stay.
 * mspack_destroy_chm_decompressor() settles a batch that is still running. */
extern int mspack_chmd_prefetch(struct mschm_decompressor *self, struct mschmd_header **chms, int n_chms);
/* diagnostics: the batch calls the CHM driver has issued in this process (counts[0]) and the interval units in them (counts[1]) --
 * a chunk's own batch, a serial span, intervals decoded again for another E8 origin and a prefetch batch count alike; counts may be
 * NULL; reset != 0 clears them after reading */
extern void mspack_chmd_batch_counts(unsigned long long counts[2], int reset);

/* ---- SZDD (reference mspack.h:1750-1790, 1876-1975) ------------------------------------------------------ */
#define MSSZDD_FMT_NORMAL (0)
#define MSSZDD_FMT_QBASIC (1)
struct msszddd_header {
  int format;
  off_t length;
  char missing_char;
};
struct msszdd_decompressor {
  struct msszddd_header *(*open)(struct msszdd_decompressor *self, const char *filename);
  void (*close)(struct msszdd_decompressor *self, struct msszddd_header *szdd);
  int (*extract)(struct msszdd_decompressor *self, struct msszddd_header *szdd, const char *filename);
  int (*decompress)(struct msszdd_decompressor *self, const char *input, const char *output);
  int (*last_error)(struct msszdd_decompressor *self);
};
extern struct msszdd_decompressor *mspack_create_szdd_decompressor(struct mspack_system *sys);
extern void mspack_destroy_szdd_decompressor(struct msszdd_decompressor *self);

/* extension of this library (plain functions: the decompressor structs keep the reference's layout).
 *
 * Decode the coded streams of MANY open SZDD files in ONE GPU batch and keep each file's bytes with its header, so that the
 * extract() calls that follow only write.  Advice: what extract() returns, writes, reports through last_error() and says through
 * sys->message is the same with and without it.
 *
 * Without it every extract() is a batch of one unit -- its own launch, arenas and copy back; an installation medium of thousands of
 * `*.ex_` / `*.dl_` files is then thousands of batches.
 *   hdrs[i]   headers this decompressor opened; NULL entries, an entry given twice, a header of another decompressor and a header that
 *             holds its bytes already are skipped.
 *   reads     The call seeks to and reads every member's coded bytes through sys->seek / sys->tell / sys->read: the sys->read calls of
 *             the later extract() have moved HERE.  extract() of a held member calls sys->seek, sys->open, sys->write and sys->close
 *             as ever, and no sys->read.
 *   room      A member's unit gets the length its header states as room when that lies in (0, largest possible expansion], else the
 *             largest possible expansion (what a solitary extract() gives it).  A member whose stream produced more than its room is
 *             decoded again, alone, by its extract() -- today's path; the answer is the same.
 *   left out  A member whose bytes cannot be read, and a member that would push the decoded bytes this decompressor keeps past
 *             mspack_hip_cache_mb(), stay out of the batch: their extract() runs as ever and reports what it reports today.
 *   lifetime  A member's bytes are released by the extract() that writes them (a second extract() of the same header decodes it again,
 *             as ever) or by close(); headers may be closed in any order, also before they are extracted.
 *   returns   MSPACK_ERR_OK (also when nothing was left to decode: no batch is started then); MSPACK_ERR_ARGS for self == NULL,
 *             hdrs == NULL or n <= 0; MSPACK_ERR_NOMEMORY; MSPACK_ERR_DECRUNCH when the batch call itself failed ("GPU batch decode
 *             failed: ..." is said then, and nothing of the batch is kept).  last_error() answers the same.  Synchronous.
 * LZSS members carry MSPACK_HIP_UF_LZSS_RING (no 4096 bytes below the unit) when the provider of the batch ABI reports
 * MSPACK_HIP_FEAT_LZSS_RING.  decompress(input, output) is unchanged: one file, one batch. */
extern int mspack_szddd_prefetch(struct msszdd_decompressor *self, struct msszddd_header **hdrs, int n);
/* diagnostics: counts[0] the batch calls the SZDD driver has issued in this process (a solitary extract() is one, a prefetch is one),
 * counts[1] the extract() calls answered from a prefetch batch, counts[2] the members decoded again alone because they did not fit
 * their room; counts may be NULL; reset != 0 clears them after reading */
extern void mspack_szddd_batch_counts(unsigned long long counts[3], int reset);

/* ---- KWAJ (reference mspack.h:1978-2036, 2156-2250) ----------------------------------------------------- */
#define MSKWAJ_COMP_NONE (0)
#define MSKWAJ_COMP_XOR (1)
#define MSKWAJ_COMP_SZDD (2)
#define MSKWAJ_COMP_LZH (3)
#define MSKWAJ_COMP_MSZIP (4)
#define MSKWAJ_HDR_HASLENGTH (0x01)
#define MSKWAJ_HDR_HASUNKNOWN1 (0x02)
#define MSKWAJ_HDR_HASUNKNOWN2 (0x04)
#define MSKWAJ_HDR_HASFILENAME (0x08)
#define MSKWAJ_HDR_HASFILEEXT (0x10)
#define MSKWAJ_HDR_HASEXTRATEXT (0x20)
struct mskwajd_header {
  unsigned short comp_type;
  off_t data_offset;
  int headers;
  off_t length;
  char *filename;
  char *extra;
  unsigned short extra_length;
};
struct mskwaj_decompressor {
  struct mskwajd_header *(*open)(struct mskwaj_decompressor *self, const char *filename);
  void (*close)(struct mskwaj_decompressor *self, struct mskwajd_header *kwaj);
  int (*extract)(struct mskwaj_decompressor *self, struct mskwajd_header *kwaj, const char *filename);
  int (*decompress)(struct mskwaj_decompressor *self, const char *input, const char *output);
  int (*last_error)(struct mskwaj_decompressor *self);
};
extern struct mskwaj_decompressor *mspack_create_kwaj_decompressor(struct mspack_system *sys);
extern void mspack_destroy_kwaj_decompressor(struct mskwaj_decompressor *self);
/* mspack_szddd_prefetch for KWAJ files, every word of it: methods 2 (LZSS), 3 (LZH) and 4 (MSZIP) go into the same batch -- LZH keeps
 * its 4096 bytes below the unit, MSZIP its 32 KiB of slack and a room rounded up to whole 32 KiB blocks (the decoder starts a block only
 * with a whole block of room left); a header's length counts when MSKWAJ_HDR_HASLENGTH is set; LZH and MSZIP
 * members answer their unit's error code behind the bytes they produced, as their extract() does today.  Methods 0 and 1 (stored)
 * and unknown methods are left to extract() as ever. */
extern int mspack_kwajd_prefetch(struct mskwaj_decompressor *self, struct mskwajd_header **hdrs, int n);
extern void mspack_kwajd_batch_counts(unsigned long long counts[3], int reset);
/* diagnostic: the LZSS members of both drivers' prefetch batches that went out with MSPACK_HIP_UF_LZSS_RING; reset != 0 clears it */
extern unsigned long long mspack_szdd_kwaj_ring_units(int reset);

/* ---- OAB (Offline Address Book, LZX DELTA) -------------------------------------------------------------- */
/* reference mspack.h:663-683, 2300-2380 */
struct msoab_decompressor {
  int (*decompress) (struct msoab_decompressor *self, const char *input, const char *output);
  int (*decompress_incremental) (struct msoab_decompressor *self, const char *input, const char *base,
                                 const char *output);
  int (*set_param)(struct msoab_decompressor *self, int param, int value);
};
#define MSOABD_PARAM_DECOMPBUF (0)

extern struct msoab_decompressor *mspack_create_oab_decompressor(struct mspack_system *sys);
extern void mspack_destroy_oab_decompressor(struct msoab_decompressor *self);

/* extension of this library (plain functions: the decompressor struct keeps the reference's layout).
 *
 * Decompress MANY address-book files in as few GPU batches as their order allows.  Each job, called alone through decompress() /
 * decompress_incremental() and in the same order, would return some value, write some bytes to its output file and say some lines
 * through sys->message: after the call jobs[k].error holds that value, the output file holds exactly those bytes (a failing job's
 * partial output included) and the lines are the same lines.
 *
 * Without it every file is a batch of its own -- planning, copies, launches and the drain for a block or two of LZX DELTA; one address
 * list is a data file plus dozens of per-language templates, a catch-up is a chain of daily patches, a mirror serves many lists.
 *   jobs[k]   input, output; base == NULL: a full file (decompress), else decompress_incremental's base.
 *   steps     Each job is GATHERED (input and base opened, headers checked, the blocks' bytes and their reference slices read, both
 *             closed again); the blocks of all gathered jobs are DECODED in one batch; the jobs are REPLAYED in order (output opened,
 *             blocks written, CRCs compared, output closed).  No more than three files are open at any time, whatever n is.  A job
 *             whose input, header or base fails at gather contributes nothing to the batch and its output is not created, as ever.
 *   a batch ends, and is decoded and replayed before the next job is gathered,
 *     order   when that job's `input` or `base` is the `output` of a job in the batch: base + patch1 -> v2, v2 + patch2 -> v3 in one
 *             call behaves as the calls in order do.  Only IDENTICAL strings (strcmp) are recognised: two spellings of one file are
 *             not, and such jobs belong into separate calls.  (A job whose `output` is its own `input` or `base` runs alone.)
 *     budget  when that job would take the batch's input plus output arena past mspack_hip_cache_mb() MiB: it starts the next batch.
 *             A job that passes the budget alone runs alone, as ever.
 *   failure   When mspack_hip_decode_batch() fails for a batch of several jobs, each of them is decoded again in a batch of its own:
 *             only a job whose OWN batch fails says "GPU batch decode failed: ..." and answers MSPACK_ERR_DECRUNCH.
 *   returns   MSPACK_ERR_ARGS for self == NULL, n < 0, jobs == NULL with n > 0, or a job without input or output (no job is started
 *             then); MSPACK_ERR_NOMEMORY when the call's own tables cannot be allocated; else MSPACK_ERR_OK, whatever the jobs'
 *             own answers are.  n == 0 issues nothing.  MSOABD_PARAM_DECOMPBUF applies to every job.  Synchronous. */
struct msoabd_job {
  const char *input;    /* the .LZX file                                            */
  const char *base;     /* NULL: a full file (decompress); else decompress_incremental's base */
  const char *output;
  int error;            /* out: what decompress() / decompress_incremental() returns for this job alone */
};
extern int mspack_oabd_decompress_many(struct msoab_decompressor *self, struct msoabd_job *jobs, int n);
/* diagnostics: counts[0] the batch calls the OAB driver has issued in this process (a lone decompress() with a compressed block is
 * one), counts[1] the jobs whose blocks went out in a batch built by mspack_oabd_decompress_many, counts[2] the jobs decoded again
 * alone because their shared batch failed; counts may be NULL; reset != 0 clears them after reading */
extern void mspack_oabd_batch_counts(unsigned long long counts[3], int reset);

#ifdef __cplusplus
}
#endif
#endif
