/* chmd.c -- CHM driver of the libmspack-compatible API (include/mspack.h), on the GPU batch decoder.
 *
 * Mirrors the behaviour of the reference's chmd.c for open / fast_open / fast_find / extract:
 *   ITSF + header sections + PMGL directory parsing and its error codes .. chmd.c:254-532
 *   section-0 (stored) files: seek + copy ................................. chmd.c:958-987
 *   ControlData / ResetTable / SpanInfo -> window, reset interval, length .. chmd.c:1072-1315
 *   lzxd lifetime: a decoder lives from the reset point of the first file it was asked for until an
 *   error or a backwards request (chmd.c:989-1040); errors of any frame it has to cross are reported
 * but NOT its control flow: every LZX reset interval (chmd.c:1147-1149) is an independent unit, so
 * the first section-1 extract() decodes ALL intervals of the CHM in one GPU batch and later
 * extract() calls are slices of that result.  The reference's decoder lifetime is emulated on top
 * (virtual start / position), because it decides (a) which frames' errors a request sees and (b) the
 * origin of the E8 translation (lzxd.c:712 uses bytes since lzxd_init): intervals whose header asks
 * for E8 are re-decoded with the origin the reference would have had.
 * fast_find follows the reference: PMGI index descent, quick-reference binary
 * search inside a chunk, UTF-8 case-folded name order (chmd.c:543-898).
 * mspack_chmd_digest (mspack.h) is extract() with another sink: the same body, the slices hashed instead of written.  With
 * MSCHMD_PARAM_HIP_DIGESTS a chunk's batch also carries one digest unit per algorithm for every file that lies wholly inside the
 * chunk (host_digest.h: chm_digest_plan, over the emitter the cabinet driver uses); their answers are kept with the chunk in the
 * table both drivers use (digest_table_harvest / digest_table_find) and answer the calls that hand over exactly the file's plain
 * range.  A chunk batch that carries digest units is NOT run as a job -- digest units are through only when the whole
 * batch is (mspack_hip.h), the decision the cabinet driver takes in decode_cabinets -- so the first call into such a chunk
 * returns when every interval of it is decoded and its slowest digest lane has ended.
 * Chunks are decoded by ONE mechanism: a struct chm_batch, issued by issue_batch() from a list of chunks.  extract() issues a batch
 * of the one chunk it needs (ensure_chunk_to), reading the CHM's own arena; mspack_chmd_prefetch (mspack.h) issues ONE batch over
 * the not-yet-decoded chunks of MANY CHMs before the first extract(), reading a copy of every CHM's arena behind one another.
 * Either way the output is one buffer the batch's chunks point into, and waiting, eviction, close() and destroy go the same way.
 */
#include <stdlib.h>
#include <stdio.h>
#include "host_common.h"
#include "host_digest.h"

#define FRAME 32768

static const char content_name[]  = "::DataSpace/Storage/MSCompressed/Content";
static const char control_name[]  = "::DataSpace/Storage/MSCompressed/ControlData";
static const char spaninfo_name[] = "::DataSpace/Storage/MSCompressed/SpanInfo";
static const char rtable_name[]   = "::DataSpace/Storage/MSCompressed/Transform/"
                                    "{7FC28940-9D31-11D0-9B27-00A0C91E9C7C}/InstanceData/ResetTable";

struct chm_chunk {                /* a run of reset intervals, decoded together as one member of a batch (struct chm_batch) */
  unsigned char *buf;             /* decoded bytes (E8 origin 0): a place in its batch's output buffer; NULL when evicted */
  unsigned long stamp;            /* LRU clock                                                      */
  int res_valid;                  /* ires[] of these intervals is filled in                         */
  /* the batch that decoded the chunk, for as long as buf points into its output (bat != NULL exactly while buf != NULL: the bytes
   * are given back to the batch, never freed); bat_k: which of its members; bat_run: the batch still runs as a job (mspack_hip.h)
   * and this chunk has not taken all of its units -- of buf and ires[] only what chunk_wait() has covered may be read then */
  struct chm_batch *bat; size_t bat_k; int bat_run;
  unsigned int job_waited;        /* units [0, job_waited) of the chunk have come through            */
  /* MSCHMD_PARAM_HIP_DIGESTS: the digests the chunk's batches took of its files, by offset in the stream (host_digest.h: struct
   * digest_table); dg_algs: the algorithms a batch of this chunk has carried units for.  Kept when buf is evicted; freed with section 1 */
  struct digest_table dg; int dg_algs;
};
struct chm_p {
  struct mschmd_header base;
  /* section 1 */
  int sec1_state;                 /* 0 = not set up, 1 = ready, <0 = -(setup error)                 */
  int window_bits;
  unsigned int fper;              /* frames per reset interval                                      */
  off_t interval_bytes, padded_len;
  unsigned int n_intervals;       /* padded_len / interval_bytes                                    */
  unsigned int n_fast;            /* intervals [0, n_fast) have a reset-table entry                 */
  int span_err; off_t span_len;   /* SpanInfo: the fallback stream length (chmd.c:1159-1166)        */
  unsigned char *arena; size_t arena_len;     /* the CHM file from the start of Content to its end  */
  int arena_pinned;                           /* page-locked (mspack_hip_pin) until free_sec1                */
  off_t content_start;            /* file offset of the Content stream                              */
  uint64_t *ioff;                 /* reset-table entry (compressed offset) of intervals [0, n_fast)  */
  size_t ftab_off;                /* arena offset of the per-frame tables (0: none), n_fast * fper uint32: every
                                     frame's compressed offset from its interval's start (MSPACK_HIP_UF_FRAME_TABLE) */
  size_t arena_room;              /* bytes of the arena buffer that belong to the batch decoder's input arena */
  mspack_hip_result *ires;        /* stand-alone result per interval                                */
  struct chm_chunk *chunks; unsigned int n_chunks, chunk_int; unsigned long stamp;
  /* the section-1 files of chm->files with length > 0, ascending by offset: one walk of the list, when section 1 is set up
   * (fast_open lists no files: none) -- what chm_digest_plan picks a chunk's digest units from */
  struct chm_digest_file *dfiles; size_t n_dfiles;
  /* the serial span of the virtual decoder (damaged / table-less files) */
  int s_valid, s_mode; off_t s_init, s_cover; unsigned char *s_buf; mspack_hip_result s_res;
  unsigned int s_log_n, s_log_cap;     /* the serial span's reset log (MSPACK_HIP_UF_LZX_LOG): frames, counted from s_init, whose
                                          reset found a block open; it lies in s_buf behind the span (s_log) */
  const unsigned char *s_log;
  unsigned int pf_stamp;          /* mspack_chmd_prefetch: chmd_p.pf_stamp of the call that last saw this CHM (an entry given twice) */
};
struct vdec {                     /* the reference's lzxd instance, replayed (chmd.c:989-1040)       */
  int alive, mode, serial, seek_pending;   /* mode 0: created at a reset-table entry, 1: at offset 0 with SpanInfo */
  off_t init, length, offset;     /* creation point, stream length it was created with, position    */
  off_t dlen;                     /* the reference's d->length (chmd.c:1176): what extract() checks offsets and lengths against.
                                     == length, except for a decoder created exactly AT the stream's stated end: lzxd_init then
                                     gets an output length of 0, which means "not known" (lzxd.c:419, 458-461) -- it decodes
                                     whatever frames follow, for as long as the input lasts */
  off_t decoded_end;              /* end of the last frame it has decoded: [offset, decoded_end) is stored
                                     up in its window and handed out without decoding (lzxd.c:397-408)  */
  uint64_t in_off;                /* compressed offset it was created at                            */
};
struct chmd_p {
  struct mschm_decompressor base;
  struct mspack_system *system;
  int error;
  struct chm_p *v_chm; struct vdec v;
  int hip_digests;                    /* MSCHMD_PARAM_HIP_DIGESTS: a mask of MSPACK_DIGEST_* */
  int hip_digests64;                  /* MSCHMD_PARAM_HIP_DIGESTS64: a mask of MSPACK_DIGEST_SHA384 | MSPACK_DIGEST_SHA512 */
  int hip_crc32;                      /* MSCHMD_PARAM_HIP_CRC32: 1 = a chunk's batch carries one MSPACK_HIP_KIND_CRC32 unit per file, for mspack_chmd_crc32() */
  struct digest_sink *sink;           /* mspack_chmd_digest is running: what extract() would write goes here instead of a file */
  int sink_whole;                     /* ... and the emit step hands over exactly the file's plain range, of a call that is good so far */
  const unsigned char *sink_kept;     /* ... and that file's digest was taken by its chunk's batch: this one */
  struct chm_batch *batches;          /* the batches that still run or whose output buffer still has users */
  unsigned int pf_stamp;              /* mspack_chmd_prefetch: one number per call */
};
/* per algorithm, successful mspack_chmd_digest() calls answered from a device digest / hashed on the host (mspack.h) */
static unsigned long long g_digest_counts[DIGEST_ALGS][2];
static unsigned long long g_crc32_counts[2];            /* the same for mspack_chmd_crc32() */
/* the algorithms asked for, CRC-32 (host_digest.h: DIGEST_ALG_CRC32) among them */
#define CHM_ASKED_ALGS(self) ((self)->hip_digests | (self)->hip_digests64 | ((self)->hip_crc32 ? DIGEST_ALG_CRC32 : 0))
/* batch calls this driver has issued, and the interval units in them (mspack.h: mspack_chmd_batch_counts) */
static unsigned long long g_batch_counts[2];
static void count_batch(size_t n_intervals)
{
  __atomic_fetch_add(&g_batch_counts[0], 1ull, __ATOMIC_RELAXED);
  __atomic_fetch_add(&g_batch_counts[1], (unsigned long long) n_intervals, __ATOMIC_RELAXED);
}

static off_t read_encint(const unsigned char **p, const unsigned char *end, int *err) {
  off_t v = 0; unsigned char c = 0x80; int i = 0;
  while ((c & 0x80) && (i++ < 9)) {
    if (*p >= end) { *err = 1; return 0; }
    c = *(*p)++;
    v = (v << 7) | (c & 0x7F);
  }
  if (i == 9 && (c & 0x80)) { *err = 1; return 0; }
  return v;
}

/* ---- headers (reference chmd.c:254-532) ------------------------------------------------------------- */
static const unsigned char itsf_guids[32] = {
  0x10, 0xFD, 0x01, 0x7C, 0xAA, 0x7B, 0xD0, 0x11, 0x9E, 0x0C, 0x00, 0xA0, 0xC9, 0x22, 0xE6, 0xEC,
  0x11, 0xFD, 0x01, 0x7C, 0xAA, 0x7B, 0xD0, 0x11, 0x9E, 0x0C, 0x00, 0xA0, 0xC9, 0x22, 0xE6, 0xEC
};

static int read_headers(struct mspack_system *sys, struct mspack_file *fh, struct mschmd_header *chm, int entire)
{
  unsigned char buf[0x54], *chunk;
  struct mschmd_file *tail = NULL;
  off_t off_hs0, filelen;
  unsigned int n, errors = 0;
  /* the reference keeps ONE bad-ENCINT flag for the whole listing (chmd.c:262, never cleared): after the first badly encoded
   * integer every later chunk ends at its first entry -- nothing more is listed (found by tools/fuzz_chmdir_cpu.py) */
  int err = 0;

  chm->files = NULL; chm->sysfiles = NULL; chm->chunk_cache = NULL;
  chm->sec0.base.chm = chm; chm->sec0.base.id = 0;
  chm->sec1.base.chm = chm; chm->sec1.base.id = 1;
  chm->sec1.content = chm->sec1.control = chm->sec1.spaninfo = chm->sec1.rtable = NULL;

  if (sys->read(fh, buf, 0x38) != 0x38) return MSPACK_ERR_READ;
  if (rd_le32(buf) != 0x46535449u) return MSPACK_ERR_SIGNATURE;
  if (memcmp(buf + 0x18, itsf_guids, 32) != 0) return MSPACK_ERR_SIGNATURE;
  chm->version = rd_le32(buf + 4);
  chm->timestamp = rd_be32(buf + 0x10);
  chm->language = rd_le32(buf + 0x14);
  if (chm->version > 3) sys->message(fh, "WARNING; CHM version > 3");
  if (sys->read(fh, buf, 0x28) != 0x28) return MSPACK_ERR_READ;
  off_hs0 = (off_t) rd_le64(buf);
  chm->dir_offset = (off_t) rd_le64(buf + 0x10);
  chm->sec0.offset = (off_t) rd_le64(buf + 0x20);
  if (sys->seek(fh, off_hs0, MSPACK_SYS_SEEK_START)) return MSPACK_ERR_SEEK;
  if (sys->read(fh, buf, 0x18) != 0x18) return MSPACK_ERR_READ;
  chm->length = (off_t) rd_le64(buf + 8);
  if (!mspack_sys_filelen(sys, fh, &filelen)) {
    if (chm->length > filelen) sys->message(fh, "WARNING; file possibly truncated by %lld bytes", (long long)(chm->length - filelen));
    else if (chm->length < filelen) sys->message(fh, "WARNING; possible %lld extra bytes at end of file", (long long)(filelen - chm->length));
  }
  if (sys->seek(fh, chm->dir_offset, MSPACK_SYS_SEEK_START)) return MSPACK_ERR_SEEK;
  if (sys->read(fh, buf, 0x54) != 0x54) return MSPACK_ERR_READ;
  chm->dir_offset = sys->tell(fh);
  chm->chunk_size = rd_le32(buf + 0x10);
  chm->density = rd_le32(buf + 0x14);
  chm->depth = rd_le32(buf + 0x18);
  chm->index_root = rd_le32(buf + 0x1C);
  chm->first_pmgl = rd_le32(buf + 0x20);
  chm->last_pmgl = rd_le32(buf + 0x24);
  chm->num_chunks = rd_le32(buf + 0x2C);
  if (chm->version < 3) chm->sec0.offset = chm->dir_offset + ((off_t) chm->chunk_size * chm->num_chunks);
  if (chm->sec0.offset > chm->length) return MSPACK_ERR_DATAFORMAT;
  if (chm->chunk_size < 0x14 + 2) return MSPACK_ERR_DATAFORMAT;
  if (chm->num_chunks == 0) return MSPACK_ERR_DATAFORMAT;
  if (chm->num_chunks > 100000) return MSPACK_ERR_DATAFORMAT;
  if (chm->chunk_size > 8192) return MSPACK_ERR_DATAFORMAT;
  if ((off_t) chm->chunk_size * (off_t) chm->num_chunks > chm->length) return MSPACK_ERR_DATAFORMAT;
  if (chm->chunk_size != 4096) sys->message(fh, "WARNING; chunk size is not 4096");
  if (chm->first_pmgl != 0) sys->message(fh, "WARNING; first PMGL chunk is not zero");
  if (chm->first_pmgl > chm->last_pmgl) return MSPACK_ERR_DATAFORMAT;
  if (chm->index_root != 0xFFFFFFFFu && chm->index_root >= chm->num_chunks) return MSPACK_ERR_DATAFORMAT;
  if (!entire) return MSPACK_ERR_OK;

  if (chm->first_pmgl != 0 && sys->seek(fh, (off_t) chm->first_pmgl * (off_t) chm->chunk_size, MSPACK_SYS_SEEK_CUR))
    return MSPACK_ERR_SEEK;
  n = chm->last_pmgl - chm->first_pmgl + 1;
  if (!(chunk = (unsigned char *) sys->alloc(sys, chm->chunk_size))) return MSPACK_ERR_NOMEMORY;
  while (n--) {
    const unsigned char *p, *end;
    int entries;
    if (sys->read(fh, chunk, (int) chm->chunk_size) != (int) chm->chunk_size) { sys->free(chunk); return MSPACK_ERR_READ; }
    if (rd_le32(chunk) != 0x4C474D50u) continue;                          /* PMGL only */
    if (rd_le32(chunk + 4) < 2) sys->message(fh, "WARNING; PMGL quickref area is too small");
    if (rd_le32(chunk + 4) > chm->chunk_size - 0x14) sys->message(fh, "WARNING; PMGL quickref area is too large");
    p = chunk + 0x14; end = chunk + chm->chunk_size - 2;
    entries = (int) rd_le16(end);
    while (entries--) {
      unsigned int name_len, section;
      const unsigned char *name;
      off_t offset, length;
      struct mschmd_file *fi;
      name_len = (unsigned int) read_encint(&p, end, &err);
      if (err || name_len > (unsigned int)(end - p)) break;
      name = p; p += name_len;
      section = (unsigned int) read_encint(&p, end, &err);
      offset = read_encint(&p, end, &err);
      length = read_encint(&p, end, &err);
      if (err) break;
      if (name_len < 2 || !name[0] || !name[1]) continue;
      if (offset == 0 && length == 0 && name[name_len - 1] == '/') continue;
      if (section > 1) { sys->message(fh, "invalid section number '%u'.", section); continue; }
      if (!(fi = (struct mschmd_file *) sys->alloc(sys, sizeof(*fi) + name_len + 1))) { sys->free(chunk); return MSPACK_ERR_NOMEMORY; }
      fi->next = NULL;
      fi->filename = (char *) &fi[1];
      fi->section = section ? (struct mschmd_section *) &chm->sec1 : (struct mschmd_section *) &chm->sec0;
      fi->offset = offset; fi->length = length;
      sys->copy((void *) name, fi->filename, name_len);
      fi->filename[name_len] = 0;
      if (name[0] == ':' && name[1] == ':') {
        if (name_len == 40 && !memcmp(name, content_name, 40)) chm->sec1.content = fi;
        else if (name_len == 44 && !memcmp(name, control_name, 44)) chm->sec1.control = fi;
        else if (name_len == 41 && !memcmp(name, spaninfo_name, 41)) chm->sec1.spaninfo = fi;
        else if (name_len == 105 && !memcmp(name, rtable_name, 105)) chm->sec1.rtable = fi;
        fi->next = chm->sysfiles; chm->sysfiles = fi;
      }
      else { if (tail) tail->next = fi; else chm->files = fi; tail = fi; }
    }
    if (entries >= 0) errors++;
  }
  sys->free(chunk);
  return errors ? MSPACK_ERR_DATAFORMAT : MSPACK_ERR_OK;
}

static void free_sec1(struct mspack_system *sys, struct chm_p *c);

static void chmd_close(struct mschm_decompressor *base, struct mschmd_header *chm)
{
  struct chmd_p *self = (struct chmd_p *) base;
  struct mspack_system *sys;
  struct mschmd_file *fi, *nfi;
  unsigned int i;
  if (!self) return;
  sys = self->system;
  self->error = MSPACK_ERR_OK;
  if (!chm) return;
  for (fi = chm->files; fi; fi = nfi) { nfi = fi->next; sys->free(fi); }
  for (fi = chm->sysfiles; fi; fi = nfi) { nfi = fi->next; sys->free(fi); }
  if (self->v_chm == (struct chm_p *) chm) { self->v_chm = NULL; self->v.alive = 0; }
  if (chm->chunk_cache) {
    for (i = 0; i < chm->num_chunks; i++) sys->free(chm->chunk_cache[i]);
    sys->free(chm->chunk_cache);
  }
  free_sec1(sys, (struct chm_p *) chm);
  sys->free(chm);
}

static struct mschmd_header *open_common(struct mschm_decompressor *base, const char *filename, int entire)
{
  struct chmd_p *self = (struct chmd_p *) base;
  struct mspack_system *sys;
  struct mspack_file *fh;
  struct chm_p *c = NULL;
  if (!self) return NULL;
  sys = self->system;
  if (!(fh = sys->open(sys, filename, MSPACK_SYS_OPEN_READ))) { self->error = MSPACK_ERR_OPEN; return NULL; }
  if ((c = (struct chm_p *) sys->alloc(sys, sizeof(*c)))) {
    int err;
    memset(c, 0, sizeof(*c));
    c->base.filename = filename;
    err = read_headers(sys, fh, &c->base, entire);
    if (err) {
      /* like the reference: a badly encoded directory that yielded SOME entries is returned with a
       * warning and no error (chmd.c:166-176) */
      if (err == MSPACK_ERR_DATAFORMAT && (c->base.files || c->base.sysfiles)) {
        sys->message(fh, "WARNING; contents are corrupt");
        err = MSPACK_ERR_OK;
      }
      else { chmd_close(base, &c->base); c = NULL; }
    }
    self->error = err;
  }
  else self->error = MSPACK_ERR_NOMEMORY;
  sys->close(fh);
  return (struct mschmd_header *) c;
}
static struct mschmd_header *chmd_open(struct mschm_decompressor *b, const char *f) { return open_common(b, f, 1); }
static struct mschmd_header *chmd_fast_open(struct mschm_decompressor *b, const char *f) { return open_common(b, f, 0); }

/* ---- fast_find (reference chmd.c:543-898) --------------------------------------------------------------
 * Descends the PMGI index (when the header names an index root) to the PMGL chunk that can hold the
 * name, or walks the PMGL chain otherwise.  Inside a chunk: binary search over the quick-reference
 * entries (one per 1 + 2^density directory entries), then a linear scan of that group.  Names compare
 * as UTF-8 code points, case-insensitively through towlower(), lengths breaking ties -- the same
 * order the directory is sorted in.  Chunks are cached in chm->chunk_cache. */
#include <wctype.h>

/* ---- names ------------------------------------------------------------------------------------------------
 * Directory names are UTF-8 and the directory is sorted by their code points after simple case folding.  The decoder
 * below has to accept exactly what the reference's accepts (chmd.c:861-880: lead bytes C2..DF / E0..EF / F0..F5, no
 * check of the continuation bytes, U+FFFD for everything else and for a sequence the name is too short for), or a
 * damaged name would be looked for in another place than the reference looks. */
struct cp_cursor { const unsigned char *at, *stop; };

static unsigned int cp_take(struct cp_cursor *cur)
{
  const unsigned int lead = *cur->at++;
  unsigned int more, cp, i;
  if (lead < 0x80u) return lead;
  if (lead >= 0xC2u && lead <= 0xDFu) { more = 1; cp = lead & 0x1Fu; }
  else if (lead >= 0xE0u && lead <= 0xEFu) { more = 2; cp = lead & 0x0Fu; }
  else if (lead >= 0xF0u && lead <= 0xF5u) { more = 3; cp = lead & 0x07u; }
  else return 0xFFFDu;
  if ((size_t)(cur->stop - cur->at) < more) return 0xFFFDu;     /* cut short: one byte consumed */
  for (i = 0; i < more; i++) cp = (cp << 6) | (*cur->at++ & 0x3Fu);
  return cp > 0x10FFFFu ? 0xFFFDu : cp;
}

/* < 0, 0, > 0: `want` sorts before / equals / sorts after `have`.  Code points that differ are compared after
 * towlower(); when one name is a prefix of the other the shorter one sorts first (byte lengths). */
static int name_order(const char *want, int want_len, const unsigned char *have, int have_len)
{
  struct cp_cursor a, b;
  a.at = (const unsigned char *) want; a.stop = a.at + want_len;
  b.at = have; b.stop = have + have_len;
  while (a.at < a.stop && b.at < b.stop) {
    const unsigned int x = cp_take(&a), y = cp_take(&b);
    if (x != y) {
      const int fx = (int) towlower((wint_t) x), fy = (int) towlower((wint_t) y);
      if (fx != fy) return fx - fy;
    }
  }
  return want_len - have_len;
}

/* ---- directory chunks --------------------------------------------------------------------------------------
 * A chunk (chm->chunk_size bytes): "PMGL" + free-space length at 4 (+ prev / next chunk numbers at
 * 0xC / 0x10, entries from 0x14) or "PMGI" + free-space length at 4 (entries from 8).  The entries are packed from the
 * front -- ENCINT name length, name, then for PMGL three ENCINTs (section, offset, length), for PMGI one (the child
 * chunk) -- and the chunk ENDS with a 16-bit entry count preceded by the quick-reference table growing downwards: the
 * i-th word below the count is the offset, from the first entry, of entry i * (1 + 2^density). */
static unsigned char *chunk_get(struct chmd_p *self, struct mschmd_header *chm, struct mspack_file *fh, unsigned int n)
{
  struct mspack_system *sys = self->system;
  const size_t bytes = chm->chunk_size;
  unsigned char *data;
  int failed = 0;
  if (n >= chm->num_chunks) return NULL;
  if (!chm->chunk_cache) {
    unsigned char **slots = (unsigned char **) sys->alloc(sys, sizeof(unsigned char *) * chm->num_chunks);
    unsigned int i;
    if (!slots) { self->error = MSPACK_ERR_NOMEMORY; return NULL; }
    for (i = 0; i < chm->num_chunks; i++) slots[i] = NULL;
    chm->chunk_cache = slots;
  }
  if (chm->chunk_cache[n]) return chm->chunk_cache[n];
  if (!(data = (unsigned char *) sys->alloc(sys, bytes))) { self->error = MSPACK_ERR_NOMEMORY; return NULL; }
  if (sys->seek(fh, chm->dir_offset + (off_t) n * (off_t) bytes, MSPACK_SYS_SEEK_START)) failed = MSPACK_ERR_SEEK;
  else if (sys->read(fh, data, (int) bytes) != (int) bytes) failed = MSPACK_ERR_READ;
  else if (memcmp(data, "PMG", 3) != 0 || (data[3] != 'L' && data[3] != 'I')) failed = MSPACK_ERR_SEEK;   /* (the reference's code for a bad signature, chmd.c:676-680) */
  if (failed) { self->error = failed; sys->free(data); return NULL; }
  chm->chunk_cache[n] = data;
  return data;
}

struct chunk_view {
  const unsigned char *first;        /* the first entry */
  const unsigned char *limit;        /* end of the entry area = chunk end - free-space length */
  const unsigned char *count_at;     /* the 16-bit entry count; quick-reference word i sits 2 * i bytes below it */
  unsigned int n_entries, n_quick, per_quick;
  int leaf;                          /* PMGL */
};
/* one entry: its name and what follows it; 0 when the entry does not fit the entry area */
static int entry_name(const struct chunk_view *cv, const unsigned char *at, const unsigned char **name, unsigned int *len)
{
  int bad = 0;
  const unsigned int l = (unsigned int) read_encint(&at, cv->limit, &bad);     /* (32 bits of it, as the reference keeps) */
  if (bad || l > (unsigned int)(cv->limit - at)) return 0;
  *name = at; *len = l;
  return 1;
}
static const unsigned char *quick_entry(const struct chunk_view *cv, unsigned int i)
{
  return cv->first + (i ? rd_le16(cv->count_at - 2u * i) : 0u);
}
static const unsigned char *pass_encints(const unsigned char *at, const unsigned char *limit, int count)
{
  while (count-- > 0) while (at < limit && (*at++ & 0x80)) ;
  return at;
}

/* -1 = malformed chunk, 0 = the name is not here, 1 = found: *res points at the entry's data (PMGL: section, offset,
 * length; PMGI: the child chunk number of the last entry not above the name), *res_end = end of the entry area.
 * The quick-reference probes are the reference's (chmd.c:705-800: the middle of a closed interval, rounded down), so
 * that a chunk whose quick-reference words or entries are damaged is judged by the same entries. */
static int search_chunk(struct mschmd_header *chm, const unsigned char *chunk, const char *filename,
                        const unsigned char **res, const unsigned char **res_end)
{
  struct chunk_view cv;
  const int want_len = (int) strlen(filename);
  const unsigned int free_len = rd_le32(chunk + 4);
  const unsigned char *at, *name, *below = NULL;
  unsigned int len, left, lo, hi;

  cv.leaf = chunk[3] == 'L';
  cv.first = chunk + (cv.leaf ? 0x14 : 8);
  cv.count_at = chunk + chm->chunk_size - 2;
  cv.limit = chunk + chm->chunk_size - free_len;
  cv.n_entries = rd_le16(cv.count_at);
  cv.per_quick = 1u + (1u << chm->density);
  if (cv.n_entries == 0 || free_len > chm->chunk_size) return -1;
  *res_end = cv.limit;
  cv.n_quick = (cv.n_entries + cv.per_quick - 1u) / cv.per_quick;
  if ((int)(2u * cv.n_quick) > (int)(cv.count_at - cv.limit)) cv.n_quick = 0;     /* a table that cannot fit: do without */

  /* which group of per_quick entries?  [lo, hi): the quick entries not yet known to sort before (below lo) or after
   * (from hi on) the name */
  at = cv.first; left = cv.n_entries;
  for (lo = 0, hi = cv.n_quick; lo < hi; ) {
    const unsigned int mid = (lo + hi - 1u) >> 1;
    int o;
    at = quick_entry(&cv, mid);
    if (!entry_name(&cv, at, &name, &len)) return -1;
    o = name_order(filename, want_len, name, (int) len);
    if (o == 0) { *res = name + len; return 1; }
    if (o > 0) lo = mid + 1u;
    else if (mid == 0u) return 0;                               /* sorts before the chunk's first entry */
    else hi = mid;
  }
  if (cv.n_quick) {
    /* lo - 1 = the last quick entry that sorts before the name: its group is the only one that can hold it */
    const unsigned int g = lo - 1u;
    at = quick_entry(&cv, g);
    left = cv.n_entries - g * cv.per_quick;
    if (left > cv.per_quick) left = cv.per_quick;
  }
  for (; left > 0; left--) {
    int o;
    if (!entry_name(&cv, at, &name, &len)) return -1;
    o = name_order(filename, want_len, name, (int) len);
    at = name + len;
    if (o == 0) { *res = at; return 1; }
    if (o < 0) break;
    if (!cv.leaf) below = at;                                   /* (an index chunk: descend below the last name not above ours) */
    at = pass_encints(at, cv.limit, cv.leaf ? 3 : 1);
  }
  *res = below;
  return below ? 1 : 0;
}

static int chmd_fast_find(struct mschm_decompressor *base, struct mschmd_header *chm, const char *filename,
                          struct mschmd_file *f_ptr, int f_size)
{
  struct chmd_p *self = (struct chmd_p *) base;
  struct mspack_system *sys;
  struct mspack_file *fh;
  const unsigned char *chunk, *p = NULL, *end = NULL;
  int err = MSPACK_ERR_OK, result = -1, e = 0;
  unsigned int n;
  if (!self || !chm || !f_ptr || f_size != (int) sizeof(struct mschmd_file)) return MSPACK_ERR_ARGS;
  sys = self->system;
  memset(f_ptr, 0, sizeof(*f_ptr));
  if (!(fh = sys->open(sys, chm->filename, MSPACK_SYS_OPEN_READ))) return MSPACK_ERR_OPEN;

  if (chm->index_root < chm->num_chunks) {
    n = chm->index_root;
    for (;;) {
      if (!(chunk = chunk_get(self, chm, fh, n))) { sys->close(fh); return self->error; }
      if ((result = search_chunk(chm, chunk, filename, &p, &end)) <= 0) break;
      if (chunk[3] == 'L') break;
      n = (unsigned int) read_encint(&p, end, &e);
      if (e) { sys->close(fh); return self->error = MSPACK_ERR_DATAFORMAT; }
    }
  }
  else {
    for (n = chm->first_pmgl; n <= chm->last_pmgl; n = rd_le32(chunk + 0x10)) {
      if (!(chunk = chunk_get(self, chm, fh, n))) { err = self->error; break; }
      if ((result = search_chunk(chm, chunk, filename, &p, &end)) > 0) break;
      if (n == rd_le32(chunk + 0x10)) break;              /* a chunk that names itself as its successor */
    }
  }
  if (result > 0) {
    unsigned int sec = (unsigned int) read_encint(&p, end, &e);
    f_ptr->section = sec == 0 ? (struct mschmd_section *) &chm->sec0 : (struct mschmd_section *) &chm->sec1;
    f_ptr->offset = read_encint(&p, end, &e);
    f_ptr->length = read_encint(&p, end, &e);
    if (e) { sys->close(fh); return self->error = MSPACK_ERR_DATAFORMAT; }
  }
  else if (result < 0) err = MSPACK_ERR_DATAFORMAT;
  sys->close(fh);
  return self->error = err;
}

static int find_sys_file(struct chmd_p *self, struct mschmd_sec_mscompressed *sec, struct mschmd_file **f_ptr, const char *name)
{
  struct mspack_system *sys = self->system;
  struct mschmd_file result;
  if (*f_ptr) return MSPACK_ERR_OK;
  if (chmd_fast_find(&self->base, sec->base.chm, name, &result, (int) sizeof(result)) || !result.section)
    return MSPACK_ERR_DATAFORMAT;
  if (!(*f_ptr = (struct mschmd_file *) sys->alloc(sys, sizeof(result)))) return MSPACK_ERR_NOMEMORY;
  **f_ptr = result;
  (*f_ptr)->filename = (char *) name;
  (*f_ptr)->next = sec->base.chm->sysfiles;
  sec->base.chm->sysfiles = *f_ptr;
  return MSPACK_ERR_OK;
}

static unsigned char *read_sec0_file(struct chmd_p *self, struct mspack_file *fh, struct mschmd_file *file, int *err)
{
  struct mspack_system *sys = self->system;
  unsigned char *data;
  int len;
  if (!file || !file->section || file->section->id != 0) { *err = MSPACK_ERR_DATAFORMAT; return NULL; }
  len = (int) file->length;
  if (!(data = (unsigned char *) sys->alloc(sys, (size_t) len + 1))) { *err = MSPACK_ERR_NOMEMORY; return NULL; }
  if (sys->seek(fh, file->section->chm->sec0.offset + file->offset, MSPACK_SYS_SEEK_START)) { *err = MSPACK_ERR_SEEK; sys->free(data); return NULL; }
  if (sys->read(fh, data, len) != len) { *err = MSPACK_ERR_READ; sys->free(data); return NULL; }
  return data;
}

/* ---- section 1 (reference chmd.c:989-1041, 1072-1315) ---------------------------------------------------
 *
 * What the reference does: extract() keeps ONE lzxd instance alive.  It is (re)created when there is none
 * or the request lies behind its position: at the reset point of the file's interval if the reset table
 * has an entry for it (stream length = UncompLen padded to the interval), else at offset 0 with SpanInfo's
 * length.  A request is lzxd_decompress(skip) + lzxd_decompress(length); every decompress call decodes
 * whole frames up to and INCLUDING the frame that holds the first byte after the request (lzxd.c:419), and
 * any error kills the instance.
 *
 * What we do: every reset interval with a table entry is an independent unit ("fast" results: decoded in
 * GPU batches of CHM_CHUNK_BYTES, buffers kept LRU within the cache budget, per-interval results kept
 * for good).  A virtual decoder (struct vdec) replays the reference's instance on top of those results.
 * An interval's stand-alone result IS the live decoder's result when the decoder was created AT it.  For
 * an interval the live decoder crosses INTO, that only holds if the stand-alone decode is clean (an
 * error there may be a match that reaches before the interval: legal for a decoder that has that
 * history, lzxd.c:622-634), the table entry is where the previous interval's bits really end
 * (result.in_next) and no block spans the reset (MSPACK_HIP_F_BLOCK_OPEN, lzxd.c:424-431).  Otherwise --
 * damaged or odd files only -- the virtual decoder goes SERIAL: one unit from its creation point on, which
 * is the reference's own control flow, exact by construction.  E8: the translation origin is the creation
 * point (lzxd.c:712); fast results use origin 0, so intervals that applied E8 are decoded again with the
 * shifted origin when the decoder was created elsewhere. */
#ifndef CHM_CHUNK_BYTES                    /* (tests/csrc/chm_digest_check.c is built with small chunks, to have several of them) */
#define CHM_CHUNK_BYTES ((off_t) 64 << 20)
#endif
#define CHM_SERIAL_SLACK 16                 /* serial spans are decoded this many intervals past the need */

static int hip_batch(mspack_hip_unit *units, size_t n, const void *in, size_t in_bytes, void *out, size_t out_bytes,
                     mspack_hip_result *res)
{
  int dv = mspack_hip_default_devices();
  return dv > 1 ? mspack_hip_decode_batch_multi(units, n, in, in_bytes, out, out_bytes, res, dv)
                : mspack_hip_decode_batch(units, n, in, in_bytes, out, out_bytes, res);
}

/* the digests a chunk's batch took (units[0 .. n): heads and tails, out_off counted from out_base, where the batch's output holds
 * the chunk's first byte -- stream offset `lo`; res: their results) join the chunk's table.  Without memory for it they are
 * dropped: those files are hashed on the host */
static void chunk_keep_digests(struct mspack_system *sys, struct chm_chunk *ch, off_t lo, const mspack_hip_unit *units,
                               const mspack_hip_result *res, size_t n, int algs, uint64_t out_base)
{
  struct digest_kept *t = (struct digest_kept *) sys->alloc(sys, (ch->dg.n + n) * sizeof(*t));
  if (!t) return;
  if (ch->dg.n) memcpy(t, ch->dg.e, ch->dg.n * sizeof(*t));
  sys->free(ch->dg.e); ch->dg.e = t;
  digest_table_harvest(&ch->dg, units, res, n, out_base, (uint64_t) lo);
  ch->dg_algs |= algs;
}

/* the algorithms a batch that decodes chunk dg_ch (from stream offset lo on) carries digest units for: asked for, not taken yet */
static int chunk_digest_algs(const struct chmd_p *self, const struct chm_p *c, off_t lo, const struct chm_chunk *dg_ch)
{
  return dg_ch && c->n_dfiles && c->padded_len > lo ? digest_device_algs(CHM_ASKED_ALGS(self) & ~dg_ch->dg_algs) : 0;
}
/* ... and those units (chm_digest_plan) for intervals [first, first+count), their ranges counted from out_base of the batch's output;
 * units == NULL: counts only */
static size_t chunk_digest_units(const struct chm_p *c, unsigned int first, unsigned int count, int algs, const double *ratio,
                                 uint64_t out_base, mspack_hip_unit *units, size_t cap)
{
  const off_t lo = (off_t) first * c->interval_bytes;
  const size_t n = chm_digest_plan(c->dfiles, c->n_dfiles, (uint64_t) lo, (uint64_t)(lo + (off_t) count * c->interval_bytes),
                                   (uint64_t) c->padded_len, algs, ratio, units, cap);
  size_t j;
  if (units && out_base) for (j = 0; j < n && j < cap; j++) if (units[j].kind != MSPACK_HIP_KIND_DIGEST_MORE) units[j].out_off += out_base;
  return n;
}

/* the units of intervals [first, first+count) of c, stand-alone; interval i's E8 origin is i*interval - e8_origin.  The CHM's arena
 * (the stream, its slack, its frame tables) lies at in_base of the batch's input arena -- a multiple of 16; 0: it IS the arena --,
 * the intervals' output one behind the other from out_base of the batch's output on */
static void interval_units(const struct chm_p *c, unsigned int first, unsigned int count, off_t e8_origin,
                           uint64_t in_base, uint64_t out_base, mspack_hip_unit *units)
{
  unsigned int k;
  memset(units, 0, (size_t) count * sizeof(*units));
  for (k = 0; k < count; k++) {
    uint64_t off = c->ioff[first + k];
    if (off > (uint64_t) c->arena_len) off = c->arena_len;        /* an entry beyond the file: nothing to read */
    units[k].in_off = in_base + off;
    /* (what is left of THIS CHM's bytes, wherever its arena lies: a stream cut short ends in the reference's two zero bytes and
     *  MSPACK_ERR_READ, readbits.h:192-214, not in what the batch holds behind it) */
    units[k].in_len = (uint32_t)((uint64_t) c->arena_len - off > 0xFFFFFFF0u ? 0xFFFFFFF0u : (uint64_t) c->arena_len - off);
    units[k].out_off = out_base + (uint64_t) k * (uint64_t) c->interval_bytes;
    units[k].out_len = (uint32_t) c->interval_bytes;
    {
      /* the stream ends where the (padded) UncompLen says: an interval that holds the end is as long as what is left of it --
       * for an interval size that is no power of two the reference's padding (& -interval, chmd.c:1153-1157) is no multiple of
       * it.  (Intervals wholly behind the stated end are only ever decoded by a decoder created AT it: unknown length, §vdec) */
      const off_t at = (off_t)(first + k) * c->interval_bytes;
      if (at < c->padded_len && c->padded_len - at < c->interval_bytes) units[k].out_len = (uint32_t)(c->padded_len - at);
    }
    units[k].kind = MSPACK_HIP_KIND_LZX;
    units[k].window_bits = (uint8_t) c->window_bits;
    units[k].reset_frames = (uint16_t) c->fper;
    units[k].e8_base = (int32_t)((off_t)(first + k) * c->interval_bytes - e8_origin);
    if (c->ftab_off) {
      units[k].flags |= MSPACK_HIP_UF_FRAME_TABLE;
      units[k].in_chunk = (uint32_t)((in_base + c->ftab_off + (uint64_t)(first + k) * c->fper * 4) / 4);
    }
  }
}

/* what every failed batch call says and answers */
static int batch_failed(struct mspack_system *sys)
{
  sys->message(NULL, "GPU batch decode failed: %s", mspack_hip_last_error());
  return MSPACK_ERR_DECRUNCH;
}

/* intervals [first, first+count) decoded again, stand-alone (interval_units) and synchronously, with another E8 origin: no chunk,
 * no digest units, the caller's buffers (vdec_emit) */
static int decode_intervals(struct chmd_p *self, struct chm_p *c, unsigned int first, unsigned int count,
                            off_t e8_origin, unsigned char *out, mspack_hip_result *res)
{
  struct mspack_system *sys = self->system;
  mspack_hip_unit *units = (mspack_hip_unit *) sys->alloc(sys, (size_t) count * sizeof(*units));
  int rc;
  if (!units) return MSPACK_ERR_NOMEMORY;
  interval_units(c, first, count, e8_origin, 0, 0, units);
  count_batch(count);
  rc = hip_batch(units, count, c->arena, c->arena_room, out, (size_t) count * (size_t) c->interval_bytes + 64, res);
  sys->free(units);
  return rc ? batch_failed(sys) : MSPACK_ERR_OK;
}

/* ---- the batch: what decodes chunks, one (extract()) or those of many CHMs (mspack_chmd_prefetch) ----
 * The batch owns the units and what it writes: the results, and ONE output buffer that its chunks share.  A member chunk's buf
 * points into that buffer (no copy per chunk); the buffer goes when its last user has gone (users), whatever happens to the other
 * CHMs.  While the batch runs as a job, `left` members have not taken all of their units yet; the last one out ends the job, and
 * units, results and the input arena go then.  The decompressor keeps the list (chmd_p.batches) so that destroying it can settle them.
 * The input is either the batch's own (in: a copy of every CHM's arena, so that nothing points into a CHM and close() of one never
 * waits) or BORROWED (in == NULL: the units address the arena of the one CHM at in_base 0 -- no copy of an arena that can be large).
 * The invariant of a borrowed input: every member is a chunk of that one CHM, and the job has ended before that CHM's arena is freed.
 * free_sec1 keeps it by dropping the CHM's chunks (chunk_drop_buf -> chunk_detach: the last one out ends the job) BEFORE it frees the
 * arena; destroying the decompressor ends every job while the CHMs, which only close() frees, still stand. */
struct chm_member {
  struct chm_chunk *ch;               /* NULL: the chunk has left (evicted, its CHM closed) */
  mspack_hip_result *ires;            /* where the results of its intervals go: its CHM's ires[] from the chunk's first interval on */
  size_t u0; unsigned int count;      /* its intervals are units [u0, u0 + count) */
};
struct chm_batch {
  struct chm_batch *next; struct chmd_p *owner;
  struct chm_member *m; size_t n, users, left;
  mspack_hip_unit *units; mspack_hip_result *res; unsigned char *in, *out; int in_pinned;
  mspack_hip_job *job;
};

/* the job, if there is one, to its end, and everything only the running batch needs given back (0, or the batch's failure) */
static int batch_end_job(struct mspack_system *sys, struct chm_batch *B)
{
  int rc = 0;
  if (B->job) { rc = mspack_hip_job_end(B->job); B->job = NULL; }
  if (B->in_pinned) { mspack_hip_unpin(B->in); B->in_pinned = 0; }
  sys->free(B->units); sys->free(B->res); mspack_arena_free(sys, B->in);
  B->units = NULL; B->res = NULL; B->in = NULL;
  return rc;
}
static void batch_free(struct mspack_system *sys, struct chm_batch *B)
{
  struct chm_batch **at;
  (void) batch_end_job(sys, B);
  for (at = &B->owner->batches; *at; at = &(*at)->next) if (*at == B) { *at = B->next; break; }
  mspack_arena_free(sys, B->out); sys->free(B->m); sys->free(B);
}
/* a chunk stops waiting for the running batch (its units are through, or nobody will ask: eviction, close); the batch goes on for
 * the others.  Returns the job's answer when this was the last one it ran for, else 0 */
static int chunk_detach(struct mspack_system *sys, struct chm_chunk *ch)
{
  struct chm_batch *B = ch->bat;
  ch->bat_run = 0;
  return --B->left == 0 ? batch_end_job(sys, B) : 0;
}
/* the chunk's decoded bytes go: it stops waiting for its batch and gives its share of the output buffer back -- the last one out
 * frees the batch */
static void chunk_drop_buf(struct mspack_system *sys, struct chm_chunk *ch)
{
  struct chm_batch *B = ch->bat;
  if (!B) return;
  if (ch->bat_run) (void) chunk_detach(sys, ch);
  B->m[ch->bat_k].ch = NULL; ch->bat = NULL; ch->buf = NULL;
  if (--B->users == 0) batch_free(sys, B);
}

/* unit i of the chunk in its running batch: its result goes to the CHM's ires[] */
static int chunk_wait_unit(struct chm_chunk *ch, unsigned int i)
{
  struct chm_batch *B = ch->bat;
  const struct chm_member *m = &B->m[ch->bat_k];
  const int rc = mspack_hip_job_wait_unit(B->job, m->u0 + i);
  if (!rc) m->ires[i] = B->res[m->u0 + i];
  return rc;
}

/* the chunk's units, if its batch is still running, to their end: buf and ires[] are the driver's again (0, or the batch's failure) */
static int chunk_settle(struct mspack_system *sys, struct chm_chunk *ch)
{
  int rc = 0, rc2;
  if (!ch->bat_run) return 0;
  while (!rc && ch->job_waited < ch->bat->m[ch->bat_k].count) if (!(rc = chunk_wait_unit(ch, ch->job_waited))) ch->job_waited++;
  rc2 = chunk_detach(sys, ch);
  return rc ? rc : rc2;
}

/* ONE batch that decodes the chunks pk[0 .. n) -- the caller fills c, ch, first, count (chunk_span) and in_base -- and makes them
 * its members.  in_total > 0: the batch reads a copy of its own of the CHMs' arenas, in_total bytes, every CHM's piece at in_base (a
 * multiple of 16; the picks of one CHM lie together); in_total == 0: it borrows the arena of the one CHM all picks are of (in_base
 * 0; struct chm_batch).  It runs as a job when it may and can -- several units, one device, no digest units: those are through only
 * when the whole batch is -- and the call returns at once then, every later call waiting for the units of its chunk only
 * (chunk_wait); otherwise it has run to its end here, the results are in ires[] and the digests it took are kept.  A batch that
 * fails says so once and leaves nothing behind: no chunk is touched */
struct chm_pick { struct chm_p *c; struct chm_chunk *ch; unsigned int first, count; uint64_t in_base, out_base; int dg_algs; size_t dg_n; };

static int issue_batch(struct chmd_p *self, struct chm_pick *pk, size_t n, uint64_t in_total, int may_job)
{
  struct mspack_system *sys = self->system;
  struct chm_batch *B = (struct chm_batch *) sys->alloc(sys, sizeof(*B));
  const void *in = pk[0].c->arena;
  size_t in_bytes = pk[0].c->arena_room, n_units = 0, n_dg = 0, out_total = 0, k, u = 0, d;
  double ratio[DIGEST_ALGS] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
  int as_job;
  if (!B) return MSPACK_ERR_NOMEMORY;
  memset(B, 0, sizeof(*B));
  B->owner = self; B->n = n;
  if (CHM_ASKED_ALGS(self)) digest_ratios(ratio);
  for (k = 0; k < n; k++) {
    pk[k].out_base = out_total;
    pk[k].dg_algs = chunk_digest_algs(self, pk[k].c, (off_t) pk[k].first * pk[k].c->interval_bytes, pk[k].ch);
    pk[k].dg_n = pk[k].dg_algs ? chunk_digest_units(pk[k].c, pk[k].first, pk[k].count, pk[k].dg_algs, ratio, 0, NULL, 0) : 0;
    out_total += ((size_t) pk[k].count * (size_t) pk[k].c->interval_bytes + 63) & ~(size_t) 63;
    n_units += pk[k].count; n_dg += pk[k].dg_n;
  }
  B->m = (struct chm_member *) sys->alloc(sys, n * sizeof(*B->m));
  B->units = (mspack_hip_unit *) sys->alloc(sys, (n_units + n_dg) * sizeof(*B->units));
  B->res = (mspack_hip_result *) sys->alloc(sys, (n_units + n_dg) * sizeof(*B->res));
  if (in_total) B->in = (unsigned char *) mspack_arena_alloc(sys, (size_t) in_total + 64);
  B->out = (unsigned char *) mspack_arena_alloc(sys, out_total + 128);
  if (!B->m || !B->units || !B->res || (in_total && !B->in) || !B->out) { batch_free(sys, B); return MSPACK_ERR_NOMEMORY; }
  for (k = 0, d = n_units; k < n; k++) {
    const struct chm_p *c = pk[k].c;
    if (in_total && (!k || c != pk[k - 1].c)) {
      /* every CHM's piece of the input arena: its stream, the zero bytes behind it, its frame tables -- on a 16-byte boundary, so
       * that the tables stay uint32-aligned and in_chunk names them (interval_units); 64 zero bytes of slack behind the last one */
      const size_t piece = (c->arena_room + 15) & ~(size_t) 15;
      memcpy(B->in + pk[k].in_base, c->arena, c->arena_room);
      memset(B->in + pk[k].in_base + c->arena_room, 0, piece - c->arena_room);
    }
    B->m[k].ch = NULL; B->m[k].ires = &pk[k].c->ires[pk[k].first]; B->m[k].u0 = u; B->m[k].count = pk[k].count;
    interval_units(c, pk[k].first, pk[k].count, 0, pk[k].in_base, pk[k].out_base, B->units + u);
    u += pk[k].count;
    if (pk[k].dg_n) { (void) chunk_digest_units(c, pk[k].first, pk[k].count, pk[k].dg_algs, ratio, pk[k].out_base, B->units + d, pk[k].dg_n); d += pk[k].dg_n; }
  }
  memset(B->res, 0, (n_units + n_dg) * sizeof(*B->res));
  if (in_total) {
    memset(B->in + in_total, 0, 64);
    /* the arena was written a moment ago: page-locked, its copy to the device is plain DMA (advice only) */
    B->in_pinned = in_total >= ((uint64_t) 4 << 20) && !mspack_arena_is_locked(B->in) && mspack_hip_pin(B->in, mspack_arena_room((size_t) in_total + 64)) == 0;
    in = B->in; in_bytes = (size_t) in_total;
  }
  count_batch(n_units);
  as_job = may_job && n_units >= 2 && !n_dg && mspack_hip_default_devices() <= 1 &&
           (B->job = mspack_hip_decode_batch_begin(B->units, n_units, in, in_bytes, B->out, out_total + 64, B->res)) != NULL;
  if (!as_job && hip_batch(B->units, n_units + n_dg, in, in_bytes, B->out, out_total + 64, B->res)) {
    const int err = batch_failed(sys);
    batch_free(sys, B);
    return err;
  }
  for (k = 0, d = n_units; k < n; k++) {
    struct chm_chunk *ch = pk[k].ch;
    B->m[k].ch = ch;
    ch->bat = B; ch->bat_k = k; ch->bat_run = as_job; ch->buf = B->out + pk[k].out_base; ch->res_valid = 1; ch->job_waited = 0;
    if (!as_job) {
      memcpy(B->m[k].ires, B->res + B->m[k].u0, (size_t) pk[k].count * sizeof(*B->res));
      if (pk[k].dg_n) {
        chunk_keep_digests(sys, ch, (off_t) pk[k].first * pk[k].c->interval_bytes, B->units + d, B->res + d, pk[k].dg_n, pk[k].dg_algs, pk[k].out_base);
        d += pk[k].dg_n;
      }
    }
  }
  B->users = n; B->left = as_job ? n : 0;
  B->next = self->batches; self->batches = B;
  if (!as_job) (void) batch_end_job(sys, B);               /* (units, results and the input arena have served) */
  return MSPACK_ERR_OK;
}

static void free_sec1(struct mspack_system *sys, struct chm_p *c) {
  unsigned int i;
  /* the chunks first, the arena behind them: a chunk is taken out of a running batch unwaited (chunk_drop_buf: the batch goes on
   * for the others), and a batch that borrows this CHM's arena has ended its job when its last chunk has left (struct chm_batch) */
  if (c->chunks) for (i = 0; i < c->n_chunks; i++) { chunk_drop_buf(sys, &c->chunks[i]); sys->free(c->chunks[i].dg.e); }
  if (c->arena_pinned) { mspack_hip_unpin(c->arena); c->arena_pinned = 0; }
  sys->free(c->chunks); mspack_arena_free(sys, c->arena); sys->free(c->ioff); sys->free(c->ires); mspack_arena_free(sys, c->s_buf);
  sys->free(c->dfiles); c->dfiles = NULL; c->n_dfiles = 0;
  c->chunks = NULL; c->arena = NULL; c->ioff = NULL; c->ires = NULL; c->s_buf = NULL; c->sec1_state = 0;
  c->n_chunks = 0; c->s_valid = 0;
}

static int dfile_order(const void *pa, const void *pb)
{
  const struct chm_digest_file *a = (const struct chm_digest_file *) pa, *b = (const struct chm_digest_file *) pb;
  if (a->offset != b->offset) return a->offset < b->offset ? -1 : 1;
  return a->length < b->length ? -1 : a->length > b->length;
}

/* c->dfiles: one walk of chm->files, once per CHM (advice for the chunks' batches: without memory for it no file gets a unit) */
static void collect_dfiles(struct mspack_system *sys, struct chm_p *c)
{
  const struct mschmd_file *fi;
  size_t n = 0;
  for (fi = c->base.files; fi; fi = fi->next) if (fi->section && fi->section->id == 1 && fi->offset >= 0 && fi->length > 0) n++;
  if (!n || !(c->dfiles = (struct chm_digest_file *) sys->alloc(sys, n * sizeof(*c->dfiles)))) return;
  for (fi = c->base.files; fi; fi = fi->next)
    if (fi->section && fi->section->id == 1 && fi->offset >= 0 && fi->length > 0) {
      c->dfiles[c->n_dfiles].offset = (uint64_t) fi->offset; c->dfiles[c->n_dfiles].length = (uint64_t) fi->length;
      c->n_dfiles++;
    }
  qsort(c->dfiles, c->n_dfiles, sizeof(*c->dfiles), dfile_order);
}

/* ControlData, the compressed stream, ResetTable and SpanInfo: everything chmd_init_decomp (chmd.c:1072-1188)
 * reads, parsed once.  Returns the error the reference's init would return for EVERY file. */
static int setup_sec1(struct chmd_p *self, struct chm_p *c, struct mspack_file *fh)
{
  struct mspack_system *sys = self->system;
  struct mschmd_sec_mscompressed *sec = &c->base.sec1;
  unsigned char *data;
  int err = MSPACK_ERR_OK;
  unsigned int version, wsize;
  off_t reset_interval;
  size_t arena_alloc = 0;            /* bytes behind c->arena */

  if ((err = find_sys_file(self, sec, &sec->content, content_name))) return err;
  if ((err = find_sys_file(self, sec, &sec->control, control_name))) return err;
  if (sec->control->length != 0x1C) return MSPACK_ERR_DATAFORMAT;
  if (!(data = read_sec0_file(self, fh, sec->control, &err))) return err;
  if (rd_le32(data + 4) != 0x43585A4Cu) { sys->free(data); return MSPACK_ERR_SIGNATURE; }
  version = rd_le32(data + 8);
  reset_interval = (off_t) rd_le32(data + 0x0C);
  wsize = rd_le32(data + 0x10);
  sys->free(data);
  if (version == 2) { reset_interval *= FRAME; wsize *= FRAME; }
  else if (version != 1) return MSPACK_ERR_DATAFORMAT;
  switch (wsize) {
  case 0x008000: c->window_bits = 15; break; case 0x010000: c->window_bits = 16; break;
  case 0x020000: c->window_bits = 17; break; case 0x040000: c->window_bits = 18; break;
  case 0x080000: c->window_bits = 19; break; case 0x100000: c->window_bits = 20; break;
  case 0x200000: c->window_bits = 21; break;
  default: return MSPACK_ERR_DATAFORMAT;
  }
  /* the reference computes in `int` (chmd.c:1075,1114-1121): an interval beyond 2^31 wraps there */
  reset_interval = (off_t)(int)(unsigned int) reset_interval;
  if (reset_interval == 0 || reset_interval % FRAME) return MSPACK_ERR_DATAFORMAT;
  /* (an interval that wrapped negative passes the reference's checks and ends in lzxd_init(reset_interval < 0) == NULL:
   *  MSPACK_ERR_NOMEMORY, lzxd.c:297-300, chmd.c:1183-1187) */
  if (reset_interval < 0) return MSPACK_ERR_NOMEMORY;
  if (reset_interval / FRAME > 65535) return MSPACK_ERR_DATAFORMAT;                          /* ours: unit field width */
  c->interval_bytes = reset_interval;
  c->fper = (unsigned int)(reset_interval / FRAME);

  /* the compressed stream: from the start of Content to the end of the FILE -- the reference's decoder
   * reads on from wherever it is (sys->read on the CHM itself), not just inside Content */
  {
    off_t start = c->base.sec0.offset + sec->content->offset, flen = 0, avail;
    size_t want;
    if (sec->content->section->id != 0) return MSPACK_ERR_DATAFORMAT;
    if (mspack_sys_filelen(sys, fh, &flen)) return MSPACK_ERR_SEEK;
    avail = (start >= 0 && flen > start) ? flen - start : 0;
    want = (size_t) avail;
    /* (room behind the stream: 128 zero bytes, then one uint32 per frame the reset table can describe) */
    {
      /* the frame table below holds n_fast * fper entries, n_fast <= table bytes / (fper * entry size) + 1 intervals:
       * at most one uint32 per 4 table bytes plus one interval's worth (fper comes from ControlData: up to 65535) */
      size_t extra = 0;
      if (!find_sys_file(self, sec, &sec->rtable, rtable_name) && sec->rtable->length >= 0x28 && sec->rtable->length <= 1000000)
        extra = (size_t) sec->rtable->length + (size_t) c->fper * 4u;
      arena_alloc = want + 128 + extra + 16;
      if (!(c->arena = (unsigned char *) mspack_arena_alloc(sys, arena_alloc))) return MSPACK_ERR_NOMEMORY;
      memset(c->arena + want, 0, arena_alloc - want);         /* (the stream itself is read over the rest) */
      c->arena_room = want + 64;
    }
    c->ftab_off = 0;
    if (want) {
      if (sys->seek(fh, start, MSPACK_SYS_SEEK_START)) return MSPACK_ERR_SEEK;
      if (sys->read(fh, c->arena, (int) want) != (int) want) return MSPACK_ERR_READ;
    }
    c->arena_len = want;
    c->content_start = start;
  }

  /* reset table (read_reset_table, chmd.c:1195-1267): which intervals have a usable entry */
  c->n_fast = 0; c->n_intervals = 0; c->padded_len = 0;
  if (!find_sys_file(self, sec, &sec->rtable, rtable_name) && sec->rtable->length >= 0x28 &&
      sec->rtable->length <= 1000000 && (data = read_sec0_file(self, fh, sec->rtable, &err))) {
    unsigned int nent = rd_le32(data + 4), esz = rd_le32(data + 8), toff = rd_le32(data + 0x0C);
    if (rd_le32(data + 0x20) == FRAME && (esz == 4 || esz == 8)) {
      off_t total = (off_t) rd_le64(data + 0x10);
      uint64_t ni, nt;
      c->padded_len = (total + reset_interval - 1) & -reset_interval;      /* chmd.c:1153-1157 */
      /* (intervals that hold bytes of the padded length: for an interval that is no power of two the reference's rounding
       *  above does not give a multiple of it) */
      ni = c->padded_len > 0 ? (uint64_t)((c->padded_len + reset_interval - 1) / reset_interval) : 0;
      if (ni > 0x7FFFFFFFu / c->fper) ni = 0x7FFFFFFFu / c->fper;
      /* entries exist for the intervals whose first frame index is below NumEntries and inside the table's file -- whatever
       * UncompLen says: the reference looks an entry up BEFORE it looks at the length (chmd.c:1146-1157), so a file that lies
       * behind a dishonest UncompLen is answered from ITS interval (and then refused: lzxd_init with a negative length ->
       * MSPACK_ERR_NOMEMORY, or "offset beyond the length" -> MSPACK_ERR_DECRUNCH), not from SpanInfo */
      nt = (uint64_t) nent / c->fper + 1u;
      { const uint64_t by_file = (uint64_t) sec->rtable->length / esz / c->fper + 1u; if (nt > by_file) nt = by_file; }
      if (nt > 0x7FFFFFFFu / c->fper) nt = 0x7FFFFFFFu / c->fper;
      if (nt && (c->ioff = (uint64_t *) sys->alloc(sys, (size_t) nt * sizeof(uint64_t)))) {
        unsigned int k;
        for (k = 0; k < nt; k++) {
          unsigned int entry = k * c->fper;
          unsigned int pos = toff + entry * esz;                              /* unsigned wrap as in chmd.c:1237 */
          if (entry >= nent || (off_t) pos > sec->rtable->length - (off_t) esz) break;
          c->ioff[k] = (esz == 4) ? rd_le32(data + pos) : (uint64_t) rd_le64(data + pos);
        }
        c->n_fast = k;
        c->n_intervals = (unsigned int) ni;
        /* the frames' offsets inside every interval, for the frame-parallel parse: a hint, never trusted */
        if (c->fper >= 2 && c->n_fast &&
            ((c->arena_len + 128 + 3) & ~(size_t) 3) + (size_t) c->n_fast * c->fper * 4u <= arena_alloc) {   /* (never without room) */
          const size_t base = (c->arena_len + 128 + 3) & ~(size_t) 3;
          uint32_t *tab = (uint32_t *)(c->arena + base);
          unsigned int j;
          int ok = 1;
          for (k = 0; k < c->n_fast && ok; k++)
            for (j = 0; j < c->fper; j++) {
              unsigned int entry = k * c->fper + j;
              unsigned int pos = toff + entry * esz;
              uint64_t v;
              if (entry >= nent || (off_t) pos > sec->rtable->length - (off_t) esz) { tab[entry] = 0xFFFFFFFFu; continue; }
              v = (esz == 4) ? rd_le32(data + pos) : (uint64_t) rd_le64(data + pos);
              tab[entry] = (v >= c->ioff[k] && v - c->ioff[k] < 0xFFFFFFF0u) ? (uint32_t)(v - c->ioff[k]) : 0xFFFFFFFFu;
            }
          c->ftab_off = base;
          c->arena_room = base + (size_t) c->n_fast * c->fper * 4;
        }
      }
    }
    sys->free(data);
  }
  /* SpanInfo (read_spaninfo, chmd.c:1275-1315): the fallback's stream length, or the error it ends in */
  c->span_err = MSPACK_ERR_OK; c->span_len = 0;
  if (find_sys_file(self, sec, &sec->spaninfo, spaninfo_name)) c->span_err = MSPACK_ERR_DATAFORMAT;
  else if (sec->spaninfo->length != 8) c->span_err = MSPACK_ERR_DATAFORMAT;
  else if (!(data = read_sec0_file(self, fh, sec->spaninfo, &err))) c->span_err = err;
  else {
    c->span_len = (off_t) rd_le64(data);
    sys->free(data);
    if (c->span_len <= 0) c->span_err = MSPACK_ERR_DATAFORMAT;
    else if (c->span_len > 0xFFFF0000LL) c->span_err = MSPACK_ERR_DATAFORMAT;   /* ours: a unit's out_len is 32 bits */
  }

  /* every batch of this CHM reads the arena: page-locked once, its copies to the device are plain DMA (advice only) */
  if (!c->arena_pinned && arena_alloc >= ((size_t) 4 << 20) && !mspack_arena_is_locked(c->arena)) c->arena_pinned = mspack_hip_pin(c->arena, mspack_arena_room(arena_alloc)) == 0;

  /* fast-result bookkeeping */
  if (c->n_fast) {
    c->chunk_int = (unsigned int)(CHM_CHUNK_BYTES / c->interval_bytes); if (!c->chunk_int) c->chunk_int = 1;
    c->n_chunks = (c->n_fast + c->chunk_int - 1) / c->chunk_int;
    if (!(c->chunks = (struct chm_chunk *) sys->alloc(sys, (size_t) c->n_chunks * sizeof(*c->chunks)))) return MSPACK_ERR_NOMEMORY;
    memset(c->chunks, 0, (size_t) c->n_chunks * sizeof(*c->chunks));      /* (nothing decoded, no batch, no digests) */
    if (!(c->ires = (mspack_hip_result *) sys->alloc(sys, (size_t) c->n_fast * sizeof(mspack_hip_result)))) return MSPACK_ERR_NOMEMORY;
    collect_dfiles(sys, c);
  }
  return MSPACK_ERR_OK;
}

/* a chunk whose batch is still running: wait until intervals up to k_to (of this chunk) have come through */
static int chunk_wait(struct chmd_p *self, struct chm_chunk *ch, unsigned int first, unsigned int k_to)
{
  struct mspack_system *sys = self->system;
  unsigned int count, upto = k_to - first + 1;
  int rc = 0;
  if (!ch->bat_run) return MSPACK_ERR_OK;
  count = ch->bat->m[ch->bat_k].count;
  if (upto > count) upto = count;
  while (!rc && ch->job_waited < upto) if (!(rc = chunk_wait_unit(ch, ch->job_waited))) ch->job_waited++;
  /* a unit failed, or all of the chunk's are through: it leaves the running batch (the last one out hears the job's answer) */
  if ((rc || ch->job_waited >= count) && chunk_detach(sys, ch)) rc = 1;
  if (!rc) return MSPACK_ERR_OK;
  /* the batch failed: what issue_batch says of a failed call, and nothing of the chunk is kept */
  rc = batch_failed(sys);
  chunk_drop_buf(sys, ch); ch->res_valid = 0;
  return rc;
}

/* chunk ci of c: its intervals [first, first + count) */
static void chunk_span(const struct chm_p *c, unsigned int ci, unsigned int *first, unsigned int *count)
{
  *first = ci * c->chunk_int;
  *count = (*first + c->chunk_int <= c->n_fast) ? c->chunk_int : c->n_fast - *first;
}

/* fast results (and, if `need_buf`, the decoded bytes) of the chunk that holds interval k -- of its intervals up to k_to */
static int ensure_chunk_to(struct chmd_p *self, struct chm_p *c, unsigned int k, unsigned int k_to, int need_buf, struct chm_chunk **out)
{
  struct mspack_system *sys = self->system;
  unsigned int ci = k / c->chunk_int, first, count, i;
  struct chm_chunk *ch = &c->chunks[ci];
  int err;
  chunk_span(c, ci, &first, &count);
  if (out) *out = ch;
  ch->stamp = ++c->stamp;
  if (ch->buf || (ch->res_valid && !need_buf)) return chunk_wait(self, ch, first, k_to);
  /* stay inside the cache budget: drop the least recently used buffers */
  {
    size_t budget = (size_t) mspack_hip_cache_mb() << 20, each = (size_t) c->chunk_int * (size_t) c->interval_bytes;
    for (;;) {
      size_t used = 0; struct chm_chunk *lru = NULL;
      for (i = 0; i < c->n_chunks; i++)
        if (c->chunks[i].buf) { used += each; if (&c->chunks[i] != ch && (!lru || c->chunks[i].stamp < lru->stamp)) lru = &c->chunks[i]; }
      if (used + each <= budget || !lru) break;
      if (chunk_settle(sys, lru)) lru->res_valid = 0;      /* (a batch that failed behind what was asked of it: decoded again when needed) */
      chunk_drop_buf(sys, lru);
    }
  }
  /* the chunk's own batch: one member, the CHM's arena borrowed; it runs as a job when it can -- extract() of the first file
   * returns when the file's intervals are through, and the caller writes it while the rest is decoded and copied back.
   * (a chunk whose bytes will not be kept -- beyond the cache budget -- is decoded synchronously: it leaves the batch at once) */
  {
    const int keep = need_buf || count * (size_t) c->interval_bytes <= ((size_t) mspack_hip_cache_mb() << 20);
    struct chm_pick pk;
    memset(&pk, 0, sizeof(pk));
    pk.c = c; pk.ch = ch; pk.first = first; pk.count = count;
    if ((err = issue_batch(self, &pk, 1, 0, keep))) return err;
    if (!keep) chunk_drop_buf(sys, ch);
  }
  return chunk_wait(self, ch, first, k_to);
}
static int ensure_chunk(struct chmd_p *self, struct chm_p *c, unsigned int k, int need_buf, struct chm_chunk **out)
{
  return ensure_chunk_to(self, c, k, k, need_buf, out);
}

static int interval_clean(const mspack_hip_result *r) {
  return r->err == MSPACK_ERR_OK || (r->err == MSPACK_ERR_READ && (r->flags & MSPACK_HIP_F_LOOKAHEAD_READ));
}

/* the serial span of the virtual decoder: ONE unit from its creation point covering at least `need` bytes */
static int ensure_serial(struct chmd_p *self, struct chm_p *c, off_t need)
{
  struct mspack_system *sys = self->system;
  struct vdec *v = &self->v;
  off_t full = v->length - v->init, cover;
  mspack_hip_unit u;
  uint64_t off = v->in_off;
  unsigned int log_cap;
  size_t log_off;
  if (need > full) need = full;
  if (c->s_valid && c->s_init == v->init && c->s_mode == v->mode && c->s_cover >= need) return MSPACK_ERR_OK;
  cover = need + (off_t) CHM_SERIAL_SLACK * c->interval_bytes;
  cover = (cover + FRAME - 1) & ~(off_t)(FRAME - 1);
  if (cover >= full) cover = full;
  if (cover > 0xFFFF0000LL) return MSPACK_ERR_DATAFORMAT;                /* ours: 32-bit unit length */
  mspack_arena_free(sys, c->s_buf); c->s_buf = NULL; c->s_valid = 0;
  /* (one log entry per reset point the span can reach, the look-ahead frame's included) */
  log_cap = (unsigned int)(cover / c->interval_bytes) + 2u;
  log_off = ((size_t) cover + 32768 + 15) & ~(size_t) 15;
  if (!(c->s_buf = (unsigned char *) mspack_arena_alloc(sys, log_off + 4 + 4 * (size_t) log_cap + 128))) return MSPACK_ERR_NOMEMORY;
  memset(&u, 0, sizeof(u));
  if (off > (uint64_t) c->arena_len) off = c->arena_len;
  u.in_off = off;
  u.in_len = (uint32_t)((uint64_t) c->arena_len - off > 0xFFFFFFF0u ? 0xFFFFFFF0u : (uint64_t) c->arena_len - off);
  u.out_off = 0; u.out_len = (uint32_t) cover;
  u.kind = MSPACK_HIP_KIND_LZX; u.window_bits = (uint8_t) c->window_bits; u.reset_frames = (uint16_t) c->fper;
  u.e8_base = 0;
  u.flags = MSPACK_HIP_UF_LZX_LOG; u.ref_len = log_cap;
  count_batch(1);
  if (mspack_hip_decode_batch(&u, 1, c->arena, c->arena_len + 64, c->s_buf, log_off + 4 + 4 * (size_t) log_cap + 64, &c->s_res)) return batch_failed(sys);
  c->s_log = c->s_buf + log_off + 4; c->s_log_cap = log_cap;
  c->s_log_n = rd_le32(c->s_buf + log_off); if (c->s_log_n > log_cap) c->s_log_n = log_cap;
  c->s_valid = 1; c->s_init = v->init; c->s_mode = v->mode; c->s_cover = cover;
  return MSPACK_ERR_OK;
}

static int vdec_decode(struct chmd_p *self, struct chm_p *c, off_t A, off_t B, off_t *good);

/* One lzxd_decompress(B - A) of the virtual decoder standing at A.  Returns the reference's code; *good =
 * first byte position that was not produced (>= B on success). */
static int vdec_phase(struct chmd_p *self, struct chm_p *c, off_t A, off_t B, off_t *good)
{
  struct vdec *v = &self->v;
  off_t fe = B / FRAME;                         /* last frame the call decodes (lzxd.c:419), absolute index */
  int err;
  *good = B;
  (void) A;
  /* bytes of the frame decoded last are stored up: a call they satisfy decodes nothing (lzxd.c:397-408) */
  if (B <= v->decoded_end) return MSPACK_ERR_OK;
  err = vdec_decode(self, c, v->decoded_end, B, good);
  if (!err) { v->decoded_end = (fe + 1) * FRAME; if (v->decoded_end > v->length) v->decoded_end = v->length; }
  return err;
}

/* the frames from position A (a frame start the decoder has not decoded yet) up to and INCLUDING the frame
 * that holds B -- a call that has to decode always goes one frame past an end on a frame boundary (lzxd.c:419) */
static int vdec_decode(struct chmd_p *self, struct chm_p *c, off_t A, off_t B, off_t *good)
{
  struct vdec *v = &self->v;
  off_t fe = B / FRAME;
  int err;
  if (!v->serial) {
    unsigned int k0 = (unsigned int)(v->init / c->interval_bytes), k, k_hi;
    off_t total_frames = v->length / FRAME;     /* table mode: the length is padded to whole intervals */
    off_t kh = fe / c->fper;
    /* (the intervals of THIS decoder's stream: c->n_intervals, but for the decoder of unknown length, struct vdec) */
    const unsigned int nv = (unsigned int)((v->length + c->interval_bytes - 1) / c->interval_bytes);
    k_hi = (kh >= (off_t) nv) ? nv - 1 : (unsigned int) kh;
    for (k = (unsigned int)(A / c->interval_bytes); k <= k_hi && (off_t) k * c->interval_bytes < v->length; k++) {
      if (k >= c->n_fast) { v->serial = 1; break; }
      if ((err = ensure_chunk(self, c, k, 0, NULL))) return err;
      if (k > k0) {
        const mspack_hip_result *p;
        if ((err = ensure_chunk(self, c, k - 1, 0, NULL))) return err;
        p = &c->ires[k - 1];
        if (!interval_clean(&c->ires[k]) || (p->flags & MSPACK_HIP_F_BLOCK_OPEN) ||
            c->ioff[k] != c->ioff[k - 1] + p->in_next) { v->serial = 1; break; }
      }
      else if (!interval_clean(&c->ires[k])) {
        off_t g = (off_t) k * c->interval_bytes + c->ires[k].good_len;
        if (fe >= g / FRAME) { *good = g; return c->ires[k].err; }
      }
    }
    if (!v->serial) {
      if (fe >= total_frames) {
        /* the request reaches the end of the stream: the reference still enters one more (empty) frame,
         * at a reset point, and reads the header bit there -- which fails only if the input is exhausted */
        if (nv && nv <= c->n_fast) {
          if ((err = ensure_chunk(self, c, nv - 1, 0, NULL))) return err;
          if (c->ires[nv - 1].flags & MSPACK_HIP_F_LOOKAHEAD_READ) { *good = v->length; return MSPACK_ERR_READ; }
        }
        if (B > v->length) { *good = v->length; return MSPACK_ERR_DECRUNCH; }         /* lzxd.c:758-761 */
      }
      return MSPACK_ERR_OK;
    }
  }
  /* serial: the decoder's own unit, positions relative to its creation point */
  {
    off_t full = v->length - v->init, need = (fe + 1) * FRAME - v->init, nframes, rfe = fe - v->init / FRAME, g;
    const mspack_hip_result *r = &c->s_res;
    if ((err = ensure_serial(self, c, need))) return err;
    nframes = (c->s_cover + FRAME - 1) / FRAME;
    {
      /* "invalid reset interval": said once per lzxd_decompress call that enters -- decodes or fails in -- a frame whose
       * reset found a block still open (lzxd.c:423-431; the warning comes before anything of that frame is read) */
      const off_t ra = (A - v->init) / FRAME;
      off_t last = rfe;
      unsigned int i;
      if (r->err && !((off_t) r->good_len >= full) && (off_t)(r->good_len / FRAME) < last) last = (off_t)(r->good_len / FRAME);
      for (i = 0; i < c->s_log_n; i++) {
        const off_t f = (off_t) rd_le32(c->s_log + 4 * (size_t) i);
        if (f >= ra && f <= last) {
          self->system->message(NULL, "WARNING; invalid reset interval detected during LZX decompression");
          break;
        }
      }
    }
    if (c->s_cover < full) {
      /* a partial span is good for the frames it holds completely */
      if ((off_t) r->good_len / FRAME > rfe) return MSPACK_ERR_OK;
      g = v->init + r->good_len; *good = g;
      return r->err ? r->err : MSPACK_ERR_DECRUNCH;
    }
    if (r->err == MSPACK_ERR_OK) {
      if (B > v->length) { *good = v->length; return MSPACK_ERR_DECRUNCH; }
      return MSPACK_ERR_OK;
    }
    if ((off_t) r->good_len >= full) {                 /* everything came out; the look-ahead failed */
      if (rfe < nframes) return MSPACK_ERR_OK;
      *good = v->length; return r->err;
    }
    if (rfe < (off_t)(r->good_len / FRAME)) return MSPACK_ERR_OK;
    *good = v->init + r->good_len;
    return r->err;
  }
}

/* the emit step's sink: the bytes go to the output file, or into mspack_chmd_digest's hash */
static int emit_slice(struct chmd_p *self, struct mspack_file *fh, const unsigned char *p, size_t n)
{
  if (self->sink) { sink_update(self->sink, p, n); return MSPACK_ERR_OK; }
  return write_slice(self->system, fh, p, n);
}

/* write [from, to) of the uncompressed stream as the virtual decoder produced it */
static int vdec_emit(struct chmd_p *self, struct chm_p *c, struct mspack_file *fh, off_t from, off_t to)
{
  struct mspack_system *sys = self->system;
  struct vdec *v = &self->v;
  if (to <= from) return MSPACK_ERR_OK;
  if (v->serial) return emit_slice(self, fh, c->s_buf + (from - v->init), (size_t)(to - from));
  if (self->sink && self->sink_whole) {
    /* mspack_chmd_digest, [from, to) is the file's plain range: the digest its chunk's batch took of it, if it did and these
     * bytes are the fast results' (no interval of the range is decoded again with a shifted E8 origin, below).  The chunk is
     * asked for as the loop below asks (its results, its place in the LRU), only its bytes are not needed */
    unsigned int k = (unsigned int)(from / c->interval_bytes), k1 = (unsigned int)((to - 1) / c->interval_bytes), i;
    if (k / c->chunk_int == k1 / c->chunk_int) {
      struct chm_chunk *ch;
      int err, shifted = 0;
      if ((err = ensure_chunk_to(self, c, k, k1, 0, &ch))) return err;
      if (v->init != 0)
        for (i = k; i <= k1; i++) if (c->ires[i].flags & MSPACK_HIP_F_E8_APPLIED) shifted = 1;
      if (!shifted && (self->sink_kept = digest_table_find(&ch->dg, (uint64_t) from, (uint64_t)(to - from), self->sink->alg)) != NULL) return MSPACK_ERR_OK;
    }
  }
  while (from < to) {
    unsigned int k = (unsigned int)(from / c->interval_bytes), ci = k / c->chunk_int;
    unsigned int cfirst = ci * c->chunk_int, clast = cfirst + c->chunk_int - 1;   /* this chunk's intervals */
    off_t cend = ((off_t) clast + 1) * c->interval_bytes, stop = to < cend ? to : cend;
    unsigned int k1 = (unsigned int)((stop - 1) / c->interval_bytes), i;
    struct chm_chunk *ch;
    int err, shifted = 0;
    if ((err = ensure_chunk_to(self, c, k, k1, 1, &ch))) return err;
    /* E8: fast results have origin 0; the reference's origin is where its decoder was created (lzxd.c:712) */
    if (v->init != 0)
      for (i = k; i <= k1; i++) if (c->ires[i].flags & MSPACK_HIP_F_E8_APPLIED) shifted = 1;
    if (shifted) {
      unsigned int cnt = k1 - k + 1;
      mspack_hip_result *r2 = (mspack_hip_result *) sys->alloc(sys, cnt * sizeof(*r2));
      unsigned char *tmp = (unsigned char *) mspack_arena_alloc(sys, (size_t) cnt * (size_t) c->interval_bytes + 128);
      err = (!r2 || !tmp) ? MSPACK_ERR_NOMEMORY : decode_intervals(self, c, k, cnt, v->init, tmp, r2);
      if (!err) err = emit_slice(self, fh, tmp + (from - (off_t) k * c->interval_bytes), (size_t)(stop - from));
      sys->free(r2); mspack_arena_free(sys, tmp);
      if (err) return err;
    }
    else if ((err = emit_slice(self, fh, ch->buf + (from - (off_t) cfirst * c->interval_bytes), (size_t)(stop - from)))) return err;
    from = stop;
  }
  return MSPACK_ERR_OK;
}

static int chmd_extract(struct mschm_decompressor *base, struct mschmd_file *file, const char *filename)
{
  struct chmd_p *self = (struct chmd_p *) base;
  struct mspack_system *sys;
  struct chm_p *c;
  struct mspack_file *fh, *infh = NULL;

  if (!self) return MSPACK_ERR_ARGS;
  if (!file || !file->section) return self->error = MSPACK_ERR_ARGS;
  sys = self->system;
  c = (struct chm_p *) file->section->chm;

  if (!(infh = sys->open(sys, c->base.filename, MSPACK_SYS_OPEN_READ))) return self->error = MSPACK_ERR_OPEN;
  if (self->v_chm != c) { self->v_chm = c; self->v.alive = 0; }
  /* (mspack_chmd_digest: no output file; the lines extract() says with the output's handle are said without one) */
  if (self->sink) fh = NULL;
  else if (!(fh = sys->open(sys, filename, MSPACK_SYS_OPEN_WRITE))) { sys->close(infh); return self->error = MSPACK_ERR_OPEN; }
  if (!file->length) { if (fh) sys->close(fh); sys->close(infh); return self->error = MSPACK_ERR_OK; }
  self->error = MSPACK_ERR_OK;

  if (file->section->id == 0) {
    if (sys->seek(infh, c->base.sec0.offset + file->offset, MSPACK_SYS_SEEK_START)) self->error = MSPACK_ERR_SEEK;
    else {
      unsigned char buf[512];
      off_t length = file->length, maxlen = c->base.length - sys->tell(infh);
      if (length > maxlen) sys->message(fh, "WARNING; file is %lld bytes longer than CHM file", (long long)(length - maxlen));
      while (length > 0) {
        int run = length > (off_t) sizeof(buf) ? (int) sizeof(buf) : (int) length;
        if (sys->read(infh, buf, run) != run) { self->error = MSPACK_ERR_READ; break; }
        if (self->sink) sink_update(self->sink, buf, (size_t) run);
        else if (sys->write(fh, buf, run) != run) { self->error = MSPACK_ERR_WRITE; break; }
        length -= run;
      }
    }
  }
  else {
    struct vdec *v = &self->v;
    int err = MSPACK_ERR_OK;
    if (c->sec1_state == 0) {
      err = setup_sec1(self, c, infh);
      if (err) { free_sec1(sys, c); c->sec1_state = -err; } else c->sec1_state = 1;
    }
    else if (c->sec1_state < 0) err = -c->sec1_state;

    /* (re)create the decoder: none alive, or the request lies behind it (chmd.c:993-999) */
    if (!err && (!v->alive || file->offset < v->offset)) {
      off_t k0 = file->offset / c->interval_bytes;
      v->alive = 0;
      if (file->offset >= 0 && k0 < (off_t) c->n_fast) {
        v->mode = 0; v->init = k0 * c->interval_bytes; v->length = v->dlen = c->padded_len; v->in_off = c->ioff[k0];
        if (v->init > v->dlen) err = MSPACK_ERR_NOMEMORY;            /* lzxd_init(output_length < 0) == NULL (lzxd.c:297-300, chmd.c:1183-1187) */
        else if (v->init == v->dlen) v->length = (off_t) c->n_fast * c->interval_bytes;    /* output_length 0: every interval the table has */
      }
      else if (c->span_err) err = c->span_err;                              /* chmd.c:1159-1166 */
      else { v->mode = 1; v->init = 0; v->length = v->dlen = c->span_len; v->in_off = 0; }
      if (!err) { v->alive = 1; v->serial = (v->mode == 1); v->offset = v->decoded_end = v->init; v->seek_pending = 1; }
    }
    if (!err) {
      if (file->offset > v->dlen) err = MSPACK_ERR_DECRUNCH;                /* chmd.c:1002-1005; the decoder lives on */
      else if (v->seek_pending && sys->seek(infh, c->content_start + (off_t) v->in_off, MSPACK_SYS_SEEK_START))
        err = MSPACK_ERR_SEEK;                                              /* chmd.c:1008-1011; it lives on, too */
      else {
        off_t length = file->length, maxlen = v->dlen - file->offset, good = 0;
        v->seek_pending = 0;
        if (file->offset > v->offset) err = vdec_phase(self, c, v->offset, file->offset, &good);   /* skip */
        if (!err) {
          int werr;
          if (length > maxlen) {
            sys->message(fh, "WARNING; file is %lld bytes longer than compressed section", (long long)(length - maxlen));
            length = maxlen + 1;                        /* decodes what exists, then errors out */
          }
          err = vdec_phase(self, c, file->offset, file->offset + length, &good);                    /* emit */
          if (good > file->offset + length) good = file->offset + length;
          if (err != MSPACK_ERR_NOMEMORY && good > file->offset) {
            if (good > v->length) good = v->length;
            self->sink_whole = !err && length == file->length && good == file->offset + file->length;
            if ((werr = vdec_emit(self, c, fh, file->offset, good))) err = werr;
          }
        }
        if (err) v->alive = 0;                          /* chmd.c:1036-1040 */
        else v->offset = file->offset + length;
      }
    }
    self->error = err;
  }
  if (fh) sys->close(fh);
  sys->close(infh);
  return self->error;
}

/* mspack.h: extract() with the writes replaced by a hash */
int mspack_chmd_digest(struct mschm_decompressor *base, struct mschmd_file *file, int alg, unsigned char *digest, size_t digest_cap)
{
  struct chmd_p *self = (struct chmd_p *) base;
  struct digest_sink k;
  int err = digest_call_args(file, alg, digest, digest_cap);
  if (!self) return MSPACK_ERR_ARGS;
  if (err) return self->error = err;
  sink_init(&k, alg);
  self->sink = &k; self->sink_whole = 0; self->sink_kept = NULL;
  err = chmd_extract(base, file, NULL);
  self->sink = NULL;
  if (err == MSPACK_ERR_OK) digest_call_done(&k, self->sink_kept, digest, g_digest_counts);
  self->sink_whole = 0; self->sink_kept = NULL;
  return err;
}

/* mspack.h: extract() with the writes replaced by zlib's CRC-32 */
int mspack_chmd_crc32(struct mschm_decompressor *base, struct mschmd_file *file, unsigned int *crc)
{
  struct chmd_p *self = (struct chmd_p *) base;
  struct digest_sink k;
  int err = crc32_call_args(file, crc);
  if (!self) return MSPACK_ERR_ARGS;
  if (err) return self->error = err;
  sink_init(&k, DIGEST_ALG_CRC32);
  self->sink = &k; self->sink_whole = 0; self->sink_kept = NULL;
  err = chmd_extract(base, file, NULL);
  self->sink = NULL;
  if (err == MSPACK_ERR_OK) crc32_call_done(&k, self->sink_kept, crc, g_crc32_counts);
  self->sink_whole = 0; self->sink_kept = NULL;
  return err;
}

void mspack_chmd_crc32_counts(unsigned long long counts[2], int reset) { crc32_counts_get(g_crc32_counts, counts, reset); }

void mspack_chmd_digest_counts(int alg, unsigned long long counts[2], int reset) { digest_counts_get(g_digest_counts, alg, counts, reset); }

void mspack_chmd_batch_counts(unsigned long long counts[2], int reset)
{
  int i;
  for (i = 0; i < 2; i++) {
    if (counts) counts[i] = __atomic_load_n(&g_batch_counts[i], __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(&g_batch_counts[i], 0ull, __ATOMIC_RELAXED);
  }
}

/* ---- mspack_chmd_prefetch (mspack.h) ---------------------------------------------------------------------------------------------- */
/* section 1 of a CHM that has not had it, for the prefetch: what extract() does first, but a CHM whose setup fails is left as it
 * was -- no failure is cached, its next extract() sets it up again and reports.  (setup_sec1 and what it calls say nothing through
 * sys->message; the directory chunks and system-file entries it looked up stay cached, as after any fast_find().) */
static void prefetch_setup(struct chmd_p *self, struct chm_p *c)
{
  struct mspack_system *sys = self->system;
  struct mspack_file *fh = sys->open(sys, c->base.filename, MSPACK_SYS_OPEN_READ);
  if (!fh) return;
  if (setup_sec1(self, c, fh)) free_sec1(sys, c); else c->sec1_state = 1;
  sys->close(fh);
}

int mspack_chmd_prefetch(struct mschm_decompressor *base, struct mschmd_header **chms, int n_chms)
{
  struct chmd_p *self = (struct chmd_p *) base;
  struct mspack_system *sys;
  struct chm_p **list;
  struct chm_pick *pk = NULL;
  const uint64_t in_limit = (uint64_t) 1 << 34;             /* what in_chunk * 4 can address */
  uint64_t in_total = 0;
  size_t budget, used = 0, n_list = 0, cap = 0, n = 0, l;
  unsigned int first, count;
  int i, err = MSPACK_ERR_OK, stop = 0;
  if (!self) return MSPACK_ERR_ARGS;
  if (n_chms < 0 || (n_chms > 0 && !chms)) return self->error = MSPACK_ERR_ARGS;
  for (i = 0; i < n_chms; i++) if (!chms[i]) return self->error = MSPACK_ERR_ARGS;
  if (n_chms == 0) return self->error = MSPACK_ERR_OK;
  sys = self->system;
  budget = (size_t) mspack_hip_cache_mb() << 20;
  if (!(list = (struct chm_p **) sys->alloc(sys, (size_t) n_chms * sizeof(*list)))) return self->error = MSPACK_ERR_NOMEMORY;
  /* every CHM once, section 1 set up; the decoded bytes they hold already count against the budget */
  if (!++self->pf_stamp) ++self->pf_stamp;
  for (i = 0; i < n_chms; i++) {
    struct chm_p *c = (struct chm_p *) chms[i];
    unsigned int ci;
    if (c->pf_stamp == self->pf_stamp) continue;
    c->pf_stamp = self->pf_stamp;
    if (c->sec1_state == 0) prefetch_setup(self, c);
    if (c->sec1_state != 1) continue;                       /* (a failure extract() has cached already, or found just now: skipped) */
    for (ci = 0; ci < c->n_chunks; ci++) {
      chunk_span(c, ci, &first, &count);
      if (c->chunks[ci].buf) used += (size_t) count * (size_t) c->interval_bytes;
    }
    cap += c->n_chunks;
    list[n_list++] = c;
  }
  if (cap && !(pk = (struct chm_pick *) sys->alloc(sys, cap * sizeof(*pk)))) { sys->free(list); return self->error = MSPACK_ERR_NOMEMORY; }
  /* the chunks: argument order, chunk order, while they fit the budget and the input arena stays addressable */
  for (l = 0; l < n_list && !stop; l++) {
    struct chm_p *c = list[l];
    const uint64_t piece = ((uint64_t) c->arena_room + 15) & ~(uint64_t) 15;
    uint64_t in_base = 0;
    unsigned int ci;
    int placed = 0;
    for (ci = 0; ci < c->n_chunks; ci++) {
      struct chm_chunk *ch = &c->chunks[ci];
      size_t bytes;
      chunk_span(c, ci, &first, &count);
      bytes = (size_t) count * (size_t) c->interval_bytes;
      if (ch->buf || ch->res_valid) continue;                 /* decoded already (a chunk of a batch that still runs has its buf) */
      if (used + bytes > budget) { stop = 1; break; }
      if (!placed) {
        if (in_total + piece + 64 > in_limit) { stop = 1; break; }
        in_base = in_total; in_total += piece; placed = 1;
      }
      pk[n].c = c; pk[n].ch = ch; pk[n].first = first; pk[n].count = count; pk[n].in_base = in_base;
      used += bytes;
      n++;
    }
  }
  /* (nothing left to decode: no batch.)  The batch has a copy of the arenas: close() of one of these CHMs does not wait for it */
  if (n) err = issue_batch(self, pk, n, in_total, 1);
  sys->free(pk); sys->free(list);
  return self->error = err;
}

int mspack_chmd_set_param(struct mschm_decompressor *base, int param, int value)
{
  struct chmd_p *self = (struct chmd_p *) base;
  if (!self) return MSPACK_ERR_ARGS;
  if (param == MSCHMD_PARAM_HIP_CRC32) { if (value != 0 && value != 1) return MSPACK_ERR_ARGS; self->hip_crc32 = value; return MSPACK_ERR_OK; }
  if (param == MSCHMD_PARAM_HIP_DIGESTS64) { if (value & ~(MSPACK_DIGEST_SHA384 | MSPACK_DIGEST_SHA512)) return MSPACK_ERR_ARGS; self->hip_digests64 = value; return MSPACK_ERR_OK; }
  if (param != MSCHMD_PARAM_HIP_DIGESTS || value < 0 || value > 7) return MSPACK_ERR_ARGS;
  self->hip_digests = value;
  return MSPACK_ERR_OK;
}

int mspack_chmd_get_param(struct mschm_decompressor *base, int param, int *value)
{
  struct chmd_p *self = (struct chmd_p *) base;
  if (!self || !value || (param != MSCHMD_PARAM_HIP_DIGESTS && param != MSCHMD_PARAM_HIP_CRC32 && param != MSCHMD_PARAM_HIP_DIGESTS64)) return MSPACK_ERR_ARGS;
  *value = param == MSCHMD_PARAM_HIP_CRC32 ? self->hip_crc32 : param == MSCHMD_PARAM_HIP_DIGESTS64 ? self->hip_digests64 : self->hip_digests;
  return MSPACK_ERR_OK;
}

static int chmd_error(struct mschm_decompressor *base) {
  struct chmd_p *self = (struct chmd_p *) base;
  return self ? self->error : MSPACK_ERR_ARGS;
}

struct mschm_decompressor *mspack_create_chm_decompressor(struct mspack_system *sys)
{
  struct chmd_p *self;
  if (!sys) sys = mspack_default_system;
  if (!mspack_valid_system(sys)) return NULL;
  if (!(self = (struct chmd_p *) sys->alloc(sys, sizeof(*self)))) return NULL;
  memset(self, 0, sizeof(*self));
  self->base.open = &chmd_open;
  self->base.close = &chmd_close;
  self->base.extract = &chmd_extract;
  self->base.last_error = &chmd_error;
  self->base.fast_open = &chmd_fast_open;
  self->base.fast_find = &chmd_fast_find;
  self->system = sys;
  self->error = MSPACK_ERR_OK;
  return &self->base;
}

void mspack_destroy_chm_decompressor(struct mschm_decompressor *base)
{
  struct chmd_p *self = (struct chmd_p *) base;
  if (!self) return;
  /* batches that still run are settled, and the output buffers that CHMs which were never closed still use are freed -- those
   * chunks count as not decoded from here on */
  while (self->batches) {
    struct chm_batch *B = self->batches;
    size_t k;
    for (k = 0; k < B->n; k++) {
      struct chm_chunk *ch = B->m[k].ch;
      if (ch) { ch->bat = NULL; ch->bat_run = 0; ch->buf = NULL; ch->res_valid = 0; }
    }
    batch_free(self->system, B);
  }
  self->system->free(self);
}
