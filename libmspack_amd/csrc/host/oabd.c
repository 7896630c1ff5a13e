/* oabd.c -- OAB (Offline Address Book, ".LZX") driver of the libmspack-compatible API, on the GPU batch
 * decoder.
 *
 * Mirrors the behaviour of the reference's oabd.c:
 *   full files ....... header (version 3.1, block_max, target_size), then blocks of 16-byte header
 *                      (flags, compressed size, uncompressed size, CRC) + data .... oabd.c:103-237
 *   patch files ...... header (version 3.2), blocks (patch size, target size, source size, CRC); every
 *                      block is an LZX DELTA stream whose reference data is the next `source size`
 *                      bytes of the base file ..................................... oabd.c:239-382
 *   window per block . 17 bits, grown until it holds the block (plus the rounded-up source) .. :191-194,:329-334
 *   CRC .............. reflected CRC-32 (edb88320) from 0xffffffff, NOT inverted at the end,
 *                      over the bytes written .................................... oabd.c:88-100, crc32.h
 * but not its control flow: every compressed block is its own lzxd_init (oabd.c:199, :340), i.e. an
 * independent unit, so ALL blocks of a file -- and, through mspack_oabd_decompress_many (mspack.h), of MANY files -- are decoded
 * in ONE GPU batch (MSPACK_HIP_KIND_LZX_DELTA) and each file is then replayed in order: each block's bytes are written, its error
 * (if any) returned at the point where the reference would have returned it.
 *
 * A file is a job, and a job takes three steps:
 *   gather ... open the input, check the header, open the base; walk the block headers and read the blocks' bytes to the end of the
 *              batch's input arena; lay the job's units out at the end of the batch's output arena and read each block's reference
 *              slice from the base to right below its unit; close input and base.
 *   decode ... one unit table over the blocks of all gathered jobs, one mspack_hip_decode_batch().
 *   replay ... in job order: open the output, write, compare the CRCs, close.
 * decompress() and decompress_incremental() are a batch of one job.
 */
#include <stdlib.h>
#include <stdio.h>
#include "host_common.h"

struct oabd_p {
  struct msoab_decompressor base;
  struct mspack_system *system;
  int buf_size;
};

struct oab_blk {
  unsigned int csize, dsize, ssize, crc;
  int compressed;
  int window_bits;
  size_t in_pos, in_have;             /* compressed / stored bytes in the arena; how many the file held */
  int ref_err;                        /* patch: error while fetching the reference data              */
  size_t out_off;                     /* compressed blocks: the unit's output in the output arena     */
  mspack_hip_result res;              /* ... and what the batch answered for it                      */
};

/* one file of a batch */
struct oab_job {
  const char *input, *base, *output;
  int patch;                          /* decompress_incremental's job: `base` is read */
  unsigned int in_hash, base_hash, out_hash;
  int early;                          /* gather's answer from before the output exists: open, header, signature, base */
  int late;                           /* its answer once the output exists and before a block is written (no memory)  */
  int tail_err;                       /* the structural problem that ended the walk: reported behind the blocks before it */
  int failed;                         /* the batch of this job alone failed; `why` is the provider's text             */
  char why[256];
  size_t blk0, n_blks;                /* its blocks in the batch's table, in file order */
  size_t in0, out0;                   /* where its part of the input / output arena begins (16-byte aligned) */
  struct mspack_file *outfh;          /* a job that names its own input or base as its output: opened at gather, as ever */
};

/* the batch now open: the blocks of the jobs gathered so far, their bytes, and the output arena with the reference slices in place */
struct oab_batch {
  struct mspack_system *sys;
  int buf_size, dev_crc, many;
  unsigned char *in, *out;
  size_t in_cap, out_cap, in_bytes, out_bytes;
  struct oab_blk *blks;
  size_t n_blks, cap_blks;
};

/* The provider of the batch ABI this driver is linked with may be older than MSPACK_HIP_UF_CRC32 (or a CPU stand-in that never
 * learnt it): the capability call is a weak reference, and a provider that does not have it is asked for nothing new. */
extern unsigned mspack_hip_features(void) __attribute__((weak));

/* mspack_oabd_batch_counts (mspack.h): batch calls issued, jobs that went out in a batch of mspack_oabd_decompress_many, jobs decoded
 * again alone because their shared batch failed */
static unsigned long long g_oab_counts[3];
static void count_add(unsigned long long *c, unsigned long long n) { __atomic_fetch_add(c, n, __ATOMIC_RELAXED); }
void mspack_oabd_batch_counts(unsigned long long counts[3], int reset)
{
  int i;
  for (i = 0; i < 3; i++) {
    if (counts) counts[i] = __atomic_load_n(&g_oab_counts[i], __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(&g_oab_counts[i], 0ull, __ATOMIC_RELAXED);
  }
}

static unsigned int crc_table[256];
static void crc_init(void) {
  unsigned int i, k;
  if (crc_table[1]) return;
  for (i = 0; i < 256; i++) {
    unsigned int c = i;
    for (k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
    crc_table[i] = c;
  }
}
static unsigned int crc_update(unsigned int c, const unsigned char *p, size_t n) {
  while (n--) c = crc_table[(c ^ *p++) & 0xFF] ^ (c >> 8);
  return c;
}

/* read up to `want` bytes; returns the count (short at end of file), -1 on a read error */
static long read_upto(struct mspack_system *sys, struct mspack_file *fh, unsigned char *dst, size_t want) {
  size_t got = 0;
  while (got < want) {
    int run = (want - got) > (1u << 20) ? (1 << 20) : (int)(want - got);
    int r = sys->read(fh, dst + got, run);
    if (r < 0) return -1;
    if (r == 0) break;
    got += (size_t) r;
  }
  return (long) got;
}

/* a file name's hash (FNV-1a): the order-dependence check compares these before it compares strings */
static unsigned int name_hash(const char *s) {
  unsigned int h = 2166136261u;
  while (s && *s) h = (h ^ (unsigned char) *s++) * 16777619u;
  return h;
}

static int same_name(const char *a, const char *b) { return a && b && !strcmp(a, b); }

/* make *arena hold `need` bytes, its first `keep` bytes kept; 0 = no memory (the arena is then as it was) */
static int arena_grow(struct mspack_system *sys, unsigned char **arena, size_t *cap, size_t keep, size_t need, size_t ncap) {
  unsigned char *n;
  if (need <= *cap) return 1;
  if (!(n = (unsigned char *) sys->alloc(sys, ncap))) return 0;
  if (*arena) { if (keep) sys->copy(*arena, n, keep); sys->free(*arena); }
  *arena = n; *cap = ncap;
  return 1;
}

/* ---- gather: one job's blocks, bytes and reference slices, behind those of the jobs before it ---------------------------------- */
static void oab_gather(struct oab_batch *B, struct oab_job *jb, int open_output)
{
  struct mspack_system *sys = B->sys;
  struct mspack_file *infh = NULL, *basefh = NULL;
  const int patch = jb->patch;
  const size_t in_was = B->in_bytes, out_was = B->out_bytes;
  unsigned char hdr[0x1c], bh[16];
  unsigned int block_max, target_size;
  const unsigned int hsize = patch ? 0x1c : 0x10;
  size_t k;

  jb->early = jb->late = jb->tail_err = MSPACK_ERR_OK; jb->failed = 0; jb->outfh = NULL;
  /* (where its first block and its first unit will begin: both loops below round up first) */
  jb->blk0 = B->n_blks; jb->n_blks = 0; jb->in0 = (in_was + 15) & ~(size_t) 15; jb->out0 = (out_was + 15) & ~(size_t) 15;

  if (!(infh = sys->open(sys, jb->input, MSPACK_SYS_OPEN_READ))) { jb->early = MSPACK_ERR_OPEN; return; }
  if (sys->read(infh, hdr, (int) hsize) != (int) hsize) { jb->early = MSPACK_ERR_READ; goto out; }
  if (rd_le32(hdr) != 3 || rd_le32(hdr + 4) != (patch ? 2u : 1u)) { jb->early = MSPACK_ERR_SIGNATURE; goto out; }
  block_max = rd_le32(hdr + 8);
  target_size = rd_le32(hdr + (patch ? 0x10 : 0x0c));
  if (patch) {
    if (block_max < 16) block_max = 16;                     /* oabd.c:283-285 */
    if (!(basefh = sys->open(sys, jb->base, MSPACK_SYS_OPEN_READ))) { jb->early = MSPACK_ERR_OPEN; goto out; }
  }
  /* (the reference opens the output here.  Nothing between here and the replay can fail before it, so the replay opens it and
   * answers the same -- except when the output IS the input or the base: then opening it changes what is read below) */
  if (open_output && !(jb->outfh = sys->open(sys, jb->output, MSPACK_SYS_OPEN_WRITE))) { jb->early = MSPACK_ERR_OPEN; goto out; }

  /* walk the block headers in file order, gather every block's bytes.  The first structural
   * problem ends the walk; it is reported once the blocks before it have been replayed. */
  while (target_size) {
    struct oab_blk b;
    long got;
    size_t room, want;
    memset(&b, 0, sizeof(b));
    if (sys->read(infh, bh, 16) != 16) { jb->tail_err = MSPACK_ERR_READ; break; }
    if (patch) {
      b.csize = rd_le32(bh); b.dsize = rd_le32(bh + 4); b.ssize = rd_le32(bh + 8); b.crc = rd_le32(bh + 12);
      b.compressed = 1;
      if (b.dsize > block_max || b.dsize > target_size || b.ssize > block_max) { jb->tail_err = MSPACK_ERR_DATAFORMAT; break; }
    }
    else {
      unsigned int flags = rd_le32(bh);
      b.csize = rd_le32(bh + 4); b.dsize = rd_le32(bh + 8); b.crc = rd_le32(bh + 12);
      if (b.dsize > block_max || b.dsize > target_size || flags > 1) { jb->tail_err = MSPACK_ERR_DATAFORMAT; break; }
      b.compressed = (int) flags;
      if (!flags && b.dsize != b.csize) { jb->tail_err = MSPACK_ERR_DATAFORMAT; break; }
    }
    if (b.compressed) {
      unsigned int wsz = patch ? (((b.ssize + 32767u) & ~32767u) + b.dsize) : b.dsize;
      b.window_bits = 17;
      while (b.window_bits < 25 && (1u << b.window_bits) < wsz) b.window_bits++;
    }
    /* the block's bytes (compressed stream, or the stored data) */
    B->in_bytes = (B->in_bytes + 15) & ~(size_t) 15;
    /* csize is untrusted: never reserve more than the file still holds (a 32-byte file must not be able to
     * ask for gigabytes; the reference streams with window-sized memory) */
    {
      off_t flen = 0, here = sys->tell(infh);
      want = (size_t) b.csize;
      if (!mspack_sys_filelen(sys, infh, &flen) && flen >= here && (off_t) want > flen - here) want = (size_t)(flen - here);
      room = want + 64;
    }
    if (!arena_grow(sys, &B->in, &B->in_cap, B->in_bytes, B->in_bytes + room, (B->in_bytes + room) * 2 + 65536)) goto nomem;
    got = read_upto(sys, infh, B->in + B->in_bytes, want);
    if (got < 0) { jb->tail_err = MSPACK_ERR_READ; break; }
    b.in_pos = B->in_bytes; b.in_have = (size_t) got;
    memset(B->in + B->in_bytes + got, 0, 64);
    B->in_bytes += (size_t) got + 16;
    if (B->n_blks == B->cap_blks) {
      size_t nc = B->cap_blks ? B->cap_blks * 2 : 64;
      struct oab_blk *n = (struct oab_blk *) sys->alloc(sys, nc * sizeof(*n));
      if (!n) goto nomem;
      if (B->blks) { sys->copy(B->blks, n, B->n_blks * sizeof(*n)); sys->free(B->blks); }
      B->blks = n; B->cap_blks = nc;
    }
    B->blks[B->n_blks++] = b; jb->n_blks++;
    target_size -= b.dsize;
    if ((size_t) got < b.csize) break;                       /* the file ends inside this block */
  }

  /* the job's units: output regions back to back, each preceded by room for its reference data */
  for (k = 0; k < jb->n_blks; k++) {
    struct oab_blk *b = &B->blks[jb->blk0 + k];
    if (!b->compressed) continue;
    B->out_bytes = (B->out_bytes + 15) & ~(size_t) 15;
    B->out_bytes += ((size_t) b->ssize + 15) & ~(size_t) 15;
    b->out_off = B->out_bytes;
    B->out_bytes += b->dsize;
  }
  if (B->out_bytes > out_was) {
    /* (a batch of one file gets exactly what it needs, as ever; one that grows over many files doubles) */
    const size_t need = B->out_bytes + 64;
    if (!arena_grow(sys, &B->out, &B->out_cap, out_was, need, out_was ? need * 2 + 65536 : need)) goto nomem;
  }
  /* patch: each block's reference data is the next `source size` bytes of the base file (oabd.c:346) */
  if (patch) {
    int base_dead = 0;
    for (k = 0; k < jb->n_blks; k++) {
      struct oab_blk *b = &B->blks[jb->blk0 + k];
      if (b->ssize == 0) continue;
      if (base_dead) { b->ref_err = MSPACK_ERR_READ; continue; }
      if (read_upto(sys, basefh, B->out + b->out_off - b->ssize, b->ssize) != (long) b->ssize) {
        b->ref_err = MSPACK_ERR_READ; base_dead = 1;
      }
    }
  }
  goto out;

nomem:                                                      /* the job leaves the batch: nothing of it is decoded or written */
  jb->late = MSPACK_ERR_NOMEMORY;
  B->n_blks = jb->blk0; jb->n_blks = 0; B->in_bytes = in_was; B->out_bytes = out_was;
out:
  if (basefh) sys->close(basefh);
  sys->close(infh);
}

/* ---- decode: the blocks of jobs[0 .. nj) in one batch ----------------------------------------------------------------------- */
/* blocks whose reference data could not be read and empty blocks are kept out of the batch */
static int oab_in_batch(const struct oab_blk *b) { return b->compressed && !b->ref_err && b->dsize != 0; }

enum { OAB_DECODED = 0, OAB_BATCH_FAILED = 1, OAB_NO_MEMORY = 2 };
static int oab_decode_once(struct oab_batch *B, struct oab_job *jobs, size_t nj)
{
  struct mspack_system *sys = B->sys;
  mspack_hip_unit *sel;
  mspack_hip_result *rsel;
  size_t j, k, nsel = 0;
  int rc;
  for (j = 0; j < nj; j++)
    for (k = 0; k < jobs[j].n_blks; k++) nsel += (size_t) oab_in_batch(&B->blks[jobs[j].blk0 + k]);
  if (!nsel) return OAB_DECODED;
  sel = (mspack_hip_unit *) sys->alloc(sys, nsel * sizeof(*sel));
  rsel = (mspack_hip_result *) sys->alloc(sys, nsel * sizeof(*rsel));
  if (!sel || !rsel) { sys->free(sel); sys->free(rsel); return OAB_NO_MEMORY; }
  memset(sel, 0, nsel * sizeof(*sel)); memset(rsel, 0, nsel * sizeof(*rsel));
  nsel = 0;
  for (j = 0; j < nj; j++)
    for (k = 0; k < jobs[j].n_blks; k++) {
      const struct oab_blk *b = &B->blks[jobs[j].blk0 + k];
      mspack_hip_unit *u;
      if (!oab_in_batch(b)) continue;
      u = &sel[nsel++];
      u->in_off = b->in_pos; u->in_len = (uint32_t) b->in_have;
      u->out_off = b->out_off; u->out_len = b->dsize;
      u->kind = MSPACK_HIP_KIND_LZX_DELTA; u->window_bits = (uint8_t) b->window_bits;
      u->ref_len = b->ssize;
      if (B->dev_crc) u->flags |= MSPACK_HIP_UF_CRC32;
    }
  rc = mspack_hip_decode_batch(sel, nsel, B->in, B->in_bytes + 48, B->out, B->out_bytes + 64, rsel);
  count_add(&g_oab_counts[0], 1);
  if (rc) {
    if (nj == 1) { jobs[0].failed = 1; snprintf(jobs[0].why, sizeof(jobs[0].why), "%s", mspack_hip_last_error()); }
  }
  else {
    nsel = 0;
    for (j = 0; j < nj; j++)
      for (k = 0; k < jobs[j].n_blks; k++) {
        struct oab_blk *b = &B->blks[jobs[j].blk0 + k];
        if (oab_in_batch(b)) b->res = rsel[nsel++];
      }
  }
  sys->free(sel); sys->free(rsel);
  return rc ? OAB_BATCH_FAILED : OAB_DECODED;
}

static void oab_decode(struct oab_batch *B, struct oab_job *jobs, size_t nj)
{
  size_t j, k;
  int st = oab_decode_once(B, jobs, nj);
  if (B->many)
    for (j = 0; j < nj; j++)
      for (k = 0; k < jobs[j].n_blks; k++)
        if (oab_in_batch(&B->blks[jobs[j].blk0 + k])) { count_add(&g_oab_counts[1], 1); break; }
  if (st == OAB_DECODED) return;
  if (nj == 1) { if (st == OAB_NO_MEMORY) jobs[0].late = MSPACK_ERR_NOMEMORY; return; }
  /* a shared batch failed: one bad file must not change its neighbours' answers -- each job again, in a batch of its own */
  for (j = 0; j < nj; j++) {
    if (st == OAB_BATCH_FAILED) count_add(&g_oab_counts[2], 1);
    if (oab_decode_once(B, &jobs[j], 1) == OAB_NO_MEMORY) jobs[j].late = MSPACK_ERR_NOMEMORY;
  }
}

/* ---- replay: one job's file in order ---------------------------------------------------------------------------------------- */
static int oab_replay(struct oab_batch *B, struct oab_job *jb)
{
  struct mspack_system *sys = B->sys;
  struct mspack_file *outfh = jb->outfh;
  int ret = jb->late;
  size_t k;
  if (jb->early) return jb->early;
  if (!outfh && !(outfh = sys->open(sys, jb->output, MSPACK_SYS_OPEN_WRITE))) return MSPACK_ERR_OPEN;
  if (!ret && jb->failed) {
    sys->message(NULL, "GPU batch decode failed: %s", jb->why);
    ret = MSPACK_ERR_DECRUNCH;
  }
  for (k = 0; k < jb->n_blks && !ret; k++) {
    struct oab_blk *b = &B->blks[jb->blk0 + k];
    if (!b->compressed) {
      /* copy_fh (oabd.c:384-403): buf_size pieces; a piece the file does not fully hold is not written */
      size_t whole = b->in_have;
      if (whole < b->dsize) whole -= whole % (size_t) B->buf_size;
      if (write_slice(sys, outfh, B->in + b->in_pos, whole < b->dsize ? whole : b->dsize)) ret = MSPACK_ERR_WRITE;
      else if (b->in_have < b->dsize) ret = MSPACK_ERR_READ;
      continue;
    }
    if (b->ref_err) { ret = b->ref_err; break; }                            /* lzxd_set_reference_data */
    {
      const mspack_hip_result *r = &b->res;
      unsigned int n = b->dsize ? r->out_len : 0;
      int err = b->dsize ? r->err : MSPACK_ERR_OK;
      if (n > b->dsize) n = b->dsize;
      if (write_slice(sys, outfh, B->out + b->out_off, n)) { ret = MSPACK_ERR_WRITE; break; }
      if (err) { ret = err; break; }
      if (b->in_have < b->csize) { ret = MSPACK_ERR_READ; break; }            /* the padding skip fails */
      /* (the device's digest covers r->out_len bytes: a block that produced more than it may write is summed here) */
      if ((B->dev_crc && b->dsize && n == r->out_len ? r->in_used : crc_update(0xffffffffu, B->out + b->out_off, n)) != b->crc) { ret = MSPACK_ERR_CHECKSUM; break; }
    }
  }
  if (!ret) ret = jb->tail_err;
  sys->close(outfh);
  return ret;
}

/* decode and replay the open batch, jobs[0 .. nj); `keep`, the job gathered behind them, moves to the front of the emptied arenas */
static void oab_flush(struct oab_batch *B, struct oab_job *jobs, size_t nj, struct oab_job *keep, int *errors)
{
  size_t j, k;
  oab_decode(B, jobs, nj);
  for (j = 0; j < nj; j++) errors[j] = oab_replay(B, &jobs[j]);
  if (!keep) { B->n_blks = B->in_bytes = B->out_bytes = 0; return; }
  for (k = 0; k < keep->n_blks; k++) {
    struct oab_blk *b = &B->blks[k];
    *b = B->blks[keep->blk0 + k];
    b->in_pos -= keep->in0;
    if (b->compressed) b->out_off -= keep->out0;
  }
  B->n_blks = keep->n_blks;
  B->in_bytes = B->in_bytes > keep->in0 ? B->in_bytes - keep->in0 : 0;            /* (a job without blocks or units begins behind the end) */
  B->out_bytes = B->out_bytes > keep->out0 ? B->out_bytes - keep->out0 : 0;
  if (B->in_bytes) memmove(B->in, B->in + keep->in0, B->in_bytes + 48);
  if (B->out_bytes) memmove(B->out, B->out + keep->out0, B->out_bytes);
  keep->blk0 = keep->in0 = keep->out0 = 0;
}

/* jobs[0 .. n) in order, as few batches as the three rules of mspack_oabd_decompress_many (mspack.h) allow; errors[k]: job k's answer */
static void oab_run(struct oabd_p *self, struct oab_job *jobs, int n, int *errors, int many)
{
  const size_t budget = (size_t) mspack_hip_cache_mb() << 20;
  struct oab_batch B;
  int first = 0, j, k;
  memset(&B, 0, sizeof(B));
  B.sys = self->system; B.buf_size = self->buf_size; B.many = many;
  /* the blocks' CRCs on the device, behind their decode (result.in_used), where the provider can; else crc_update */
  B.dev_crc = mspack_hip_features && (mspack_hip_features() & MSPACK_HIP_FEAT_CRC32);
  crc_init();
  for (j = 0; j < n; j++) {
    struct oab_job *jb = &jobs[j];
    int own, after = 0;
    jb->in_hash = name_hash(jb->input); jb->out_hash = name_hash(jb->output); jb->base_hash = name_hash(jb->base);
    own = same_name(jb->input, jb->output) || (jb->patch && same_name(jb->base, jb->output));
    /* order dependence: a job that reads what a job of the open batch writes waits for that batch's replay */
    for (k = first; k < j && !after; k++)
      after = (jobs[k].out_hash == jb->in_hash && same_name(jobs[k].output, jb->input)) ||
              (jb->patch && jobs[k].out_hash == jb->base_hash && same_name(jobs[k].output, jb->base));
    if (j > first && (after || own)) { oab_flush(&B, &jobs[first], (size_t)(j - first), NULL, &errors[first]); first = j; }
    oab_gather(&B, jb, own);
    /* budget: the job that takes the arenas past it starts the next batch (alone it runs whatever its size, as ever) */
    if (j > first && B.in_bytes + B.out_bytes > budget) { oab_flush(&B, &jobs[first], (size_t)(j - first), jb, &errors[first]); first = j; }
    if (own) { oab_flush(&B, jb, 1, NULL, &errors[j]); first = j + 1; }
  }
  if (first < n) oab_flush(&B, &jobs[first], (size_t)(n - first), NULL, &errors[first]);
  self->system->free(B.blks); self->system->free(B.in); self->system->free(B.out);
}

static int oab_one(struct msoab_decompressor *base, const char *input, const char *basefile, const char *output, int patch)
{
  struct oabd_p *self = (struct oabd_p *) base;
  struct oab_job *jb;
  int err = MSPACK_ERR_NOMEMORY;
  if (!self) return MSPACK_ERR_ARGS;
  if (!(jb = (struct oab_job *) self->system->alloc(self->system, sizeof(*jb)))) return err;
  memset(jb, 0, sizeof(*jb));
  jb->input = input; jb->base = basefile; jb->output = output; jb->patch = patch;
  oab_run(self, jb, 1, &err, 0);
  self->system->free(jb);
  return err;
}
static int oabd_decompress(struct msoab_decompressor *base, const char *input, const char *output) {
  return oab_one(base, input, NULL, output, 0);
}
static int oabd_decompress_incremental(struct msoab_decompressor *base, const char *input, const char *basefile,
                                       const char *output) {
  return oab_one(base, input, basefile, output, 1);
}

int mspack_oabd_decompress_many(struct msoab_decompressor *base, struct msoabd_job *jobs, int n)
{
  struct oabd_p *self = (struct oabd_p *) base;
  struct oab_job *st;
  int *errors, k;
  if (!self || n < 0 || (n > 0 && !jobs)) return MSPACK_ERR_ARGS;
  for (k = 0; k < n; k++) if (!jobs[k].input || !jobs[k].output) return MSPACK_ERR_ARGS;
  if (!n) return MSPACK_ERR_OK;
  st = (struct oab_job *) self->system->alloc(self->system, (size_t) n * sizeof(*st));
  errors = (int *) self->system->alloc(self->system, (size_t) n * sizeof(*errors));
  if (!st || !errors) { self->system->free(st); self->system->free(errors); return MSPACK_ERR_NOMEMORY; }
  memset(st, 0, (size_t) n * sizeof(*st));
  for (k = 0; k < n; k++) { st[k].input = jobs[k].input; st[k].base = jobs[k].base; st[k].output = jobs[k].output; st[k].patch = jobs[k].base != NULL; }
  oab_run(self, st, n, errors, 1);
  for (k = 0; k < n; k++) jobs[k].error = errors[k];
  self->system->free(st); self->system->free(errors);
  return MSPACK_ERR_OK;
}

static int oabd_param(struct msoab_decompressor *base, int param, int value) {
  struct oabd_p *self = (struct oabd_p *) base;
  if (self && param == MSOABD_PARAM_DECOMPBUF && value >= 16) { self->buf_size = value; return MSPACK_ERR_OK; }
  return MSPACK_ERR_ARGS;
}

struct msoab_decompressor *mspack_create_oab_decompressor(struct mspack_system *sys)
{
  struct oabd_p *self;
  if (!sys) sys = mspack_default_system;
  if (!mspack_valid_system(sys)) return NULL;
  if (!(self = (struct oabd_p *) sys->alloc(sys, sizeof(*self)))) return NULL;
  self->base.decompress = &oabd_decompress;
  self->base.decompress_incremental = &oabd_decompress_incremental;
  self->base.set_param = &oabd_param;
  self->system = sys;
  self->buf_size = 4096;
  return &self->base;
}

void mspack_destroy_oab_decompressor(struct msoab_decompressor *base)
{
  struct oabd_p *self = (struct oabd_p *) base;
  if (self) self->system->free(self);
}
