/* szdd_kwaj.c -- SZDD and KWAJ drivers of the libmspack-compatible API (include/mspack.h), on the GPU
 * batch decoder.
 *
 * Mirrors the reference's szddd.c and kwajd.c:
 *   SZDD headers (normal "SZDD\x88\xF0\x27\x33" 'A' missing-char length, QBasic "SZ \x88\xF0\x27\x33\xD1"
 *   length) and their error codes ............................................ szddd.c:140-170
 *   KWAJ header, optional fields (length, two unknown fields, 8.3 name parts, extra text) and their
 *   error codes .............................................................. kwajd.c:155-250
 *   open() keeps the input file open until close() (szddd.c:72-107, kwajd.c:93-147)
 *   extract(): seek to the data, open the output, decode, close the output .... szddd.c:177-214, kwajd.c:257-331
 *   methods: SZDD = LZSS (EXPAND or QBASIC start position); KWAJ 0 copy, 1 XOR 0xFF, 2 LZSS (QBASIC),
 *   3 LZH, 4 MSZIP blocks framed by 16-bit lengths
 * The stored methods (KWAJ 0/1) are copies and run on the host like the reference's; everything coded is
 * ONE unit for the batch decoder (MSPACK_HIP_KIND_LZSS / _KWAJ_LZH / MSZIP with MSPACK_HIP_UF_MSZIP_KWAJ).
 * None of these streams carries a length the decoder uses: the unit gets room for the largest possible
 * expansion (LZSS: 18 bytes per 2 input bytes; LZH: 17 bytes per input byte), MSZIP grows on demand.
 *
 * mspack_szddd_prefetch / mspack_kwajd_prefetch (mspack.h): the coded streams of MANY open headers in ONE batch -- an installation
 * medium is thousands of such files, and one batch of one unit each was a launch, an arena and a copy back per file.  A member's
 * room is the length its header states (when it lies within the largest possible expansion); its decoded bytes stay with the header
 * (struct sk_kept) until the extract() that writes them, or close().  A member that did not fit its room is decoded again, alone
 * and with the largest room, by its extract() -- what every extract() without prefetch does.
 */
#include <stdlib.h>
#include <stdio.h>
#include "host_common.h"

#define SZDD_INPUT 2048
#define KWAJ_INPUT 2048

/* (a provider of the batch ABI that has not learnt of MSPACK_HIP_UF_LZSS_RING -- the tests' CPU stand-in -- is asked for nothing new:
 * the capability call is a weak reference, as in oabd.c) */
extern unsigned mspack_hip_features(void) __attribute__((weak));

/* what a prefetch batch left with a header: its decoded bytes, inside the batch's output arena (shared, counted) */
struct sk_batch { unsigned char *out; size_t refs; };
enum { SK_NONE = 0, SK_HELD = 1, SK_REFIT = 2, SK_PENDING = 3 };
struct sk_kept {
  int state;                            /* SK_HELD: data / len / err are the unit's; SK_REFIT: it did not fit its room -- extract() decodes it alone */
  int err;
  const unsigned char *data;
  size_t len, room;
  struct sk_batch *batch;
};
struct szdd_hdr_p { struct msszddd_header base; struct mspack_file *fh; struct sk_kept kept; void *owner; };
struct kwaj_hdr_p { struct mskwajd_header base; struct mspack_file *fh; struct sk_kept kept; void *owner; };
struct szdd_p { struct msszdd_decompressor base; struct mspack_system *system; int error; size_t kept_bytes; };
struct kwaj_p { struct mskwaj_decompressor base; struct mspack_system *system; int error; size_t kept_bytes; };

/* mspack_szddd_batch_counts / mspack_kwajd_batch_counts (mspack.h): batches issued, extract() calls answered from a prefetch batch,
 * members decoded again alone; and the LZSS members of both drivers' prefetch batches that went out with MSPACK_HIP_UF_LZSS_RING */
static unsigned long long g_szdd_counts[3], g_kwaj_counts[3], g_ring_units;
static void count_add(unsigned long long *c, unsigned long long n) { __atomic_fetch_add(c, n, __ATOMIC_RELAXED); }
static void counts_read(unsigned long long *g, unsigned long long *c, int n, int reset)
{
  int i;
  for (i = 0; i < n; i++) {
    if (c) c[i] = __atomic_load_n(&g[i], __ATOMIC_RELAXED);
    if (reset) __atomic_store_n(&g[i], 0ull, __ATOMIC_RELAXED);
  }
}
void mspack_szddd_batch_counts(unsigned long long c[3], int reset) { counts_read(g_szdd_counts, c, 3, reset); }
void mspack_kwajd_batch_counts(unsigned long long c[3], int reset) { counts_read(g_kwaj_counts, c, 3, reset); }
unsigned long long mspack_szdd_kwaj_ring_units(int reset) { unsigned long long v; counts_read(&g_ring_units, &v, 1, reset); return v; }

/* read everything from the current position to the end of the file; -1 = read error */
static long slurp(struct mspack_system *sys, struct mspack_file *fh, unsigned char **data)
{
  size_t cap = 65536, n = 0;
  unsigned char *buf = (unsigned char *) sys->alloc(sys, cap + 64);
  if (!buf) return -2;
  for (;;) {
    int r;
    if (n + 32768 > cap) {
      unsigned char *nb = (unsigned char *) sys->alloc(sys, cap * 2 + 64);
      if (!nb) { sys->free(buf); return -2; }
      sys->copy(buf, nb, n); sys->free(buf); buf = nb; cap *= 2;
    }
    r = sys->read(fh, buf + n, 32768);
    if (r < 0) { sys->free(buf); return -1; }
    if (r == 0) break;
    n += (size_t) r;
  }
  memset(buf + n, 0, 64);
  *data = buf;
  return (long) n;
}

/* decode ONE coded stream on the GPU and write what it produced */
static int run_unit(struct mspack_system *sys, struct mspack_file *outfh, const unsigned char *in, size_t in_len,
                    int kind, int mode, unsigned int unit_flags, size_t room, unsigned long long *counts)
{
  for (;;) {
    mspack_hip_unit u;
    mspack_hip_result r;
    unsigned char *out;
    const size_t below = (kind == MSPACK_HIP_KIND_MSZIP) ? 0 : 4096, slack = (kind == MSPACK_HIP_KIND_MSZIP) ? 32768 : 0;
    int rc, err;
    if (room > 0xFFFF0000u - 65536u) return MSPACK_ERR_NOMEMORY;
    if (!(out = (unsigned char *) sys->alloc(sys, below + room + slack + 64))) return MSPACK_ERR_NOMEMORY;
    memset(&u, 0, sizeof(u)); memset(&r, 0, sizeof(r));
    u.in_off = 0; u.in_len = (uint32_t) in_len;
    u.out_off = below; u.out_len = (uint32_t) room;
    u.kind = (uint8_t) kind; u.window_bits = (uint8_t) mode; u.flags = unit_flags;
    rc = mspack_hip_decode_batch(&u, 1, in, in_len + 48, out, below + room + slack + 64, &r);
    count_add(&counts[0], 1);
    if (rc) {
      sys->message(NULL, "GPU batch decode failed: %s", mspack_hip_last_error());
      sys->free(out);
      return MSPACK_ERR_DECRUNCH;
    }
    if (r.flags & MSPACK_HIP_F_OUT_FULL) { sys->free(out); room *= 4; continue; }     /* MSZIP: more room */
    err = r.err;
    if (write_slice(sys, outfh, out + below, r.out_len > room ? room : r.out_len) && !err) err = MSPACK_ERR_WRITE;
    sys->free(out);
    return err;
  }
}

/* ---- prefetch: many streams, one batch ---------------------------------------------------------------- */
/* the largest possible expansion of n coded bytes: what a solitary extract() gives its unit */
static size_t worst_room(int kind, size_t n)
{
  if (kind == MSPACK_HIP_KIND_LZSS) return n * 9 + 64;
  if (kind == MSPACK_HIP_KIND_KWAJ_LZH) return n * 18 + 4096;
  return (n * 8 + 65536 + 32767) & ~(size_t) 32767;
}
struct sk_item {                        /* one member to be */
  struct sk_kept *kept;
  struct mspack_file *fh;
  off_t data_off, stated;               /* where its coded bytes begin; the length its header states (0: none) */
  int kind, mode, ok;
  unsigned int flags;
  size_t in_len, room, below, slack, in_off, out_off;
};
static void sk_release(struct mspack_system *sys, struct sk_kept *k, size_t *kept_bytes)
{
  if (k->state == SK_HELD) {
    *kept_bytes -= k->room;
    if (--k->batch->refs == 0) { mspack_arena_free(sys, k->batch->out); sys->free(k->batch); }
  }
  memset(k, 0, sizeof(*k));
}
/* extract() of a held member: what run_unit does with its unit's result */
static int sk_emit(struct mspack_system *sys, struct mspack_file *outfh, const struct sk_kept *k)
{
  int err = k->err;
  if (write_slice(sys, outfh, k->data, k->len) && !err) err = MSPACK_ERR_WRITE;
  return err;
}
/* it[0 .. n): read, decode in ONE batch, keep.  MSPACK_ERR_OK / _NOMEMORY / _DECRUNCH */
static int sk_prefetch(struct mspack_system *sys, struct sk_item *it, int n, size_t *kept_bytes, unsigned long long *counts)
{
  const int ring = mspack_hip_features && (mspack_hip_features() & MSPACK_HIP_FEAT_LZSS_RING);
  const size_t budget = (size_t) mspack_hip_cache_mb() << 20;
  size_t in_total = 0, out_total = 0, kept_new = 0, nu = 0, n_ring = 0;
  unsigned char *in = NULL, *out = NULL;
  mspack_hip_unit *units = NULL;
  mspack_hip_result *res = NULL;
  struct sk_batch *B = NULL;
  int i, rc, err = MSPACK_ERR_OK;
  for (i = 0; i < n; i++) {
    struct sk_item *m = &it[i];
    off_t flen;
    size_t worst;
    m->ok = 0;
    if (mspack_sys_filelen(sys, m->fh, &flen) || flen < m->data_off || (uint64_t)(flen - m->data_off) > 0x0FFFFFFFu) continue;
    m->in_len = (size_t)(flen - m->data_off);
    worst = worst_room(m->kind, m->in_len);
    m->room = (m->stated > 0 && (uint64_t) m->stated <= (uint64_t) worst) ? (size_t) m->stated : worst;
    /* (KWAJ-framed MSZIP decodes a block only with 32 KiB of room left, mszip_kernel.hpp: its room counts in whole blocks, as worst_room does) */
    if (m->kind == MSPACK_HIP_KIND_MSZIP) m->room = (m->room + 32767) & ~(size_t) 32767;
    if (m->room > 0xFFFF0000u - 65536u) continue;
    m->flags = (m->kind == MSPACK_HIP_KIND_MSZIP) ? MSPACK_HIP_UF_MSZIP_KWAJ : (m->kind == MSPACK_HIP_KIND_LZSS && ring) ? MSPACK_HIP_UF_LZSS_RING : 0u;
    m->below = (m->kind == MSPACK_HIP_KIND_MSZIP || (m->flags & MSPACK_HIP_UF_LZSS_RING)) ? 0 : 4096;
    m->slack = (m->kind == MSPACK_HIP_KIND_MSZIP) ? 32768 : 0;
    if (*kept_bytes + kept_new + m->room > budget) continue;      /* beyond mspack_hip_cache_mb(): its extract() decodes it */
    kept_new += m->room;
    m->in_off = in_total; in_total += (m->in_len + 15) & ~(size_t) 15;
    m->out_off = out_total + m->below; out_total += (m->below + m->room + m->slack + 15) & ~(size_t) 15;
    m->ok = 1; nu++;
  }
  if (!nu) return MSPACK_ERR_OK;
  in = (unsigned char *) mspack_arena_alloc(sys, in_total + 64);
  out = (unsigned char *) mspack_arena_alloc(sys, out_total + 64);
  units = (mspack_hip_unit *) sys->alloc(sys, nu * sizeof(*units));
  res = (mspack_hip_result *) sys->alloc(sys, nu * sizeof(*res));
  B = (struct sk_batch *) sys->alloc(sys, sizeof(*B));
  if (!in || !out || !units || !res || !B) { err = MSPACK_ERR_NOMEMORY; goto done; }
  B->out = out; B->refs = 0;
  memset(units, 0, nu * sizeof(*units)); memset(res, 0, nu * sizeof(*res));
  nu = 0;
  for (i = 0; i < n; i++) {
    struct sk_item *m = &it[i];
    size_t got = 0;
    mspack_hip_unit *u;
    if (!m->ok) continue;
    m->ok = 0;
    if (sys->seek(m->fh, m->data_off, MSPACK_SYS_SEEK_START)) continue;       /* (its extract() reports that) */
    while (got < m->in_len) {
      const size_t want = m->in_len - got;
      const int r = sys->read(m->fh, in + m->in_off + got, want > 32768 ? 32768 : (int) want);
      if (r < 0) break;
      if (r == 0) { m->in_len = got; break; }
      got += (size_t) r;
    }
    if (got < m->in_len) continue;                                             /* a failed read: left out */
    u = &units[nu];
    u->in_off = m->in_off; u->in_len = (uint32_t) m->in_len; u->out_off = m->out_off; u->out_len = (uint32_t) m->room;
    u->kind = (uint8_t) m->kind; u->window_bits = (uint8_t) m->mode; u->flags = m->flags;
    if (m->flags & MSPACK_HIP_UF_LZSS_RING) n_ring++;
    m->ok = 1; nu++;
  }
  if (!nu) goto done;
  rc = mspack_hip_decode_batch(units, nu, in, in_total + 48, out, out_total + 64, res);
  count_add(&counts[0], 1);
  if (rc) {
    sys->message(NULL, "GPU batch decode failed: %s", mspack_hip_last_error());
    err = MSPACK_ERR_DECRUNCH;
    goto done;
  }
  count_add(&g_ring_units, n_ring);
  nu = 0;
  for (i = 0; i < n; i++) {
    struct sk_item *m = &it[i];
    const mspack_hip_result *r;
    if (!m->ok) continue;
    r = &res[nu++];
    if (r->out_len > m->room || (r->flags & MSPACK_HIP_F_OUT_FULL)) { m->kept->state = SK_REFIT; continue; }
    m->kept->state = SK_HELD; m->kept->err = r->err; m->kept->data = out + m->out_off; m->kept->len = r->out_len;
    m->kept->room = m->room; m->kept->batch = B;
    B->refs++; *kept_bytes += m->room;
  }
done:
  for (i = 0; i < n; i++) if (it[i].kept->state == SK_PENDING) it[i].kept->state = SK_NONE;
  if (!B || B->refs == 0) { mspack_arena_free(sys, out); sys->free(B); }
  mspack_arena_free(sys, in); sys->free(units); sys->free(res);
  return err;
}

/* ---- SZDD --------------------------------------------------------------------------------------------- */
static const unsigned char sig_expand[8] = { 0x53, 0x5A, 0x44, 0x44, 0x88, 0xF0, 0x27, 0x33 };
static const unsigned char sig_qbasic[8] = { 0x53, 0x5A, 0x20, 0x88, 0xF0, 0x27, 0x33, 0xD1 };

static int szdd_headers(struct mspack_system *sys, struct mspack_file *fh, struct msszddd_header *hdr)
{
  unsigned char buf[8];
  if (sys->read(fh, buf, 8) != 8) return MSPACK_ERR_READ;
  if (!memcmp(buf, sig_expand, 8)) {
    hdr->format = MSSZDD_FMT_NORMAL;
    if (sys->read(fh, buf, 6) != 6) return MSPACK_ERR_READ;
    if (buf[0] != 0x41) return MSPACK_ERR_DATAFORMAT;
    hdr->missing_char = (char) buf[1];
    hdr->length = (off_t) rd_le32(buf + 2);
  }
  else if (!memcmp(buf, sig_qbasic, 8)) {
    hdr->format = MSSZDD_FMT_QBASIC;
    if (sys->read(fh, buf, 4) != 4) return MSPACK_ERR_READ;
    hdr->missing_char = '\0';
    hdr->length = (off_t) rd_le32(buf);
  }
  else return MSPACK_ERR_SIGNATURE;
  return MSPACK_ERR_OK;
}

static struct msszddd_header *szdd_open(struct msszdd_decompressor *base, const char *filename)
{
  struct szdd_p *self = (struct szdd_p *) base;
  struct mspack_system *sys;
  struct szdd_hdr_p *hdr;
  struct mspack_file *fh;
  if (!self) return NULL;
  sys = self->system;
  fh = sys->open(sys, filename, MSPACK_SYS_OPEN_READ);
  hdr = (struct szdd_hdr_p *) sys->alloc(sys, sizeof(*hdr));
  if (fh && hdr) { hdr->fh = fh; memset(&hdr->kept, 0, sizeof(hdr->kept)); hdr->owner = self; self->error = szdd_headers(sys, fh, &hdr->base); }
  else { if (!fh) self->error = MSPACK_ERR_OPEN; if (!hdr) self->error = MSPACK_ERR_NOMEMORY; }
  if (self->error) { if (fh) sys->close(fh); sys->free(hdr); hdr = NULL; }
  return (struct msszddd_header *) hdr;
}

static void szdd_close(struct msszdd_decompressor *base, struct msszddd_header *hdr)
{
  struct szdd_p *self = (struct szdd_p *) base;
  if (!self || !self->system || !hdr) return;
  sk_release(self->system, &((struct szdd_hdr_p *) hdr)->kept, &self->kept_bytes);
  self->system->close(((struct szdd_hdr_p *) hdr)->fh);
  self->system->free(hdr);
  self->error = MSPACK_ERR_OK;
}

static int szdd_extract(struct msszdd_decompressor *base, struct msszddd_header *hdr, const char *filename)
{
  struct szdd_p *self = (struct szdd_p *) base;
  struct mspack_system *sys;
  struct mspack_file *fh, *outfh;
  unsigned char *data = NULL;
  long n;
  if (!self) return MSPACK_ERR_ARGS;
  if (!hdr) return self->error = MSPACK_ERR_ARGS;
  sys = self->system;
  fh = ((struct szdd_hdr_p *) hdr)->fh;
  if (sys->seek(fh, (off_t)(hdr->format == MSSZDD_FMT_NORMAL ? 14 : 12), MSPACK_SYS_SEEK_START)) return self->error = MSPACK_ERR_SEEK;
  if (!(outfh = sys->open(sys, filename, MSPACK_SYS_OPEN_WRITE))) return self->error = MSPACK_ERR_OPEN;
  {
    struct sk_kept *k = &((struct szdd_hdr_p *) hdr)->kept;
    if (k->state == SK_HELD) {                            /* a prefetch batch decoded it */
      self->error = sk_emit(sys, outfh, k);
      sk_release(sys, k, &self->kept_bytes);
      count_add(&g_szdd_counts[1], 1);
      sys->close(outfh);
      return self->error;
    }
    if (k->state == SK_REFIT) { k->state = SK_NONE; count_add(&g_szdd_counts[2], 1); }
  }
  n = slurp(sys, fh, &data);
  if (n == -2) self->error = MSPACK_ERR_NOMEMORY;
  else if (n == -1) self->error = MSPACK_ERR_READ;        /* (the reference fails at the first bad read) */
  else {
    self->error = run_unit(sys, outfh, data, (size_t) n, MSPACK_HIP_KIND_LZSS,
                           hdr->format == MSSZDD_FMT_NORMAL ? 0 : 2, 0, (size_t) n * 9 + 64, g_szdd_counts);
    sys->free(data);
  }
  sys->close(outfh);
  return self->error;
}

static int szdd_decompress(struct msszdd_decompressor *base, const char *input, const char *output)
{
  struct szdd_p *self = (struct szdd_p *) base;
  struct msszddd_header *hdr;
  int error;
  if (!self) return MSPACK_ERR_ARGS;
  if (!(hdr = szdd_open(base, input))) return self->error;
  error = szdd_extract(base, hdr, output);
  szdd_close(base, hdr);
  return self->error = error;
}

static int szdd_error(struct msszdd_decompressor *base) {
  struct szdd_p *self = (struct szdd_p *) base;
  return self ? self->error : MSPACK_ERR_ARGS;
}

struct msszdd_decompressor *mspack_create_szdd_decompressor(struct mspack_system *sys)
{
  struct szdd_p *self;
  if (!sys) sys = mspack_default_system;
  if (!mspack_valid_system(sys)) return NULL;
  if (!(self = (struct szdd_p *) sys->alloc(sys, sizeof(*self)))) return NULL;
  self->base.open = &szdd_open; self->base.close = &szdd_close; self->base.extract = &szdd_extract;
  self->base.decompress = &szdd_decompress; self->base.last_error = &szdd_error;
  self->system = sys; self->error = MSPACK_ERR_OK; self->kept_bytes = 0;
  return &self->base;
}
int mspack_szddd_prefetch(struct msszdd_decompressor *base, struct msszddd_header **hdrs, int n)
{
  struct szdd_p *self = (struct szdd_p *) base;
  struct mspack_system *sys;
  struct sk_item *it;
  int i, ni = 0;
  if (!self) return MSPACK_ERR_ARGS;
  if (!hdrs || n <= 0) return self->error = MSPACK_ERR_ARGS;
  sys = self->system;
  if (!(it = (struct sk_item *) sys->alloc(sys, (size_t) n * sizeof(*it)))) return self->error = MSPACK_ERR_NOMEMORY;
  for (i = 0; i < n; i++) {
    struct szdd_hdr_p *h = (struct szdd_hdr_p *) hdrs[i];
    if (!h || h->owner != (void *) self || h->kept.state != SK_NONE) continue;      /* NULL, another decompressor's, held (or known not to fit), given twice */
    memset(&it[ni], 0, sizeof(it[ni]));
    it[ni].kept = &h->kept; it[ni].fh = h->fh; it[ni].stated = h->base.length;
    it[ni].data_off = (off_t)(h->base.format == MSSZDD_FMT_NORMAL ? 14 : 12);
    it[ni].kind = MSPACK_HIP_KIND_LZSS; it[ni].mode = h->base.format == MSSZDD_FMT_NORMAL ? 0 : 2;
    h->kept.state = SK_PENDING;
    ni++;
  }
  self->error = ni ? sk_prefetch(sys, it, ni, &self->kept_bytes, g_szdd_counts) : MSPACK_ERR_OK;
  sys->free(it);
  return self->error;
}
void mspack_destroy_szdd_decompressor(struct msszdd_decompressor *base) {
  struct szdd_p *self = (struct szdd_p *) base;
  if (self) self->system->free(self);
}

/* ---- KWAJ --------------------------------------------------------------------------------------------- */
/* one 8.3 name part: up to `max` bytes of a NUL-terminated string (kwajd.c:212-238) */
static int kwaj_name_part(struct mspack_system *sys, struct mspack_file *fh, char **fn, int max)
{
  unsigned char buf[16];
  int len, i;
  if ((len = sys->read(fh, buf, max)) < 2) return MSPACK_ERR_READ;
  for (i = 0; i < len; i++) if (!(*(*fn)++ = (char) buf[i])) break;
  if (i == max && buf[max - 1] != '\0') return MSPACK_ERR_DATAFORMAT;
  if (sys->seek(fh, (off_t)(i + 1 - len), MSPACK_SYS_SEEK_CUR)) return MSPACK_ERR_SEEK;
  (*fn)--;                                              /* drop the terminator */
  return MSPACK_ERR_OK;
}

static int kwaj_headers(struct mspack_system *sys, struct mspack_file *fh, struct mskwajd_header *hdr)
{
  unsigned char buf[16];
  int i, err;
  hdr->filename = NULL; hdr->extra = NULL;
  if (sys->read(fh, buf, 14) != 14) return MSPACK_ERR_READ;
  if (rd_le32(buf) != 0x4A41574Bu || rd_le32(buf + 4) != 0xD127F088u) return MSPACK_ERR_SIGNATURE;
  hdr->comp_type = (unsigned short) rd_le16(buf + 8);
  hdr->data_offset = (off_t) rd_le16(buf + 10);
  hdr->headers = (int) rd_le16(buf + 12);
  hdr->length = 0; hdr->extra_length = 0;
  if (hdr->headers & MSKWAJ_HDR_HASLENGTH) {
    if (sys->read(fh, buf, 4) != 4) return MSPACK_ERR_READ;
    hdr->length = (off_t) rd_le32(buf);
  }
  if (hdr->headers & MSKWAJ_HDR_HASUNKNOWN1) { if (sys->read(fh, buf, 2) != 2) return MSPACK_ERR_READ; }
  if (hdr->headers & MSKWAJ_HDR_HASUNKNOWN2) {
    if (sys->read(fh, buf, 2) != 2) return MSPACK_ERR_READ;
    i = (int) rd_le16(buf);
    if (sys->seek(fh, (off_t) i, MSPACK_SYS_SEEK_CUR)) return MSPACK_ERR_SEEK;
  }
  if (hdr->headers & (MSKWAJ_HDR_HASFILENAME | MSKWAJ_HDR_HASFILEEXT)) {
    char *fn = (char *) sys->alloc(sys, 13);
    if (!(hdr->filename = fn)) return MSPACK_ERR_NOMEMORY;
    if (hdr->headers & MSKWAJ_HDR_HASFILENAME) { if ((err = kwaj_name_part(sys, fh, &fn, 9))) return err; }
    if (hdr->headers & MSKWAJ_HDR_HASFILEEXT) {
      *fn++ = '.';
      if ((err = kwaj_name_part(sys, fh, &fn, 4))) return err;
    }
    *fn = '\0';
  }
  if (hdr->headers & MSKWAJ_HDR_HASEXTRATEXT) {
    if (sys->read(fh, buf, 2) != 2) return MSPACK_ERR_READ;
    i = (int) rd_le16(buf);
    if (!(hdr->extra = (char *) sys->alloc(sys, (size_t) i + 1))) return MSPACK_ERR_NOMEMORY;
    if (sys->read(fh, hdr->extra, i) != i) return MSPACK_ERR_READ;
    hdr->extra[i] = '\0';
    hdr->extra_length = (unsigned short) i;
  }
  return MSPACK_ERR_OK;
}

static void kwaj_close(struct mskwaj_decompressor *base, struct mskwajd_header *hdr)
{
  struct kwaj_p *self = (struct kwaj_p *) base;
  if (!self || !self->system || !hdr) return;
  sk_release(self->system, &((struct kwaj_hdr_p *) hdr)->kept, &self->kept_bytes);
  self->system->close(((struct kwaj_hdr_p *) hdr)->fh);
  self->system->free(hdr->filename); self->system->free(hdr->extra);
  self->system->free(hdr);
  self->error = MSPACK_ERR_OK;
}

static struct mskwajd_header *kwaj_open(struct mskwaj_decompressor *base, const char *filename)
{
  struct kwaj_p *self = (struct kwaj_p *) base;
  struct mspack_system *sys;
  struct kwaj_hdr_p *hdr;
  struct mspack_file *fh;
  if (!self) return NULL;
  sys = self->system;
  /* like kwajd_open (kwajd.c:95-123): no file, no header object */
  if (!(fh = sys->open(sys, filename, MSPACK_SYS_OPEN_READ))) { self->error = MSPACK_ERR_OPEN; return NULL; }
  hdr = (struct kwaj_hdr_p *) sys->alloc(sys, sizeof(*hdr));
  if (hdr) {
    memset(hdr, 0, sizeof(*hdr));                 /* filename / extra are freed on every error path */
    hdr->fh = fh; hdr->owner = self; self->error = kwaj_headers(sys, fh, &hdr->base);
  }
  else self->error = MSPACK_ERR_NOMEMORY;
  if (self->error) {
    if (fh) sys->close(fh);
    if (hdr) { sys->free(hdr->base.filename); sys->free(hdr->base.extra); }
    sys->free(hdr);
    hdr = NULL;
  }
  return (struct mskwajd_header *) hdr;
}

static int kwaj_extract(struct mskwaj_decompressor *base, struct mskwajd_header *hdr, const char *filename)
{
  struct kwaj_p *self = (struct kwaj_p *) base;
  struct mspack_system *sys;
  struct mspack_file *fh, *outfh;
  if (!self) return MSPACK_ERR_ARGS;
  if (!hdr) return self->error = MSPACK_ERR_ARGS;
  sys = self->system;
  fh = ((struct kwaj_hdr_p *) hdr)->fh;
  if (sys->seek(fh, hdr->data_offset, MSPACK_SYS_SEEK_START)) return self->error = MSPACK_ERR_SEEK;
  if (!(outfh = sys->open(sys, filename, MSPACK_SYS_OPEN_WRITE))) return self->error = MSPACK_ERR_OPEN;
  self->error = MSPACK_ERR_OK;
  if (hdr->comp_type == MSKWAJ_COMP_NONE || hdr->comp_type == MSKWAJ_COMP_XOR) {
    unsigned char *buf = (unsigned char *) sys->alloc(sys, KWAJ_INPUT);
    if (buf) {
      int rd, i;
      while ((rd = sys->read(fh, buf, KWAJ_INPUT)) > 0) {
        if (hdr->comp_type == MSKWAJ_COMP_XOR) for (i = 0; i < rd; i++) buf[i] ^= 0xFF;
        if (sys->write(outfh, buf, rd) != rd) { self->error = MSPACK_ERR_WRITE; break; }
      }
      if (rd < 0) self->error = MSPACK_ERR_READ;
      sys->free(buf);
    }
    else self->error = MSPACK_ERR_NOMEMORY;
  }
  else if (((struct kwaj_hdr_p *) hdr)->kept.state == SK_HELD) {          /* a prefetch batch decoded it */
    struct sk_kept *k = &((struct kwaj_hdr_p *) hdr)->kept;
    self->error = sk_emit(sys, outfh, k);
    sk_release(sys, k, &self->kept_bytes);
    count_add(&g_kwaj_counts[1], 1);
  }
  else if (hdr->comp_type == MSKWAJ_COMP_SZDD || hdr->comp_type == MSKWAJ_COMP_LZH || hdr->comp_type == MSKWAJ_COMP_MSZIP) {
    unsigned char *data = NULL;
    long n;
    struct sk_kept *k = &((struct kwaj_hdr_p *) hdr)->kept;
    if (k->state == SK_REFIT) { k->state = SK_NONE; count_add(&g_kwaj_counts[2], 1); }
    n = slurp(sys, fh, &data);
    if (n == -2) self->error = MSPACK_ERR_NOMEMORY;
    else if (n == -1) self->error = MSPACK_ERR_READ;
    else {
      if (hdr->comp_type == MSKWAJ_COMP_SZDD)
        self->error = run_unit(sys, outfh, data, (size_t) n, MSPACK_HIP_KIND_LZSS, 2, 0, (size_t) n * 9 + 64, g_kwaj_counts);
      else if (hdr->comp_type == MSKWAJ_COMP_LZH)
        self->error = run_unit(sys, outfh, data, (size_t) n, MSPACK_HIP_KIND_KWAJ_LZH, 0, 0, (size_t) n * 18 + 4096, g_kwaj_counts);
      else
        self->error = run_unit(sys, outfh, data, (size_t) n, MSPACK_HIP_KIND_MSZIP, 0, MSPACK_HIP_UF_MSZIP_KWAJ,
                               ((size_t) n * 8 + 65536 + 32767) & ~(size_t) 32767, g_kwaj_counts);
      sys->free(data);
    }
  }
  else self->error = MSPACK_ERR_DATAFORMAT;
  sys->close(outfh);
  return self->error;
}

static int kwaj_decompress(struct mskwaj_decompressor *base, const char *input, const char *output)
{
  struct kwaj_p *self = (struct kwaj_p *) base;
  struct mskwajd_header *hdr;
  int error;
  if (!self) return MSPACK_ERR_ARGS;
  if (!(hdr = kwaj_open(base, input))) return self->error;
  error = kwaj_extract(base, hdr, output);
  kwaj_close(base, hdr);
  return self->error = error;
}

static int kwaj_error(struct mskwaj_decompressor *base) {
  struct kwaj_p *self = (struct kwaj_p *) base;
  return self ? self->error : MSPACK_ERR_ARGS;
}

struct mskwaj_decompressor *mspack_create_kwaj_decompressor(struct mspack_system *sys)
{
  struct kwaj_p *self;
  if (!sys) sys = mspack_default_system;
  if (!mspack_valid_system(sys)) return NULL;
  if (!(self = (struct kwaj_p *) sys->alloc(sys, sizeof(*self)))) return NULL;
  self->base.open = &kwaj_open; self->base.close = &kwaj_close; self->base.extract = &kwaj_extract;
  self->base.decompress = &kwaj_decompress; self->base.last_error = &kwaj_error;
  self->system = sys; self->error = MSPACK_ERR_OK; self->kept_bytes = 0;
  return &self->base;
}
int mspack_kwajd_prefetch(struct mskwaj_decompressor *base, struct mskwajd_header **hdrs, int n)
{
  struct kwaj_p *self = (struct kwaj_p *) base;
  struct mspack_system *sys;
  struct sk_item *it;
  int i, ni = 0;
  if (!self) return MSPACK_ERR_ARGS;
  if (!hdrs || n <= 0) return self->error = MSPACK_ERR_ARGS;
  sys = self->system;
  if (!(it = (struct sk_item *) sys->alloc(sys, (size_t) n * sizeof(*it)))) return self->error = MSPACK_ERR_NOMEMORY;
  for (i = 0; i < n; i++) {
    struct kwaj_hdr_p *h = (struct kwaj_hdr_p *) hdrs[i];
    const int ct = h ? h->base.comp_type : -1;
    if (!h || h->owner != (void *) self || h->kept.state != SK_NONE) continue;
    if (ct != MSKWAJ_COMP_SZDD && ct != MSKWAJ_COMP_LZH && ct != MSKWAJ_COMP_MSZIP) continue;      /* stored and unknown methods: extract() as ever */
    memset(&it[ni], 0, sizeof(it[ni]));
    it[ni].kept = &h->kept; it[ni].fh = h->fh; it[ni].data_off = h->base.data_offset;
    it[ni].stated = (h->base.headers & MSKWAJ_HDR_HASLENGTH) ? h->base.length : 0;
    it[ni].kind = ct == MSKWAJ_COMP_SZDD ? MSPACK_HIP_KIND_LZSS : ct == MSKWAJ_COMP_LZH ? MSPACK_HIP_KIND_KWAJ_LZH : MSPACK_HIP_KIND_MSZIP;
    it[ni].mode = ct == MSKWAJ_COMP_SZDD ? 2 : 0;
    h->kept.state = SK_PENDING;
    ni++;
  }
  self->error = ni ? sk_prefetch(sys, it, ni, &self->kept_bytes, g_kwaj_counts) : MSPACK_ERR_OK;
  sys->free(it);
  return self->error;
}
void mspack_destroy_kwaj_decompressor(struct mskwaj_decompressor *base) {
  struct kwaj_p *self = (struct kwaj_p *) base;
  if (self) self->system->free(self);
}
