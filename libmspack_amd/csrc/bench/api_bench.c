/* api_bench.c -- BENCH / TEST INFRASTRUCTURE (not the decode product): times the library through the API the north star
 * names -- mspack_create_cab_decompressor() / mspack_create_chm_decompressor() -> open() -> extract() of every file
 * (reference cabd.c:1075-1214, chmd.c:906-1041) -- with an in-memory mspack_system written in C, the way the reference's
 * own test/cabd_memory.c and test/cabd_md5.c:145 drive it.  No Python on the timed path: bench.py and the parity tests
 * hand over a container image and get the extracted bytes and the time split back.
 *
 * The mspack_system here: "in" is the container image (read-only), every other name opened for writing appends to the
 * caller's output buffer (files land one behind the other in extraction order), messages are counted.  Time spent inside
 * read / seek / write callbacks is accumulated, so that the harness can split a run into the driver's reads (gather),
 * the library's own phases (mspack_hip_host_path_stats: plan, H2D + launches, wait + D2H) and sys->write.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <time.h>
#include "../../../include/mspack.h"
#include "../../../include/mspack_hip.h"

typedef struct mspk_api_stats {
  double total_s;            /* create + open + every extract + close + destroy */
  double open_s;             /* open(): headers, file list (CHM: directory chunks) */
  double first_extract_s;    /* the first extract(): it gathers and decodes the batch */
  double read_s, write_s;    /* inside sys->read / seek, inside sys->write */
  double lib_plan_ms, lib_issue_ms, lib_drain_ms;   /* the host-buffer entry points' own phases, summed over their calls */
  unsigned long long bytes_out, bytes_read;
  unsigned int n_files, n_errors, n_messages, lib_calls;
  int first_error;
} mspk_api_stats;

struct mem_sys {
  struct mspack_system sys;
  const unsigned char *image; size_t image_len;
  /* (mspk_api_bench_cabs: many images, back to back in `image`; image k is image[many_offs[k] .. many_offs[k + 1]), its name "c<k>") */
  const unsigned long long *many_offs; unsigned int n_many;
  unsigned char *out; size_t out_cap, out_len;
  double read_s, write_s;
  unsigned long long bytes_read;
  unsigned int n_messages;
};
struct mem_file { struct mem_sys *ms; int writing; size_t pos; const unsigned char *img; size_t img_len; };

static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double) ts.tv_sec + 1e-9 * (double) ts.tv_nsec; }

static struct mspack_file *ms_open(struct mspack_system *self, const char *filename, int mode)
{
  struct mem_sys *ms = (struct mem_sys *) self;
  struct mem_file *f;
  const int writing = mode == MSPACK_SYS_OPEN_WRITE || mode == MSPACK_SYS_OPEN_APPEND || mode == MSPACK_SYS_OPEN_UPDATE;
  const unsigned char *img = ms->image; size_t img_len = ms->image_len;
  if (!writing && ms->many_offs && filename[0] == 'c') {
    const unsigned long k = strtoul(filename + 1, NULL, 10);
    if (k >= ms->n_many) return NULL;
    img = ms->image + ms->many_offs[k]; img_len = (size_t)(ms->many_offs[k + 1] - ms->many_offs[k]);
  }
  else if (!writing && strcmp(filename, "in") != 0) return NULL;
  if (!(f = (struct mem_file *) malloc(sizeof(*f)))) return NULL;
  f->ms = ms; f->writing = writing; f->pos = 0; f->img = img; f->img_len = img_len;
  return (struct mspack_file *) f;
}
static void ms_close(struct mspack_file *file) { free(file); }
static int ms_read(struct mspack_file *file, void *buffer, int bytes)
{
  struct mem_file *f = (struct mem_file *) file;
  struct mem_sys *ms = f->ms;
  const double t0 = now_s();
  size_t n;
  if (f->writing || bytes < 0) return -1;
  n = f->img_len - f->pos;
  if (n > (size_t) bytes) n = (size_t) bytes;
  memcpy(buffer, f->img + f->pos, n);
  f->pos += n; ms->bytes_read += n;
  ms->read_s += now_s() - t0;
  return (int) n;
}
static int ms_write(struct mspack_file *file, void *buffer, int bytes)
{
  struct mem_file *f = (struct mem_file *) file;
  struct mem_sys *ms = f->ms;
  const double t0 = now_s();
  if (!f->writing || bytes < 0) return -1;
  if (ms->out_len + (size_t) bytes > ms->out_cap) return -1;
  memcpy(ms->out + ms->out_len, buffer, (size_t) bytes);
  ms->out_len += (size_t) bytes;
  ms->write_s += now_s() - t0;
  return bytes;
}
static int ms_seek(struct mspack_file *file, off_t offset, int mode)
{
  struct mem_file *f = (struct mem_file *) file;
  off_t base = mode == MSPACK_SYS_SEEK_START ? 0 : (mode == MSPACK_SYS_SEEK_CUR ? (off_t) f->pos : (off_t) f->img_len);
  if (f->writing) return -1;
  if (base + offset < 0 || (size_t)(base + offset) > f->img_len) return -1;
  f->pos = (size_t)(base + offset);
  return 0;
}
static off_t ms_tell(struct mspack_file *file) { return (off_t)((struct mem_file *) file)->pos; }
/* messages: counted; formatted and kept (one line each) when the run asked for the log.  `file` may be NULL, so the
 * system is found through the one instance a run uses (the harness is single-threaded). */
static struct mem_sys *g_cur;
static char *g_log; static size_t g_log_cap, g_log_len;
static void log_line(const char *line)
{
  size_t n = strlen(line);
  if (!g_log || g_log_len + n + 2 > g_log_cap) return;
  memcpy(g_log + g_log_len, line, n); g_log_len += n;
  g_log[g_log_len++] = '\n'; g_log[g_log_len] = 0;
}
static void ms_message(struct mspack_file *file, const char *format, ...)
{
  char line[512];
  va_list ap;
  (void) file;
  if (g_cur) g_cur->n_messages++;
  if (!g_log) return;
  va_start(ap, format);
  vsnprintf(line, sizeof(line), format, ap);
  va_end(ap);
  log_line(line);
}
/* (alloc / free / copy: the library's own defaults, as in api.MemSystem -- an in-memory FILE layer, not an allocator.  With its
 *  default allocator the library may take its big staging arenas from page-locked memory it keeps, mspack_hip.h) */
extern struct mspack_system *mspack_default_system;

static void mem_sys_init(struct mem_sys *ms, const unsigned char *image, size_t image_len, unsigned char *out, size_t out_cap)
{
  memset(ms, 0, sizeof(*ms));
  ms->sys.open = ms_open; ms->sys.close = ms_close; ms->sys.read = ms_read; ms->sys.write = ms_write;
  ms->sys.seek = ms_seek; ms->sys.tell = ms_tell; ms->sys.message = ms_message;
  ms->sys.alloc = mspack_default_system->alloc; ms->sys.free = mspack_default_system->free; ms->sys.copy = mspack_default_system->copy;
  ms->sys.null_ptr = NULL;
  ms->image = image; ms->image_len = image_len; ms->out = out; ms->out_cap = out_cap;
  g_cur = ms;
}

static void finish(struct mem_sys *ms, mspk_api_stats *st, double t_start)
{
  double ph[4] = { 0, 0, 0, 0 };
  st->total_s = now_s() - t_start;
  st->read_s = ms->read_s; st->write_s = ms->write_s;
  st->bytes_out = ms->out_len; st->bytes_read = ms->bytes_read; st->n_messages = ms->n_messages;
  mspack_hip_host_path_stats(ph, 0);
  st->lib_plan_ms = ph[0]; st->lib_issue_ms = ph[1]; st->lib_drain_ms = ph[2]; st->lib_calls = (unsigned int) ph[3];
}

/* one cabinet image: open, extract every file in list order (the first extract() decodes every folder in one batch).
 * offsets (optional, n_files + 1 entries): where each file's bytes start in `out`. */
int mspk_api_bench_cab(const unsigned char *cab, size_t cab_len, unsigned char *out, size_t out_cap,
                       unsigned long long *offsets, unsigned int max_files, mspk_api_stats *st)
{
  struct mem_sys ms;
  struct mscab_decompressor *d;
  struct mscabd_cabinet *c;
  struct mscabd_file *f;
  double t0, t1;
  memset(st, 0, sizeof(*st));
  mem_sys_init(&ms, cab, cab_len, out, out_cap);
  mspack_hip_host_path_stats(NULL, 1);
  t0 = now_s();
  if (!(d = mspack_create_cab_decompressor(&ms.sys))) return -1;
  t1 = now_s();
  c = d->open(d, "in");
  st->open_s = now_s() - t1;
  if (!c) { st->first_error = d->last_error(d); mspack_destroy_cab_decompressor(d); return -2; }
  for (f = c->files; f; f = f->next) {
    const double e0 = now_s();
    int err;
    if (offsets && st->n_files < max_files) offsets[st->n_files] = ms.out_len;
    err = d->extract(d, f, "out");
    if (st->n_files == 0) st->first_extract_s = now_s() - e0;
    if (err) { if (!st->n_errors) st->first_error = err; st->n_errors++; }
    st->n_files++;
  }
  if (offsets && st->n_files < max_files) offsets[st->n_files] = ms.out_len;
  d->close(d, c);
  mspack_destroy_cab_decompressor(d);
  finish(&ms, st, t0);
  return 0;
}

/* MANY cabinet images on ONE decompressor -- the directory of small cabinets: open them all, then extract every file, cabinet by
 * cabinet.  prefetch == 0: every cabinet's first extract() forms its own batch; != 0: mspack_cabd_prefetch() of all of them first
 * (its time is reported as first_extract_s).  images: the cabinets back to back, image k = [offs[k], offs[k + 1]). */
int mspk_api_bench_cabs(const unsigned char *images, const unsigned long long *offs, unsigned int n_cabs, int prefetch,
                        unsigned char *out, size_t out_cap, mspk_api_stats *st)
{
  struct mem_sys ms;
  struct mscab_decompressor *d;
  struct mscabd_cabinet **cabs;
  char (*names)[12];
  unsigned int k;
  double t0, t1;
  int rc = 0;
  memset(st, 0, sizeof(*st));
  mem_sys_init(&ms, images, (size_t) offs[n_cabs], out, out_cap);
  ms.many_offs = offs; ms.n_many = n_cabs;
  cabs = (struct mscabd_cabinet **) calloc(n_cabs ? n_cabs : 1, sizeof(*cabs));
  names = (char (*)[12]) calloc(n_cabs ? n_cabs : 1, sizeof(*names));         /* (they must outlive the cabinets) */
  if (!cabs || !names) { free(cabs); free(names); return -1; }
  mspack_hip_host_path_stats(NULL, 1);
  t0 = now_s();
  if (!(d = mspack_create_cab_decompressor(&ms.sys))) { free(cabs); free(names); return -1; }
  t1 = now_s();
  for (k = 0; k < n_cabs && !rc; k++) {
    snprintf(names[k], sizeof(names[k]), "c%u", k);
    if (!(cabs[k] = d->open(d, names[k]))) { st->first_error = d->last_error(d); rc = -2; }
  }
  st->open_s = now_s() - t1;
  if (!rc && prefetch) {
    const double e0 = now_s();
    const int err = mspack_cabd_prefetch(d, cabs, (int) n_cabs);
    st->first_extract_s = now_s() - e0;
    if (err) { st->first_error = err; rc = -3; }
  }
  for (k = 0; k < n_cabs && !rc; k++) {
    struct mscabd_file *f;
    for (f = cabs[k]->files; f; f = f->next) {
      const double e0 = now_s();
      const int err = d->extract(d, f, "out");
      if (st->n_files == 0 && !prefetch) st->first_extract_s = now_s() - e0;
      if (err) { if (!st->n_errors) st->first_error = err; st->n_errors++; }
      st->n_files++;
    }
  }
  for (k = 0; k < n_cabs; k++) if (cabs[k]) d->close(d, cabs[k]);
  mspack_destroy_cab_decompressor(d);
  finish(&ms, st, t0);
  free(cabs); free(names);
  return rc;
}

/* the same cabinets, every file's MD5 through mspack_cabd_md5() instead of extract() (tools/md5_bench.py): hip_md5 = the value of
 * MSCABD_PARAM_HIP_MD5; digests receives sixteen bytes per file, in call order (at most max_files of them).  One image with
 * prefetch == 0 is "one cabinet": its first md5() forms the batch. */
static int cabs_digest_run(const unsigned char *images, const unsigned long long *offs, unsigned int n_cabs, int prefetch, int param, int value,
                           int alg, unsigned int stride, unsigned char *digests, unsigned int max_files, mspk_api_stats *st);
int mspk_api_bench_cabs_md5(const unsigned char *images, const unsigned long long *offs, unsigned int n_cabs, int prefetch, int hip_md5,
                            unsigned char *digests, unsigned int max_files, mspk_api_stats *st)
{
  return cabs_digest_run(images, offs, n_cabs, prefetch, MSCABD_PARAM_HIP_MD5, hip_md5, MSPACK_DIGEST_MD5, 16, digests, max_files, st);
}
/* ... and through mspack_cabd_digest() with algorithm alg (tools/digest_bench.py): hip_digests = the value of MSCABD_PARAM_HIP_DIGESTS;
 * digests receives 32 bytes per file (the algorithm's 16, 20 or 32, then zeros) */
int mspk_api_bench_cabs_digest(const unsigned char *images, const unsigned long long *offs, unsigned int n_cabs, int prefetch, int hip_digests,
                               int alg, unsigned char *digests, unsigned int max_files, mspk_api_stats *st)
{
  return cabs_digest_run(images, offs, n_cabs, prefetch, MSCABD_PARAM_HIP_DIGESTS, hip_digests, alg, 32, digests, max_files, st);
}
/* ... and with MSPACK_DIGEST_SHA384 / _SHA512 (tools/sha512_digest_bench.py): hip_digests64 = the value of MSCABD_PARAM_HIP_DIGESTS64;
 * digests receives 64 bytes per file (the algorithm's 48 or 64, then zeros) */
int mspk_api_bench_cabs_digest64(const unsigned char *images, const unsigned long long *offs, unsigned int n_cabs, int prefetch, int hip_digests64,
                                 int alg, unsigned char *digests, unsigned int max_files, mspk_api_stats *st)
{
  return cabs_digest_run(images, offs, n_cabs, prefetch, MSCABD_PARAM_HIP_DIGESTS64, hip_digests64, alg, 64, digests, max_files, st);
}
static int cabs_digest_run(const unsigned char *images, const unsigned long long *offs, unsigned int n_cabs, int prefetch, int param, int value,
                           int alg, unsigned int stride, unsigned char *digests, unsigned int max_files, mspk_api_stats *st)
{
  struct mem_sys ms;
  struct mscab_decompressor *d;
  struct mscabd_cabinet **cabs;
  char (*names)[12];
  unsigned int k;
  double t0, t1;
  int rc = 0;
  memset(st, 0, sizeof(*st));
  mem_sys_init(&ms, images, (size_t) offs[n_cabs], NULL, 0);
  ms.many_offs = offs; ms.n_many = n_cabs;
  cabs = (struct mscabd_cabinet **) calloc(n_cabs ? n_cabs : 1, sizeof(*cabs));
  names = (char (*)[12]) calloc(n_cabs ? n_cabs : 1, sizeof(*names));
  if (!cabs || !names) { free(cabs); free(names); return -1; }
  mspack_hip_host_path_stats(NULL, 1);
  t0 = now_s();
  if (!(d = mspack_create_cab_decompressor(&ms.sys))) { free(cabs); free(names); return -1; }
  if (d->set_param(d, param, value)) rc = -4;
  t1 = now_s();
  for (k = 0; k < n_cabs && !rc; k++) {
    snprintf(names[k], sizeof(names[k]), "c%u", k);
    if (!(cabs[k] = d->open(d, names[k]))) { st->first_error = d->last_error(d); rc = -2; }
  }
  st->open_s = now_s() - t1;
  if (!rc && prefetch) {
    const double e0 = now_s();
    const int err = mspack_cabd_prefetch(d, cabs, (int) n_cabs);
    st->first_extract_s = now_s() - e0;
    if (err) { st->first_error = err; rc = -3; }
  }
  for (k = 0; k < n_cabs && !rc; k++) {
    struct mscabd_file *f;
    for (f = cabs[k]->files; f; f = f->next) {
      unsigned char dg[64];
      const double e0 = now_s();
      const int err = (memset(dg, 0, sizeof(dg)), mspack_cabd_digest(d, f, alg, dg, sizeof(dg)));
      if (st->n_files == 0 && !prefetch) st->first_extract_s = now_s() - e0;
      if (err) { if (!st->n_errors) st->first_error = err; st->n_errors++; }
      if (digests && st->n_files < max_files) memcpy(digests + stride * (size_t) st->n_files, dg, stride);
      st->bytes_out += f->length;
      st->n_files++;
    }
  }
  for (k = 0; k < n_cabs; k++) if (cabs[k]) d->close(d, cabs[k]);
  mspack_destroy_cab_decompressor(d);
  {
    const unsigned long long hashed = st->bytes_out;
    finish(&ms, st, t0);
    st->bytes_out = hashed;                 /* (nothing was written: the bytes the digests cover) */
  }
  free(cabs); free(names);
  return rc;
}

/* one CHM image: open, extract every file of the directory in list order */
int mspk_api_bench_chm(const unsigned char *chm, size_t chm_len, unsigned char *out, size_t out_cap,
                       unsigned long long *offsets, unsigned int max_files, mspk_api_stats *st)
{
  struct mem_sys ms;
  struct mschm_decompressor *d;
  struct mschmd_header *h;
  struct mschmd_file *f;
  double t0, t1;
  memset(st, 0, sizeof(*st));
  mem_sys_init(&ms, chm, chm_len, out, out_cap);
  mspack_hip_host_path_stats(NULL, 1);
  t0 = now_s();
  if (!(d = mspack_create_chm_decompressor(&ms.sys))) return -1;
  t1 = now_s();
  h = d->open(d, "in");
  st->open_s = now_s() - t1;
  if (!h) { st->first_error = d->last_error(d); mspack_destroy_chm_decompressor(d); return -2; }
  for (f = h->files; f; f = f->next) {
    const double e0 = now_s();
    int err;
    if (offsets && st->n_files < max_files) offsets[st->n_files] = ms.out_len;
    err = d->extract(d, f, "out");
    if (st->n_files == 0) st->first_extract_s = now_s() - e0;
    if (err) { if (!st->n_errors) st->first_error = err; st->n_errors++; }
    st->n_files++;
  }
  if (offsets && st->n_files < max_files) offsets[st->n_files] = ms.out_len;
  d->close(d, h);
  mspack_destroy_chm_decompressor(d);
  finish(&ms, st, t0);
  return 0;
}

/* the same CHM, every file's digest through mspack_chmd_digest() with algorithm alg instead of extract() (tools/chm_digest_bench.py):
 * hip_digests = the value of MSCHMD_PARAM_HIP_DIGESTS; digests receives 32 bytes per file in list order (the algorithm's 16, 20 or
 * 32, then zeros; at most max_files of them) */
int mspk_api_bench_chm_digest(const unsigned char *chm, size_t chm_len, int hip_digests, int alg, unsigned char *digests,
                              unsigned int max_files, mspk_api_stats *st)
{
  struct mem_sys ms;
  struct mschm_decompressor *d;
  struct mschmd_header *h;
  struct mschmd_file *f;
  double t0, t1;
  memset(st, 0, sizeof(*st));
  mem_sys_init(&ms, chm, chm_len, NULL, 0);
  mspack_hip_host_path_stats(NULL, 1);
  t0 = now_s();
  if (!(d = mspack_create_chm_decompressor(&ms.sys))) return -1;
  if (mspack_chmd_set_param(d, MSCHMD_PARAM_HIP_DIGESTS, hip_digests)) { mspack_destroy_chm_decompressor(d); return -4; }
  t1 = now_s();
  h = d->open(d, "in");
  st->open_s = now_s() - t1;
  if (!h) { st->first_error = d->last_error(d); mspack_destroy_chm_decompressor(d); return -2; }
  for (f = h->files; f; f = f->next) {
    unsigned char dg[32];
    const double e0 = now_s();
    const int err = (memset(dg, 0, sizeof(dg)), mspack_chmd_digest(d, f, alg, dg, sizeof(dg)));
    if (st->n_files == 0) st->first_extract_s = now_s() - e0;
    if (err) { if (!st->n_errors) st->first_error = err; st->n_errors++; }
    if (digests && st->n_files < max_files) memcpy(digests + 32 * (size_t) st->n_files, dg, 32);
    st->bytes_out += (unsigned long long) f->length;
    st->n_files++;
  }
  d->close(d, h);
  mspack_destroy_chm_decompressor(d);
  {
    const unsigned long long hashed = st->bytes_out;
    finish(&ms, st, t0);
    st->bytes_out = hashed;                 /* (nothing was written: the bytes the digests cover) */
  }
  return 0;
}

/* MANY CHM images on ONE decompressor -- the help collection of small CHMs (tools/chm_prefetch_bench.py): open them all, then every
 * file, CHM by CHM.  prefetch == 0: every CHM's first call decodes its own chunk; != 0: mspack_chmd_prefetch() of all of them first
 * (its time is reported as first_extract_s).  alg == 0: extract() into `out`; else mspack_chmd_digest(alg) with
 * MSCHMD_PARAM_HIP_DIGESTS = hip_digests, digests receiving 32 bytes per file in call order (at most max_files of them).
 * images: the CHMs back to back, image k = [offs[k], offs[k + 1]). */
int mspk_api_bench_chms(const unsigned char *images, const unsigned long long *offs, unsigned int n_chms, int prefetch, int hip_digests,
                        int alg, unsigned char *out, size_t out_cap, unsigned char *digests, unsigned int max_files, mspk_api_stats *st)
{
  struct mem_sys ms;
  struct mschm_decompressor *d;
  struct mschmd_header **chms;
  char (*names)[12];
  unsigned int k;
  double t0, t1;
  int rc = 0;
  memset(st, 0, sizeof(*st));
  mem_sys_init(&ms, images, (size_t) offs[n_chms], alg ? NULL : out, alg ? 0 : out_cap);
  ms.many_offs = offs; ms.n_many = n_chms;
  chms = (struct mschmd_header **) calloc(n_chms ? n_chms : 1, sizeof(*chms));
  names = (char (*)[12]) calloc(n_chms ? n_chms : 1, sizeof(*names));         /* (they must outlive the CHMs) */
  if (!chms || !names) { free(chms); free(names); return -1; }
  mspack_hip_host_path_stats(NULL, 1);
  t0 = now_s();
  if (!(d = mspack_create_chm_decompressor(&ms.sys))) { free(chms); free(names); return -1; }
  if (mspack_chmd_set_param(d, MSCHMD_PARAM_HIP_DIGESTS, hip_digests)) rc = -4;
  t1 = now_s();
  for (k = 0; k < n_chms && !rc; k++) {
    snprintf(names[k], sizeof(names[k]), "c%u", k);
    if (!(chms[k] = d->open(d, names[k]))) { st->first_error = d->last_error(d); rc = -2; }
  }
  st->open_s = now_s() - t1;
  if (!rc && prefetch) {
    const double e0 = now_s();
    const int err = mspack_chmd_prefetch(d, chms, (int) n_chms);
    st->first_extract_s = now_s() - e0;
    if (err) { st->first_error = err; rc = -3; }
  }
  for (k = 0; k < n_chms && !rc; k++) {
    struct mschmd_file *f;
    for (f = chms[k]->files; f; f = f->next) {
      unsigned char dg[32];
      const double e0 = now_s();
      const int err = alg ? (memset(dg, 0, sizeof(dg)), mspack_chmd_digest(d, f, alg, dg, sizeof(dg))) : d->extract(d, f, "out");
      if (st->n_files == 0 && !prefetch) st->first_extract_s = now_s() - e0;
      if (err) { if (!st->n_errors) st->first_error = err; st->n_errors++; }
      if (alg && digests && st->n_files < max_files) memcpy(digests + 32 * (size_t) st->n_files, dg, 32);
      if (alg) st->bytes_out += (unsigned long long) f->length;
      st->n_files++;
    }
  }
  for (k = 0; k < n_chms; k++) if (chms[k]) d->close(d, chms[k]);
  mspack_destroy_chm_decompressor(d);
  {
    const unsigned long long hashed = st->bytes_out;
    finish(&ms, st, t0);
    if (alg) st->bytes_out = hashed;        /* (nothing was written: the bytes the digests cover) */
  }
  free(chms); free(names);
  return rc;
}

/* the files order[0..n) of one cabinet image extracted one after another with ONE decompressor (MSCABD_PARAM_FIXMSZIP /
 * _SALVAGE as given) -- the call sequence of oracle/ref_harness.c:refh_cab_extract, for the driver tests that compare error
 * codes, bytes and the MESSAGE LOG with the real reference's.  Every extract's bytes land at out_offs[i]; msgs receives the
 * formatted messages, one per line, with a '#extract i' line in front of every call. */
int mspk_api_cab_run(const unsigned char *cab, size_t cab_len, const int *order, int n_order, int fix_mszip, int salvage,
                     unsigned char *out, size_t out_cap, unsigned long long *out_offs, unsigned long long *out_lens, int *errs,
                     char *msgs, size_t msgs_cap)
{
  struct mem_sys ms;
  struct mscab_decompressor *d;
  struct mscabd_cabinet *c;
  int i;
  mem_sys_init(&ms, cab, cab_len, out, out_cap);
  g_log = msgs; g_log_cap = msgs_cap; g_log_len = 0;
  if (msgs && msgs_cap) msgs[0] = 0;
  if (!(d = mspack_create_cab_decompressor(&ms.sys))) { g_log = NULL; return -1; }
  d->set_param(d, MSCABD_PARAM_FIXMSZIP, fix_mszip);
  d->set_param(d, MSCABD_PARAM_SALVAGE, salvage);
  if (!(c = d->open(d, "in"))) { i = d->last_error(d); mspack_destroy_cab_decompressor(d); g_log = NULL; return i ? i : -2; }
  for (i = 0; i < n_order; i++) {
    struct mscabd_file *f = c->files;
    char mark[32];
    int k = order[i];
    size_t before = ms.out_len;
    while (f && k-- > 0) f = f->next;
    out_offs[i] = before; out_lens[i] = 0;
    if (!f) { errs[i] = MSPACK_ERR_ARGS; continue; }
    snprintf(mark, sizeof(mark), "#extract %d", i);
    log_line(mark);
    errs[i] = d->extract(d, f, "out");
    out_lens[i] = ms.out_len - before;
  }
  d->close(d, c);
  mspack_destroy_cab_decompressor(d);
  g_log = NULL;
  return 0;
}
