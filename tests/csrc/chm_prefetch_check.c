/* tests/csrc/chm_prefetch_check.c -- TEST INFRASTRUCTURE ONLY: mspack_chmd_prefetch (include/mspack.h) under ASan + UBSan + LSan, as a
 * program of its own.  tests/test_chm_prefetch.py compiles it with libmspack_amd/csrc/host/[all].c, tests/csrc/batch_standin.c and
 * the oracle, all with -fsanitize=address,undefined -- chmd.c with CHM_CHUNK_BYTES of 1 MiB: every CHM here but the last is below
 * that and one chunk as ever, the last has three (one_batch_once, sequence 6) --, and runs it:
 *
 *     chm_prefetch_check TMPDIR CHM... -- CHM CHM CHM CHM CHM CHM
 *
 * Every sequence runs twice: once without the prefetch calls -- the codes and bytes of every extract() are noted -- and once with
 * them, every extract() compared with what was noted (a damaged CHM's answers depend on the order of the calls: the same order).
 * On the stand-in's lazy jobs, without jobs (MSPACK_HIP_JOBS=0) and on two devices (the synchronous sharded call): (1)
 * prefetch, close the second CHM while the batch runs, extract every file of the others, last CHM first; (2) prefetch, close all,
 * destroy -- nothing extracted; (3) prefetch of a part, close one of it, destroy; (4) a budget of 1 MiB; over the six CHMs behind
 * "--", the sequences where a chunk's own batch and the batch of many CHMs meet (one_batch_once); and once: the argument
 * cases.  Exit 0 and "CHM_PREFETCH_CHECK_OK"; the sanitizers' reports (leaks included) fail the run by themselves. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mspack.h"
#include "mspack_hip.h"

#define MAXCHMS 8
#define MAXFILES 64
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "chm_prefetch_check: line %d: %s\n", __LINE__, #c); exit(2); } } while (0)

static int n_chms;
static char **paths;
static char out_path[1024];
static int n_files[MAXCHMS];
/* the log of a sequence's extract() calls: noted by the run without the call (g_with == 0), compared by the run with it */
#define MAXLOG 2048
static struct { int err; long len; unsigned char *data; } g_log[MAXLOG];
static int g_with, g_at, g_noted;

static unsigned char *slurp(const char *path, long *len)
{
  FILE *f = fopen(path, "rb");
  unsigned char *p;
  CHECK(f);
  CHECK(!fseek(f, 0, SEEK_END)); *len = ftell(f); CHECK(*len >= 0 && !fseek(f, 0, SEEK_SET));
  CHECK((p = (unsigned char *) malloc((size_t) *len + 1)));
  CHECK(fread(p, 1, (size_t) *len, f) == (size_t) *len);
  fclose(f);
  return p;
}

static int list_files(struct mschmd_header *chm, struct mschmd_file **list)
{
  struct mschmd_file *f;
  int n = 0;
  for (f = chm->files; f; f = f->next) { CHECK(n < MAXFILES); list[n++] = f; }
  return n;
}

static void open_all(struct mschm_decompressor *d, struct mschmd_header **chms)
{
  int k;
  for (k = 0; k < n_chms; k++) CHECK((chms[k] = d->open(d, paths[k])));
}

/* file i of CHM k: the code and the bytes of the decompressor that was never told */
static void same_as_without(struct mschm_decompressor *d, struct mschmd_header *chm, int k, int i)
{
  struct mschmd_file *list[MAXFILES];
  long len;
  unsigned char *p;
  int err;
  CHECK(list_files(chm, list) == n_files[k]);
  err = d->extract(d, list[i], out_path);
  CHECK(d->last_error(d) == err);
  p = slurp(out_path, &len);
  if (!g_with) {
    CHECK(g_at < MAXLOG);
    g_log[g_at].err = err; g_log[g_at].len = len; g_log[g_at].data = p;
    g_noted = ++g_at;
    return;
  }
  CHECK(g_at < g_noted);
  if (err != g_log[g_at].err || len != g_log[g_at].len || memcmp(p, g_log[g_at].data, (size_t) len)) {
    fprintf(stderr, "chm_prefetch_check: call %d (CHM %d file %d): err %d, %ld bytes; without the call err %d, %ld bytes\n", g_at, k, i, err, len, g_log[g_at].err, g_log[g_at].len);
    exit(2);
  }
  g_at++;
  free(p);
}
static int prefetch(struct mschm_decompressor *d, struct mschmd_header **chms, int n)
{
  return g_with ? mspack_chmd_prefetch(d, chms, n) : MSPACK_ERR_OK;
}

static void sequences_once(void)
{
  struct mschm_decompressor *d;
  struct mschmd_header *chms[MAXCHMS], *part[3];
  unsigned long long c0[2], c1[2];
  int k, i;

  /* (1) close one CHM of the batch, extract from the others */
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  open_all(d, chms);
  mspack_chmd_batch_counts(c0, 0);
  CHECK(prefetch(d, chms, n_chms) == MSPACK_ERR_OK && d->last_error(d) == MSPACK_ERR_OK);
  mspack_chmd_batch_counts(c1, 0);
  CHECK(!g_with || (c1[0] == c0[0] + 1 && c1[1] > c0[1]));
  d->close(d, chms[1]); chms[1] = NULL;
  for (k = n_chms - 1; k >= 0; k--) if (chms[k]) for (i = n_files[k] - 1; i >= 0; i--) same_as_without(d, chms[k], k, i);
  for (k = 0; k < n_chms; k++) if (chms[k]) for (i = 0; i < n_files[k]; i += 2) same_as_without(d, chms[k], k, i);
  for (k = 0; k < n_chms; k++) if (chms[k]) d->close(d, chms[k]);
  mspack_destroy_chm_decompressor(d);

  /* (2) close all and destroy without extracting anything */
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  open_all(d, chms);
  CHECK(prefetch(d, chms, n_chms) == MSPACK_ERR_OK);
  for (k = n_chms - 1; k >= 0; k--) d->close(d, chms[k]);
  mspack_destroy_chm_decompressor(d);

  /* (3) a part of the list, one of it closed, one file of another, then everything goes */
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  open_all(d, chms);
  part[0] = chms[3]; part[1] = chms[0]; part[2] = chms[3];
  CHECK(prefetch(d, part, 3) == MSPACK_ERR_OK);
  d->close(d, chms[0]); chms[0] = NULL;
  same_as_without(d, chms[3], 3, n_files[3] - 1);
  same_as_without(d, chms[2], 2, 0);                       /* (not of the batch: decoded on demand) */
  CHECK(prefetch(d, chms + 1, n_chms - 1) == MSPACK_ERR_OK);
  for (k = 0; k < n_chms; k++) if (chms[k]) d->close(d, chms[k]);
  mspack_destroy_chm_decompressor(d);

  /* (4) a budget of 1 MiB: the first CHMs only, chunks evicted behind the call */
  {
    const int old = mspack_hip_cache_mb();
    CHECK(mspack_hip_set_cache_mb(1) == 0);
    CHECK((d = mspack_create_chm_decompressor(NULL)));
    open_all(d, chms);
    CHECK(prefetch(d, chms, n_chms) == MSPACK_ERR_OK);
    for (i = 0; i < MAXFILES; i++) for (k = 0; k < n_chms; k++) if (i < n_files[k]) same_as_without(d, chms[k], k, i);
    for (k = 0; k < n_chms; k++) d->close(d, chms[k]);
    mspack_destroy_chm_decompressor(d);
    CHECK(mspack_hip_set_cache_mb(old) == 0);
  }
}

/* the sequences where a chunk's own batch (extract()) and the batch of many CHMs meet -- both are a struct chm_batch, the first
 * with one member -- over the second set: 0 lzx16-r2 (12 intervals), 1 w15-r1 (3), 2 w16-r2-small (2), 3 a CHM of one interval,
 * 4 lzx21-r2 (12), 5 a CHM of 3 MiB (48: three chunks in this build, sequence 6).  tests/test_chm_prefetch.py:
 * one_batch_sequences walks sequences 1 to 5; 6 needs the small chunks this program is built with */
unsigned long mspack_standin_jobs_begun(void);
static void counted(const unsigned long long c0[2], unsigned long long calls, unsigned long long units)
{
  unsigned long long c1[2];
  mspack_chmd_batch_counts(c1, 0);
  CHECK(!g_with || (c1[0] == c0[0] + calls && c1[1] == c0[1] + units));     /* (the run without the calls issues other batches) */
}
static void one_batch_once(void)
{
  struct mschm_decompressor *d, *d2;
  struct mschmd_header *chms[MAXCHMS];
  unsigned long long c0[2];
  unsigned long b0;
  int k, i, t;
  CHECK(n_chms == 6);

  /* (1) the chunk's own job runs with most of its units unwaited: close at once; destroy without closing (what the CHM itself
   * holds is given back through a second decompressor: close() needs the system alone) */
  CHECK((d = mspack_create_chm_decompressor(NULL)) && (chms[0] = d->open(d, paths[0])));
  same_as_without(d, chms[0], 0, 0);
  d->close(d, chms[0]);
  mspack_destroy_chm_decompressor(d);
  CHECK((d = mspack_create_chm_decompressor(NULL)) && (chms[0] = d->open(d, paths[0])));
  same_as_without(d, chms[0], 0, 0);
  mspack_destroy_chm_decompressor(d);
  CHECK((d2 = mspack_create_chm_decompressor(NULL)));
  d2->close(d2, chms[0]);
  mspack_destroy_chm_decompressor(d2);

  /* (2) two CHMs on demand, then all four told: the batch holds the others' units only; everything backward; closed in an order
   * that frees a one-member batch (CHM 0's) between the members of the shared one (CHMs 1 and 3) */
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  for (k = 0; k < 4; k++) CHECK((chms[k] = d->open(d, paths[k])));
  mspack_chmd_batch_counts(c0, 0);
  same_as_without(d, chms[0], 0, 0);
  same_as_without(d, chms[2], 2, 1);
  counted(c0, 2, 12 + 2);
  CHECK(prefetch(d, chms, 4) == MSPACK_ERR_OK);
  counted(c0, 3, 12 + 2 + 3 + 1);
  for (k = 3; k >= 0; k--) for (i = n_files[k] - 1; i >= 0; i--) same_as_without(d, chms[k], k, i);
  counted(c0, 3, 12 + 2 + 3 + 1);
  d->close(d, chms[1]); d->close(d, chms[0]); d->close(d, chms[3]); d->close(d, chms[2]);
  mspack_destroy_chm_decompressor(d);

  /* (3) two told, the first of them closed, one file of a third on demand, then all told: nothing is issued twice */
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  for (k = 0; k < 4; k++) CHECK((chms[k] = d->open(d, paths[k])));
  mspack_chmd_batch_counts(c0, 0);
  CHECK(prefetch(d, chms, 2) == MSPACK_ERR_OK);
  counted(c0, 1, 12 + 3);
  d->close(d, chms[0]);
  same_as_without(d, chms[2], 2, 1);                       /* (its file 0 is the empty one) */
  counted(c0, 2, 12 + 3 + 2);
  CHECK(prefetch(d, chms + 1, 3) == MSPACK_ERR_OK);
  counted(c0, 3, 12 + 3 + 2 + 1);
  for (k = 3; k >= 1; k--) for (i = n_files[k] - 1; i >= 0; i--) same_as_without(d, chms[k], k, i);
  CHECK(prefetch(d, chms + 1, 3) == MSPACK_ERR_OK);
  counted(c0, 3, 12 + 3 + 2 + 1);
  for (k = 1; k < 4; k++) d->close(d, chms[k]);
  mspack_destroy_chm_decompressor(d);

  /* (4) two CHMs of 768 KiB on demand, their files in turn: at the default budget (noted), at 1 MiB (compared).  (The driver's LRU
   * counts per CHM: each keeps its one chunk while the other's job may still run, nothing is evicted; sequence 6 evicts) */
  {
    const int old = mspack_hip_cache_mb();
    if (g_with) CHECK(mspack_hip_set_cache_mb(1) == 0);
    CHECK((d = mspack_create_chm_decompressor(NULL)) && (chms[0] = d->open(d, paths[0])) && (chms[4] = d->open(d, paths[4])));
    for (i = 0; i < MAXFILES; i++) for (k = 0; k <= 4; k += 4) if (i < n_files[k]) same_as_without(d, chms[k], k, i);
    d->close(d, chms[4]); d->close(d, chms[0]);
    mspack_destroy_chm_decompressor(d);
    CHECK(mspack_hip_set_cache_mb(old) == 0);
  }

  /* (6) eviction of a chunk whose own job still runs (chunk_settle on the LRU victim).  The program is built with chunks of 1 MiB
   * (CHM_CHUNK_BYTES): CHM 5 -- 3 MiB, 48 intervals of 64 KiB -- has three chunks of 16 units, every other CHM here still one.  Its
   * files: 0 in chunk 0's first interval, 1 in chunk 1, 2 in chunk 2, 3 further into chunk 0, 4 across the border of chunks 0 and
   * 1.  At 1 MiB (compared) one chunk fits: every request for another chunk evicts one whose job has only the units through that
   * the call before it needed; at the default budget (noted) every chunk is decoded once */
  {
    static const int order[6] = { 0, 1, 4, 2, 3, 0 };
    const int old = mspack_hip_cache_mb();
    unsigned long long c1[2];
    if (g_with) CHECK(mspack_hip_set_cache_mb(1) == 0);
    CHECK((d = mspack_create_chm_decompressor(NULL)) && (chms[5] = d->open(d, paths[5])));
    CHECK(n_files[5] == 5);
    mspack_chmd_batch_counts(c0, 0);
    for (i = 0; i < 6; i++) same_as_without(d, chms[5], 5, order[i]);
    mspack_chmd_batch_counts(c1, 0);
    /* (default: chunks 0, 1, 2 once.  1 MiB: 0; 1; file 4 needs interval 15's RESULT first -- of chunk 0, evicted with unit 0
     * alone waited for: what chunk_settle took over on the way out -- then the bytes of 0 and of 1 again; 2; 0 again; held) */
    CHECK(c1[0] - c0[0] == (g_with ? 6u : 3u) && c1[1] - c0[1] == (g_with ? 96u : 48u));
    d->close(d, chms[5]);
    mspack_destroy_chm_decompressor(d);
    CHECK(mspack_hip_set_cache_mb(old) == 0);
  }

  /* (5) the CHM of one interval on demand, and told alone: a batch of one unit each, never a job */
  b0 = mspack_standin_jobs_begun();
  for (t = 0; t < 2; t++) {
    CHECK((d = mspack_create_chm_decompressor(NULL)) && (chms[3] = d->open(d, paths[3])));
    mspack_chmd_batch_counts(c0, 0);
    if (t) { CHECK(prefetch(d, &chms[3], 1) == MSPACK_ERR_OK); counted(c0, 1, 1); }
    for (i = n_files[3] - 1; i >= 0; i--) same_as_without(d, chms[3], 3, i);
    if (t) counted(c0, 1, 1);
    d->close(d, chms[3]);
    mspack_destroy_chm_decompressor(d);
  }
  CHECK(mspack_standin_jobs_begun() == b0);
}

/* the two sets of CHMs the program is given (main) */
static struct chm_set { int n; char **paths; int n_files[MAXCHMS]; } g_sets[2];
static void use_set(int s)
{
  n_chms = g_sets[s].n; paths = g_sets[s].paths;
  memcpy(n_files, g_sets[s].n_files, sizeof(n_files));
}

static void sequences(void)
{
  int j;
  g_noted = 0;
  for (g_with = 0; g_with < 2; g_with++) {
    g_at = 0;
    use_set(0); sequences_once();
    use_set(1); one_batch_once();
  }
  use_set(0);
  CHECK(g_at == g_noted && g_noted > 150);
  for (j = 0; j < g_noted; j++) free(g_log[j].data);
}

int main(int argc, char **argv)
{
  struct mschm_decompressor *d;
  struct mschmd_header *chms[MAXCHMS];
  struct mschmd_file *list[MAXFILES];
  unsigned long long c0[2], c1[2];
  int k, s, sep;
  for (sep = 2; sep < argc && strcmp(argv[sep], "--"); sep++) ;
  CHECK(sep >= 6 && sep - 2 <= MAXCHMS && argc - sep - 1 == 6);
  g_sets[0].n = sep - 2; g_sets[0].paths = argv + 2;
  g_sets[1].n = argc - sep - 1; g_sets[1].paths = argv + sep + 1;
  snprintf(out_path, sizeof(out_path), "%s/out.bin", argv[1]);
  for (s = 1; s >= 0; s--) {                               /* every CHM's file count; the first set stays in use */
    use_set(s);
    CHECK((d = mspack_create_chm_decompressor(NULL)));
    open_all(d, chms);
    for (k = 0; k < n_chms; k++) { g_sets[s].n_files[k] = list_files(chms[k], list); d->close(d, chms[k]); }
    mspack_destroy_chm_decompressor(d);
  }
  use_set(0);

  /* the argument cases: nothing is gathered, no batch is started */
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  open_all(d, chms);
  mspack_chmd_batch_counts(c0, 0);
  CHECK(mspack_chmd_prefetch(NULL, chms, 1) == MSPACK_ERR_ARGS);
  CHECK(mspack_chmd_prefetch(d, chms, -1) == MSPACK_ERR_ARGS && d->last_error(d) == MSPACK_ERR_ARGS);
  CHECK(mspack_chmd_prefetch(d, NULL, 1) == MSPACK_ERR_ARGS && d->last_error(d) == MSPACK_ERR_ARGS);
  { struct mschmd_header *bad[2]; bad[0] = chms[0]; bad[1] = NULL; CHECK(mspack_chmd_prefetch(d, bad, 2) == MSPACK_ERR_ARGS && d->last_error(d) == MSPACK_ERR_ARGS); }
  CHECK(mspack_chmd_prefetch(d, NULL, 0) == MSPACK_ERR_OK && d->last_error(d) == MSPACK_ERR_OK);
  CHECK(mspack_chmd_prefetch(d, chms, 0) == MSPACK_ERR_OK);
  mspack_chmd_batch_counts(c1, 0);
  CHECK(c1[0] == c0[0] && c1[1] == c0[1]);
  mspack_chmd_batch_counts(NULL, 0);
  CHECK(mspack_chmd_prefetch(d, chms, n_chms) == MSPACK_ERR_OK);
  CHECK(mspack_chmd_prefetch(d, chms, n_chms) == MSPACK_ERR_OK);          /* everything is in the running batch: no second one */
  mspack_chmd_batch_counts(c1, 0);
  CHECK(c1[0] == c0[0] + 1);
  for (k = 0; k < n_chms; k++) d->close(d, chms[k]);
  mspack_destroy_chm_decompressor(d);

  sequences();                                              /* lazy jobs */
  CHECK(!setenv("MSPACK_HIP_JOBS", "0", 1));
  sequences();                                              /* no jobs */
  CHECK(!unsetenv("MSPACK_HIP_JOBS"));
  CHECK(mspack_hip_set_default_devices(2) == 0);
  sequences();                                              /* the sharded call */
  CHECK(mspack_hip_set_default_devices(1) == 0);

  remove(out_path);
  printf("CHM_PREFETCH_CHECK_OK\n");
  return 0;
}
