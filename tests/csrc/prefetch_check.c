/* tests/csrc/prefetch_check.c -- TEST INFRASTRUCTURE ONLY: mspack_cabd_prefetch (include/mspack.h) under ASan + UBSan + LSan, as a
 * program of its own.  tests/test_cab_prefetch.py compiles it with libmspack_amd/csrc/host/[all].c, tests/csrc/batch_standin.c (the
 * lazy CPU stand-in for the batch ABI) and the oracle, all with -fsanitize=address,undefined, and runs it:
 *
 *     prefetch_check DIR CAB...
 *
 * CAB...: cabinets the test wrote, the plaintext of file i of each beside it as CAB.i; DIR holds split-1.cab .. split-3.cab (one
 * set) and is where the extracts are written.  Scenarios: (1) all cabinets in one batch, every file in two orders -- the answers
 * of a decompressor that was never told to prefetch, and the plaintext; (5) cabinets closed while the batch runs -- the first at
 * once, the others after their extracts; all of them before anything was waited for; the decompressor destroyed last; (6) the
 * argument checks; and a set whose members' files disappear after open(): a chain that breaks in the middle, and a folder that
 * cannot be started at all (MSPACK_ERR_OPEN: rolled back out of the batch).  Exit 0 and "PREFETCH_CHECK_OK" when everything is
 * as expected; the sanitizers' reports (leaks included) fail the run by themselves. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "mspack.h"

unsigned long mspack_standin_jobs_begun(void);

#define MAXCABS 16
#define MAXFILES 64
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "prefetch_check: line %d: %s\n", __LINE__, #c); exit(2); } } while (0)

struct blob { unsigned char *p; size_t n; };
static struct blob slurp(const char *path)
{
  struct blob b = { NULL, 0 };
  FILE *f = fopen(path, "rb");
  long n;
  if (!f) return b;
  fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
  b.p = (unsigned char *) malloc((size_t) n + 1); CHECK(b.p);
  b.n = fread(b.p, 1, (size_t) n, f);
  fclose(f);
  return b;
}
static void spit(const char *path, struct blob b)
{
  FILE *f = fopen(path, "wb");
  CHECK(f && fwrite(b.p, 1, b.n, f) == b.n);
  fclose(f);
}

struct answer { int err; struct blob out; };
static char g_out[4096];

static struct answer extract(struct mscab_decompressor *d, struct mscabd_file *f)
{
  struct answer a;
  unlink(g_out);                                            /* (a call that fails before it opens its output leaves no file) */
  a.err = d->extract(d, f, g_out);
  CHECK(d->last_error(d) == a.err);
  a.out = slurp(g_out);
  return a;
}
static int same(struct answer a, struct answer b) { return a.err == b.err && a.out.n == b.out.n && (!a.out.n || !memcmp(a.out.p, b.out.p, a.out.n)); }

/* every file of cabs[0 .. n), cabinet by cabinet: forwards, then everything backwards -> 2 * (number of files) answers */
static size_t extract_all(struct mscab_decompressor *d, struct mscabd_cabinet **cabs, int n, struct answer *ans)
{
  struct mscabd_file *list[MAXCABS * MAXFILES];
  size_t nf = 0, k, m = 0;
  int c;
  for (c = 0; c < n; c++) {
    struct mscabd_file *f;
    if (!cabs[c]) continue;
    for (f = cabs[c]->files; f; f = f->next) { CHECK(nf < MAXCABS * MAXFILES); list[nf++] = f; }
  }
  for (k = 0; k < nf; k++) ans[m++] = extract(d, list[k]);
  for (k = nf; k-- > 0; ) ans[m++] = extract(d, list[k]);
  return m;
}
static void drop(struct answer *a, size_t n) { while (n--) free(a[n].out.p); }

int main(int argc, char **argv)
{
  struct mscab_decompressor *d;
  struct mscabd_cabinet *cabs[MAXCABS];
  static struct answer plain_run[2 * MAXCABS * MAXFILES], pf_run[2 * MAXCABS * MAXFILES];
  const int n = argc - 2;
  const char *dir = argv[1];
  size_t np, nq, k;
  unsigned long b0;
  int c, i;
  CHECK(argc >= 2 + 4 && n <= MAXCABS);
  snprintf(g_out, sizeof(g_out), "%s/extract.out", dir);

  /* ---- (1) one batch, same answers ---- */
  CHECK((d = mspack_create_cab_decompressor(NULL)));
  for (c = 0; c < n; c++) CHECK((cabs[c] = d->open(d, argv[2 + c])));
  np = extract_all(d, cabs, n, plain_run);
  for (c = 0; c < n; c++) d->close(d, cabs[c]);
  mspack_destroy_cab_decompressor(d);

  CHECK((d = mspack_create_cab_decompressor(NULL)));
  for (c = 0; c < n; c++) CHECK((cabs[c] = d->open(d, argv[2 + c])));
  b0 = mspack_standin_jobs_begun();
  CHECK(mspack_cabd_prefetch(d, cabs, n) == MSPACK_ERR_OK && d->last_error(d) == MSPACK_ERR_OK);
  CHECK(mspack_standin_jobs_begun() == b0 + 1);
  nq = extract_all(d, cabs, n, pf_run);
  CHECK(np == nq && np > 0);
  for (k = 0; k < np; k++) CHECK(same(plain_run[k], pf_run[k]));
  /* the forward half against the plaintext beside the cabinets (the last cabinet is the damaged one: its first file only) */
  for (c = 0, k = 0; c < n; c++) {
    struct mscabd_file *f;
    for (f = cabs[c]->files, i = 0; f; f = f->next, i++, k++) {
      char path[4200];
      struct answer want;
      snprintf(path, sizeof(path), "%s.%d", argv[2 + c], i);
      want.err = MSPACK_ERR_OK; want.out = slurp(path);
      if (c < n - 1 || i == 0) CHECK(same(want, pf_run[k]));
      else CHECK(pf_run[k].err != MSPACK_ERR_OK);
      free(want.out.p);
    }
  }
  for (c = 0; c < n; c++) d->close(d, cabs[c]);
  mspack_destroy_cab_decompressor(d);
  drop(pf_run, nq);

  /* ---- (5) close while the job runs ---- */
  CHECK((d = mspack_create_cab_decompressor(NULL)));
  for (c = 0; c < 4; c++) CHECK((cabs[c] = d->open(d, argv[2 + c])));
  CHECK(mspack_cabd_prefetch(d, cabs, 4) == MSPACK_ERR_OK);
  b0 = mspack_standin_jobs_begun();
  d->close(d, cabs[0]); cabs[0] = NULL;                     /* (nothing of the batch has been waited for yet) */
  for (c = 3; c >= 1; c--) {
    struct mscabd_file *f;
    for (f = cabs[c]->files, i = 0; f; f = f->next, i++) {
      char path[4200];
      struct answer want, got = extract(d, f);
      snprintf(path, sizeof(path), "%s.%d", argv[2 + c], i);
      want.err = MSPACK_ERR_OK; want.out = slurp(path);
      CHECK(same(want, got));
      free(want.out.p); free(got.out.p);
    }
  }
  CHECK(mspack_standin_jobs_begun() == b0);
  for (c = 1; c < 4; c++) d->close(d, cabs[c]);
  /* ... and a batch nobody ever waits for: its last folder to leave gives it back */
  for (c = 0; c < n; c++) CHECK((cabs[c] = d->open(d, argv[2 + c])));
  CHECK(mspack_cabd_prefetch(d, cabs, n) == MSPACK_ERR_OK);
  for (c = n; c-- > 0; ) d->close(d, cabs[c]);
  mspack_destroy_cab_decompressor(d);

  /* ---- (6) arguments ---- */
  CHECK((d = mspack_create_cab_decompressor(NULL)));
  CHECK((cabs[0] = d->open(d, argv[2])) && (cabs[2] = d->open(d, argv[2 + 1])));
  cabs[1] = NULL;
  b0 = mspack_standin_jobs_begun();
  CHECK(mspack_cabd_prefetch(NULL, cabs, 1) == MSPACK_ERR_ARGS);
  CHECK(mspack_cabd_prefetch(d, cabs, 3) == MSPACK_ERR_ARGS && d->last_error(d) == MSPACK_ERR_ARGS);
  CHECK(mspack_cabd_prefetch(d, cabs, -1) == MSPACK_ERR_ARGS && d->last_error(d) == MSPACK_ERR_ARGS);
  CHECK(mspack_cabd_prefetch(d, NULL, 1) == MSPACK_ERR_ARGS && d->last_error(d) == MSPACK_ERR_ARGS);
  CHECK(mspack_cabd_prefetch(d, NULL, 0) == MSPACK_ERR_OK && d->last_error(d) == MSPACK_ERR_OK);
  CHECK(mspack_cabd_prefetch(d, cabs, 0) == MSPACK_ERR_OK);
  CHECK(mspack_standin_jobs_begun() == b0);
  cabs[1] = cabs[0];                                        /* (the same cabinet twice) */
  CHECK(mspack_cabd_prefetch(d, cabs, 3) == MSPACK_ERR_OK && mspack_standin_jobs_begun() == b0 + 1);
  CHECK(mspack_cabd_prefetch(d, cabs, 3) == MSPACK_ERR_OK && mspack_standin_jobs_begun() == b0 + 1);
  d->close(d, cabs[0]); d->close(d, cabs[2]);
  CHECK((cabs[0] = d->open(d, argv[2 + n - 2])));            /* (the cabinet with the stored folder only) */
  CHECK(mspack_cabd_prefetch(d, cabs, 1) == MSPACK_ERR_OK && mspack_standin_jobs_begun() == b0 + 1);
  d->close(d, cabs[0]);
  mspack_destroy_cab_decompressor(d);

  /* ---- a set whose files go away after open(): first its last member (the chain breaks in the middle: the folder is in the batch,
   *      with the feeder's error), then its first too (folders that start there cannot be started: MSPACK_ERR_OPEN, out of the batch) ---- */
  {
    char path[3][4200];
    struct blob img[3];
    int round, pf;
    for (i = 0; i < 3; i++) { snprintf(path[i], sizeof(path[i]), "%s/split-%d.cab", dir, i + 1); img[i] = slurp(path[i]); CHECK(img[i].n); }
    for (round = 0; round < 2; round++) {
      size_t cnt[2] = { 0, 0 };
      for (pf = 0; pf < 2; pf++) {
        struct answer *ans = pf ? pf_run : plain_run + np;      /* (plain_run[0 .. np) is still scenario 1's) */
        struct mscabd_cabinet *set[4];
        CHECK(np + 2 * MAXFILES <= 2 * MAXCABS * MAXFILES);
        for (i = 0; i < 3; i++) spit(path[i], img[i]);
        CHECK((d = mspack_create_cab_decompressor(NULL)));
        for (i = 0; i < 3; i++) CHECK((set[i] = d->open(d, path[i])));
        CHECK((set[3] = d->open(d, argv[2])));
        CHECK(d->append(d, set[0], set[1]) == MSPACK_ERR_OK && d->append(d, set[1], set[2]) == MSPACK_ERR_OK);
        CHECK(unlink(path[2]) == 0);
        if (round) CHECK(unlink(path[0]) == 0);
        if (pf) { struct mscabd_cabinet *arg[3]; arg[0] = set[1]; arg[1] = set[3]; arg[2] = set[0]; CHECK(mspack_cabd_prefetch(d, arg, 3) == MSPACK_ERR_OK); }
        set[1] = set[3];                                       /* (the set's list once, then the single cabinet) */
        cnt[pf] = extract_all(d, set, 2, ans);
        d->close(d, set[0]); d->close(d, set[3]);
        mspack_destroy_cab_decompressor(d);
      }
      CHECK(cnt[0] == cnt[1] && cnt[0] > 2);
      for (k = 0; k < cnt[0]; k++) CHECK(same(plain_run[np + k], pf_run[k]));
      if (round) { int opens = 0; for (k = 0; k < cnt[0]; k++) opens += pf_run[k].err == MSPACK_ERR_OPEN; CHECK(opens > 0); }
      CHECK(pf_run[cnt[0] / 2 - 1].err == MSPACK_ERR_OK && pf_run[cnt[0] / 2 - 1].out.n > 0);   /* (the single cabinet's file) */
      drop(plain_run + np, cnt[0]); drop(pf_run, cnt[1]);
    }
    for (i = 0; i < 3; i++) free(img[i].p);
  }
  drop(plain_run, np);
  unlink(g_out);
  puts("PREFETCH_CHECK_OK");
  return 0;
}
