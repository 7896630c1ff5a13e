/* tests/csrc/chm_digest_check.c -- TEST INFRASTRUCTURE ONLY: mspack_chmd_digest (include/mspack.h) under ASan + UBSan + LSan, as a
 * program of its own.  tests/test_chm_digest.py compiles it with libmspack_amd/csrc/host/[all].c (chmd.c with CHM_CHUNK_BYTES of
 * 1 MiB, so that a CHM of a few MiB has several chunks), tests/csrc/batch_standin.c and the oracle, all with
 * -fsanitize=address,undefined, and runs it:
 *
 *     chm_digest_check CHM WANT
 *
 * WANT: one line per file of the CHM in list order, "md5hex sha1hex sha256hex" of its bytes.  Scenarios: (1) one digest, then
 * close at once; (2) every file's digest, all algorithms, with a cache budget of 1 MiB -- every chunk evicts the one before --,
 * forwards and then again backwards, extract() calls in between; (3) close and destroy with every chunk's bytes and tables alive
 * (a generous budget).  Exit 0 and "CHM_DIGEST_CHECK_OK" when every digest is the expected one; the sanitizers' reports (leaks
 * included) fail the run by themselves. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mspack.h"
#include "mspack_hip.h"

#define MAXFILES 256
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "chm_digest_check: line %d: %s\n", __LINE__, #c); exit(2); } } while (0)

static const int algs[3] = { MSPACK_DIGEST_MD5, MSPACK_DIGEST_SHA1, MSPACK_DIGEST_SHA256 };
static const int lens[3] = { 16, 20, 32 };
static char want[MAXFILES][3][65];

static void hex(const unsigned char *d, int n, char *out)
{
  int i;
  for (i = 0; i < n; i++) sprintf(out + 2 * i, "%02x", d[i]);
}
static void check_file(struct mschm_decompressor *d, struct mschmd_file *f, int i, int a)
{
  unsigned char dg[32];
  char got[65];
  memset(dg, 0x55, sizeof(dg));
  CHECK(mspack_chmd_digest(d, f, algs[a], dg, sizeof(dg)) == MSPACK_ERR_OK && d->last_error(d) == MSPACK_ERR_OK);
  hex(dg, lens[a], got);
  if (strcmp(got, want[i][a])) { fprintf(stderr, "chm_digest_check: file %d alg %d: %s, expected %s\n", i, algs[a], got, want[i][a]); exit(2); }
}

int main(int argc, char **argv)
{
  struct mschm_decompressor *d;
  struct mschmd_header *chm;
  struct mschmd_file *f, *list[MAXFILES];
  unsigned char dg[32];
  int n = 0, i, a, value = -1;
  FILE *w;
  CHECK(argc == 3);
  CHECK((w = fopen(argv[2], "r")));
  while (n < MAXFILES && fscanf(w, "%64s %64s %64s", want[n][0], want[n][1], want[n][2]) == 3) n++;
  fclose(w);
  CHECK(n >= 3);

  /* ---- (1) one digest, then close at once ---- */
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  CHECK(mspack_chmd_set_param(d, MSCHMD_PARAM_HIP_DIGESTS, 7) == MSPACK_ERR_OK);
  CHECK(mspack_chmd_get_param(d, MSCHMD_PARAM_HIP_DIGESTS, &value) == MSPACK_ERR_OK && value == 7);
  CHECK((chm = d->open(d, argv[1])));
  for (f = chm->files, i = 0; f; f = f->next) { CHECK(i < MAXFILES); list[i++] = f; }
  CHECK(i == n);
  check_file(d, list[n / 2], n / 2, 2);
  d->close(d, chm);
  mspack_destroy_chm_decompressor(d);

  /* ---- (2) every file, the chunks evicting each other; then again, backwards, with extract() calls in between ---- */
  CHECK(mspack_hip_set_cache_mb(1) == 0);
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  CHECK(mspack_chmd_set_param(d, MSCHMD_PARAM_HIP_DIGESTS, 7) == MSPACK_ERR_OK);
  CHECK((chm = d->open(d, argv[1])));
  for (f = chm->files, i = 0; f; f = f->next) list[i++] = f;
  for (i = 0; i < n; i++) for (a = 0; a < 3; a++) check_file(d, list[i], i, a);
  for (i = n; i-- > 0; ) {
    if (i % 3 == 0) CHECK(d->extract(d, list[i], "/dev/null") == MSPACK_ERR_OK);
    check_file(d, list[i], i, i % 3);
  }
  /* the argument checks leave everything as it is */
  memset(dg, 0x55, sizeof(dg));
  CHECK(mspack_chmd_digest(d, list[0], 3, dg, 32) == MSPACK_ERR_ARGS && dg[0] == 0x55);
  CHECK(mspack_chmd_digest(d, list[0], MSPACK_DIGEST_SHA256, dg, 31) == MSPACK_ERR_ARGS && dg[0] == 0x55);
  CHECK(mspack_chmd_digest(d, NULL, MSPACK_DIGEST_MD5, dg, 32) == MSPACK_ERR_ARGS && dg[0] == 0 && dg[16] == 0x55);
  check_file(d, list[0], 0, 0);
  d->close(d, chm);
  mspack_destroy_chm_decompressor(d);

  /* ---- (3) close and destroy with every chunk and its tables alive ---- */
  CHECK(mspack_hip_set_cache_mb(1024) == 0);
  CHECK((d = mspack_create_chm_decompressor(NULL)));
  CHECK(mspack_chmd_set_param(d, MSCHMD_PARAM_HIP_DIGESTS, 7) == MSPACK_ERR_OK);
  CHECK((chm = d->open(d, argv[1])));
  for (f = chm->files, i = 0; f; f = f->next) list[i++] = f;
  for (i = 0; i < n; i++) check_file(d, list[i], i, (i + 1) % 3);
  d->close(d, chm);
  mspack_destroy_chm_decompressor(d);

  puts("CHM_DIGEST_CHECK_OK");
  return 0;
}
