/* tests/csrc/oab_poison_provider.c -- TEST INFRASTRUCTURE ONLY (tests/test_oab_many.py).  Linked in front of tests/csrc/batch_standin.c,
 * which is compiled with -Dmspack_hip_decode_batch=standin_decode_batch for this: a provider of the batch ABI whose batch call FAILS
 * (returns non-zero, as the real one does for an error of the runtime) whenever the batch holds a unit whose coded bytes begin with
 * "POISONED", and is the stand-in's otherwise.  It lets the CPU suite see what the OAB driver does when a batch of several files fails. */
#include <string.h>
#include "../../include/mspack_hip.h"

int standin_decode_batch(mspack_hip_unit *units, size_t n_units, const void *in, size_t in_bytes, void *out, size_t out_bytes,
                         mspack_hip_result *results);

static unsigned long g_failed;
unsigned long mspack_poison_batches_failed(void) { return g_failed; }

int mspack_hip_decode_batch(mspack_hip_unit *units, size_t n_units, const void *in, size_t in_bytes, void *out, size_t out_bytes,
                            mspack_hip_result *results)
{
  size_t i;
  for (i = 0; i < n_units; i++)
    if (units[i].in_len >= 8 && units[i].in_off + 8 <= in_bytes && !memcmp((const char *) in + units[i].in_off, "POISONED", 8)) {
      g_failed++;
      return -1;
    }
  return standin_decode_batch(units, n_units, in, in_bytes, out, out_bytes, results);
}
