"""CPU: mspack_oabd_decompress_many and mspack_oabd_batch_counts in the C ABI -- the two symbols are exported, a program that takes
their addresses with the prototypes include/mspack.h documents and uses struct msoabd_job's four fields compiles without a warning
and links, the Python mirror of the struct has the C layout, and struct msoab_decompressor keeps the reference's three methods.
No compute calls are made here."""
import ctypes as C
import os
import subprocess
import tempfile

import libmspack_amd as M
from libmspack_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mspack_oabd_decompress_many", "mspack_oabd_batch_counts"]


def c_values(body, link=False):
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "mspack_hip.h"\n#include "mspack.h"\nint main(void) {\n%s\nreturn 0; }\n' % body
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.c"), os.path.join(td, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-D_FILE_OFFSET_BITS=64", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe] +
                              (["-L", os.path.dirname(M.HIP_SO), "-l:" + os.path.basename(M.HIP_SO), "-Wl,-rpath," + os.path.dirname(M.HIP_SO)] if link else []))
        return [int(x) for x in subprocess.check_output([exe]).decode().split()]


def test_new_symbols_are_exported(built):
    L = M.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert c_values('''
  int (*a)(struct msoab_decompressor *, struct msoabd_job *, int) = mspack_oabd_decompress_many;
  void (*b)(unsigned long long *, int) = mspack_oabd_batch_counts;
  struct msoabd_job j;
  j.input = "in.lzx"; j.base = NULL; j.output = "out.oab"; j.error = 0;
  printf("%d %d\\n", (int) sizeof(a) + (int) sizeof(b), j.error + (j.base == NULL) + (j.input != j.output));''', link=True) == [16, 2]


def test_struct_layouts(built):
    a = c_values('''
  printf("%zu %zu %zu %zu %zu\\n", sizeof(struct msoabd_job), offsetof(struct msoabd_job, input), offsetof(struct msoabd_job, base),
         offsetof(struct msoabd_job, output), offsetof(struct msoabd_job, error));
  printf("%zu %d\\n", sizeof(struct msoab_decompressor), MSOABD_PARAM_DECOMPBUF);''')
    J = api.MsoabdJob
    assert a[:5] == [C.sizeof(J), J.input.offset, J.base.offset, J.output.offset, J.error.offset] == [32, 0, 8, 16, 24]
    assert a[5:] == [3 * 8, 0] and C.sizeof(api.MsoabDecompressor) == 3 * 8        # three methods, as in the reference
