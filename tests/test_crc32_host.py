"""The drivers' plain-C CRC-32 (libmspack_amd/csrc/host/crc32.c / crc32.h: table-driven, zlib's convention) stand-alone under
AddressSanitizer + UBSan, like tests/test_md5_host.py: tests/csrc/crc32_check.c is a program of its own.  Against zlib.crc32 on the edge
lengths of the device tests at sixteen alignments, and on split updates (the program compares those itself)."""
import os
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libmspack_amd", "csrc", "host")
LENGTHS = [0, 1, 3, 15, 16, 17, 1023, 1024, 65535, 65536, 65537, 131072 + 5, 196608 - 1]


def test_host_crc32_under_asan_ubsan(tmp_path):
    exe = os.path.join(ROOT, "tests", "_build", "crc32_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    p = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", HOST, os.path.join(ROOT, "tests", "csrc", "crc32_check.c"), os.path.join(HOST, "crc32.c"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=97"))
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "CRC_OK" in out and "Sanitizer" not in out and "runtime error" not in out, out[-3000:]
    x, buf = 0x12345678, bytearray(196608 + 64)
    for i in range(len(buf)):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        buf[i] = x >> 24
    rows = [tuple(int(t) for t in line.split()) for line in out.splitlines() if line and line[0].isdigit()]
    assert len(rows) == 16 * len(LENGTHS) and sorted(set(r[0] for r in rows)) == sorted(LENGTHS)
    for n, off, got in rows:
        assert got == zlib.crc32(bytes(buf[off:off + n])) & 0xFFFFFFFF, (n, off)
