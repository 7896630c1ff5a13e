"""The drivers' plain-C SHA-384 and SHA-512 (libmspack_amd/csrc/host/sha512.c, written from FIPS 180-4) stand-alone under
AddressSanitizer + UBSan: tests/csrc/sha512_check.c checks the standard's example messages (empty, "abc", the 896-bit one) and the
lengths at which the padding changes its path (111 / 112 / 113: one final block or two; 127 / 128 / 129, 239 / 240, 255 / 256 / 257:
the block edges) and two long ones, each in one update, in pieces of 1, 7, 128 and 1000 bytes and in uneven pieces of 1, 2, 3, ...
bytes, all against hashlib."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libmspack_amd", "csrc", "host")
ALGS = ((384, hashlib.sha384), (512, hashlib.sha512))
LENGTHS = [0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 255, 256, 257, 1000, 100003]


def message(n):
    return bytes((i * 131 + (i >> 8) * 17 + 7) & 0xFF for i in range(n))


@pytest.fixture(scope="module")
def sha512_check():
    os.makedirs(os.path.join(ROOT, "tests", "_build"), exist_ok=True)
    out = os.path.join(ROOT, "tests", "_build", "sha512_check")
    p = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HOST,
                        os.path.join(ROOT, "tests", "csrc", "sha512_check.c"), os.path.join(HOST, "sha512.c"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return out


def test_plain_c_sha512_under_sanitizers(sha512_check, tmp_path):
    lines = ["%d %d %s\n" % (alg, n, h(message(n)).hexdigest()) for alg, h in ALGS for n in LENGTHS]
    lst = tmp_path / "vectors.txt"
    lst.write_text("".join(lines))
    p = subprocess.run([sha512_check, str(lst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and ("SHA512_OK %d cases" % len(lines)).encode() in p.stdout, p.stdout.decode()[-3000:]
    assert b"Sanitizer" not in p.stdout and b"runtime error" not in p.stdout, p.stdout.decode()[-3000:]


def test_a_wrong_digest_is_seen(sha512_check, tmp_path):
    lst = tmp_path / "vectors.txt"
    lst.write_text("512 3 %s\n" % hashlib.sha512(b"abc").hexdigest())           # (not the digest of message(3))
    p = subprocess.run([sha512_check, str(lst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 1 and b"SHA512_FAIL SHA-512 length 3" in p.stdout, p.stdout.decode()[-3000:]
