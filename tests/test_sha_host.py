"""The drivers' plain-C SHA-1 and SHA-256 (libmspack_amd/csrc/host/sha.c, written from FIPS 180-4) stand-alone under AddressSanitizer +
UBSan: tests/csrc/sha_check.c checks the standard's example messages (empty, "abc", the 448-bit and the 896-bit one), every length
0..130 (one piece, and pieces of 1, 7, 64 and 1000 bytes) and a 200-byte message fed in two updates cut at every point, all against
hashlib."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libmspack_amd", "csrc", "host")
ALGS = ((1, hashlib.sha1), (256, hashlib.sha256))


def message(n):
    return bytes((i * 131 + (i >> 8) * 17 + 7) & 0xFF for i in range(n))


@pytest.fixture(scope="module")
def sha_check():
    os.makedirs(os.path.join(ROOT, "tests", "_build"), exist_ok=True)
    out = os.path.join(ROOT, "tests", "_build", "sha_check")
    p = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HOST,
                        os.path.join(ROOT, "tests", "csrc", "sha_check.c"), os.path.join(HOST, "sha.c"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return out


def test_plain_c_sha_under_sanitizers(sha_check, tmp_path):
    lines = []
    for alg, h in ALGS:
        for n in list(range(131)) + [1000, 4097]:
            lines.append("%d %d %s\n" % (alg, n, h(message(n)).hexdigest()))
        for cut in range(201):
            lines.append("%d 200 %s %d\n" % (alg, h(message(200)).hexdigest(), cut))
    lst = tmp_path / "vectors.txt"
    lst.write_text("".join(lines))
    p = subprocess.run([sha_check, str(lst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and ("SHA_OK %d cases" % len(lines)).encode() in p.stdout, p.stdout.decode()[-3000:]


def test_a_wrong_digest_is_seen(sha_check, tmp_path):
    lst = tmp_path / "vectors.txt"
    lst.write_text("1 3 %s\n" % hashlib.sha1(b"abc").hexdigest())           # (not the digest of message(3))
    p = subprocess.run([sha_check, str(lst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode == 1 and b"SHA_FAIL SHA-1 length 3" in p.stdout, p.stdout.decode()[-3000:]
