"""The drivers' plain-C MD5 (libmspack_amd/csrc/host/md5.c, written from RFC 1321) stand-alone under AddressSanitizer + UBSan:
tests/csrc/md5_check.c checks the RFC's test strings, every length 0..200 (and a few long ones) against digests recorded from
hashlib (tests/golden/md5_vectors.json), each in one piece and fed in pieces of 1, 7, 64 and 1000 bytes."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "libmspack_amd", "csrc", "host")


@pytest.fixture(scope="module")
def md5_check():
    os.makedirs(os.path.join(ROOT, "tests", "_build"), exist_ok=True)
    out = os.path.join(ROOT, "tests", "_build", "md5_check")
    p = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", HOST,
                        os.path.join(ROOT, "tests", "csrc", "md5_check.c"), os.path.join(HOST, "md5.c"), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return out


def test_plain_c_md5_under_sanitizers(md5_check, tmp_path):
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "md5_vectors.json")))["vectors"]
    assert [n for n, _h in vec[:201]] == list(range(201))
    lst = tmp_path / "vectors.txt"
    lst.write_text("".join("%d %s\n" % (n, h) for n, h in vec))
    p = subprocess.run([md5_check, str(lst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0 and ("MD5_OK %d lengths" % len(vec)).encode() in p.stdout, p.stdout.decode()[-3000:]
