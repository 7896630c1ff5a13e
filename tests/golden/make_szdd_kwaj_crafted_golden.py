"""Generates tests/golden/szdd_kwaj_crafted.json: what the REAL reference (oracle/_ref, development container) answers for the
SZDD and KWAJ files that tests/test_szdd_kwaj.py builds around hand-built streams of tests/crafted_streams.py: open error, extract
error, header fields, output length and MD5.  The builders are deterministic; the test rebuilds the same files (their MD5s are
recorded).  Each file is asked for three times with other work in between: these streams read no byte the reference has not
initialised, so the answers must agree."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import helpers  # noqa: E402
from test_szdd_kwaj import crafted_file_cases, sig  # noqa: E402


def main():
    assert helpers.have_ref()
    out = []
    cases = crafted_file_cases()
    for name, kind, blob in cases:
        a = sig(helpers.ref_szdd_kwaj(kind, blob))
        helpers.ref_szdd_kwaj(cases[0][1], cases[0][2])
        b = sig(helpers.ref_szdd_kwaj(kind, blob))
        helpers.ref_szdd_kwaj(cases[2][1], cases[2][2])
        assert a == b == sig(helpers.ref_szdd_kwaj(kind, blob)), name
        out.append(dict(name=name, blob_md5=hashlib.md5(blob).hexdigest(), ok=a))
        print(name, a)
    json.dump(out, open(os.path.join(HERE, "szdd_kwaj_crafted.json"), "w"), indent=0)


if __name__ == "__main__":
    main()
