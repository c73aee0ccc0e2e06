#!/usr/bin/env python3
"""Regenerates tests/golden/coeffs_expected.json: what the REFERENCE's own make_coeffs (formantanalyzer's inner module 4, with its numeric.js)
returns under Node for every syllable of tests/coeffs_cases.py, one syllable per call through make_coeffs_golden.js — 23 doubles as hex, or
the message numeric threw with.  The inputs are not stored (the cases module builds them again); a digest of each case's bytes is.

Build-container only (needs /root/reference and node).  Nothing of the reference's source is written anywhere.

    python3 tests/golden/gen/make_coeffs_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLD)))
from tests import coeffs_cases as cc  # noqa: E402

REF = "/root/reference"


def main():
    job = dict(bundle=os.path.join(REF, "dist/main.js"),
               cases=[dict(name=c["name"], fr=c["fr"].astype(float).tolist(), sums=cc.sums3(c).astype(float).tolist()) for c in cc.CASES])
    with tempfile.TemporaryDirectory() as td:
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_coeffs_golden.js"), jp, op], check=True, timeout=900)
        got = json.load(open(op))
    cases = []
    for c, g in zip(cc.CASES, got["cases"]):
        assert g["name"] == c["name"]
        cases.append(dict(name=c["name"], sl=c["sl"], digest=cc.digest(c), row=g["row"], threw=g["threw"]))
    out = dict(generator="tests/golden/gen/make_coeffs_golden.py", node=got["node"], cases=cases)
    path = os.path.join(GOLD, "coeffs_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", sum(1 for c in cases if c["threw"]), "of", len(cases), "cases threw")


if __name__ == "__main__":
    sys.exit(main())
