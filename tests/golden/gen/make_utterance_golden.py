#!/usr/bin/env python3
"""Regenerates tests/golden/utterance_expected.json: what the REFERENCE's own get_utterance_features (inner module 7 of its bundle) returns under
Node for every result prefix of every case of tests/utterance_cases.py, through make_utterance_golden.js — per row the non-zero slots of the 264
only, as (slot, index into the file's table of distinct doubles, each a big-endian hex string).  The inputs are not stored (the cases module
builds them again); a digest of each case's bytes is.  Y()'s ingredients (first start, summed lengths) are not stored either: the cases module
recomputes them.

Build-container only (needs /root/reference and node).  Nothing of the reference's source is written anywhere.

    python3 tests/golden/gen/make_utterance_golden.py
"""
import base64
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLD)))
from tests import utterance_cases as uc  # noqa: E402

REF = "/root/reference"
ZERO = "0000000000000000"


def main():
    job = dict(bundle=os.path.join(REF, "dist/main.js"),
               cases=[dict(name=c["name"], segs=[[s[0], s[1]] for s in c["segs"]],
                           results=[dict(syl=[list(p) for p in r["syl"]], frames=base64.b64encode(r["frames"].tobytes()).decode()) for r in c["results"]])
                      for c in uc.CASES])
    with tempfile.TemporaryDirectory() as td:
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_utterance_golden.js"), jp, op], check=True, timeout=900)
        got = json.load(open(op))
    values, index, cases, nrows, nslots = [], {}, [], 0, 0
    for c, g in zip(uc.CASES, got["cases"]):
        assert g["name"] == c["name"] and len(g["rows"]) == len(c["results"])
        rows = []
        for row in g["rows"]:
            assert len(row) == uc.NBINS
            flat = []
            for slot, h in enumerate(row):
                if h != ZERO:
                    if h not in index:
                        index[h] = len(values)
                        values.append(h)
                    flat += [slot, index[h]]
            rows.append(flat)
            nrows += 1
            nslots += len(flat) // 2
        cases.append(dict(name=c["name"], digest=uc.digest(c), rows=rows))
    out = dict(generator="tests/golden/gen/make_utterance_golden.py", node=got["node"], values=values, cases=cases)
    path = os.path.join(GOLD, "utterance_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases,", nrows, "rows,", nslots, "non-zero slots,", len(values), "distinct doubles")


if __name__ == "__main__":
    sys.exit(main())
