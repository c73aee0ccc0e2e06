#!/usr/bin/env python3
"""Regenerates tests/golden/ensemble_expected.json (the fixture of the multi-DB prediction path) by running the REFERENCE
application's own ml5 bundle and src/prediction.js under Node through make_ensemble_golden.js, with `available_DBs` set to each
case's list of model DBs.

Build-container only (needs /root/reference and node).  Inputs are the clips of tests/golden/classify_expected.json (20 clips,
43 callbacks, 135 rows); the cases are [1, 2], [2, 1] and the six DBs the application ships, [1, 2, 4, 5, 6, 7].  Stored: every DB's
probabilities on the rows and its legend (the 1.18 MB weight files of DBs 4 .. 7 stay where they are), and per case and callback
callback_after_pred's pair, min_entropy_db, the gauge values and the entropy text, plus every DB's Label_conf_all per clip in key
order.  Nothing of the reference's source is written anywhere.

The reference ships ONE weight file under four names: dist/nnmodel/4 .. 7 hold byte-identical model.weights.bin (their md5 sums match), so
the probabilities stored for DBs 4, 5, 6 and 7 are equal and the six-DB case exercises, among those four, only "a tie goes to the earlier DB"
(DB 4 takes every callback and launch maximum the other three would).  They are stored per DB all the same: the fixture records what the
application computes with its shipped list, not what distinguishes its members.

    python3 tests/golden/gen/make_ensemble_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
REF = "/root/reference"
CASES = [[1, 2], [2, 1], [1, 2, 4, 5, 6, 7]]


def main():
    clips = json.load(open(os.path.join(GOLD, "classify_expected.json")))["clips"]
    dbs = sorted({d for c in CASES for d in c})
    job = dict(ml5=os.path.join(REF, "dist/ml5.min.js"), prediction=os.path.join(REF, "src/prediction.js"),
               models={str(d): os.path.join(REF, "dist/nnmodel", str(d), "cats_emotion") for d in dbs}, cases=CASES, clips=clips)
    with tempfile.TemporaryDirectory() as td:
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_ensemble_golden.js"), jp, op], check=True, timeout=1200)
        out = json.load(open(op))
    out["inputs"] = "tests/golden/classify_expected.json: clips"
    n_cb = sum(len(c["callbacks"]) for c in clips)
    for case in out["cases"]:
        assert sum(len(c["callbacks"]) for c in case["clips"]) == n_cb
    path = os.path.join(GOLD, "ensemble_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(clips), "clips,", n_cb, "callbacks,", sum(len(cb["feat"]) for c in clips for cb in c["callbacks"]), "rows")


if __name__ == "__main__":
    sys.exit(main())
