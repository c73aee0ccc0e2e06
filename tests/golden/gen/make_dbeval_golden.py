#!/usr/bin/env python3
"""Regenerates tests/golden/dbeval_expected.json: the named cases of tests/dbeval_cases.py through the REFERENCE application's own
src/stats.js (only_mean, variance, covariance and the CCC expression of calc_ccc, on each ordinal case's pairs) and src/prediction.js
(Label_conf_all after each file's callbacks went through predict_by_multiple_syllables, on fixed probability tables) under Node
(make_dbeval_golden.js).

Build-container only (needs the reference's sources and node).  The fixture holds the cases' inputs and what the reference answered;
nothing of the reference's source is written anywhere.  NaN and the infinities are stored as strings.

    python3 tests/golden/gen/make_dbeval_golden.py [out.json]
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
REF = "/root/reference"
sys.path.insert(0, ROOT)

from tests import dbeval_cases  # noqa: E402


def main():
    ordinal, fold = dbeval_cases.ordinal_golden_cases(), dbeval_cases.fold_golden_cases()
    with tempfile.TemporaryDirectory() as td:
        job = dict(stats=os.path.join(REF, "src/stats.js"), prediction=os.path.join(REF, "src/prediction.js"), ordinal=ordinal, fold=fold)
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_dbeval_golden.js"), jp, op], check=True, timeout=600)
        out = json.load(open(op))
    assert [c["name"] for c in out["ordinal"]] == [c["name"] for c in ordinal] and [c["name"] for c in out["fold"]] == [c["name"] for c in fold]
    for c, inp in zip(out["ordinal"], ordinal):
        c["input"] = inp
    for c, inp in zip(out["fold"], fold):
        assert len(c["files"]) == len(inp["files"])
        c["input"] = inp
    out["inputs"] = "tests/dbeval_cases.py: ordinal_golden_cases, fold_golden_cases"
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLD, "dbeval_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(ordinal), "ordinal cases,", sum(len(c["files"]) for c in fold), "files")


if __name__ == "__main__":
    sys.exit(main())
