#!/usr/bin/env python3
"""Regenerates tests/golden/fold_expected.json: the hand-built cases of tests/fold_cases.py through the REFERENCE application's own
src/prediction.js under Node (make_fold_golden.js), with nn_mod's classifier replaced by a stub that answers with the cases'
confidences.  How ml5's classifyMultiple orders equal and all-NaN confidences is obtained from ml5 itself first, through throw-away
model directories written to a temp folder (one Dense softmax layer with a zero kernel: the biases alone decide the probabilities, a NaN
feature makes the row NaN), and stored next to the cases.

Build-container only (needs /root/reference and node).  The fixture holds the cases' inputs (step, legends, t_len, confidences) and
what the reference answered; nothing of the reference's source is written anywhere.  NaN is stored as the string "NaN".

    python3 tests/golden/gen/make_fold_golden.py [out.json]
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLD))
REF = "/root/reference"
sys.path.insert(0, ROOT)

from tests import fold_cases  # noqa: E402
from webspeechanalyzer_amd import nnmodel  # noqa: E402


def enc(v):
    v = float(v)
    return "NaN" if v != v else v


def case_json(c):
    return dict(name=c["name"], step_s=c["step_s"], legends=c["legends"], dtype=c["dtype"],
                callbacks=[dict(t_len=cb["t_len"], conf=[[[enc(v) for v in row] for row in m] for m in cb["conf"]]) for cb in c["callbacks"]])


def probe_dirs(td):
    """name, legend, biases, input rows: equal biases give bit-equal probabilities"""
    probes = []
    for name, legend, bias, rows in (
            ("four-equal", ["p", "q", "r", "s"], [0, 0, 0, 0], [[0.5, 0.5], [0.25, 0.75]]),
            ("two-pairs", ["p", "q", "r", "s"], [1, 0, 1, 0], [[0.5, 0.5], [0.25, 0.75]]),
            ("second-pair-larger", ["p", "q", "r", "s"], [0, 1, 0, 1], [[0.5, 0.5], [0.25, 0.75]]),
            ("all-nan", ["p", "q", "r", "s"], [0.5, 0, 1, 0.25], [["NaN", 0.5], [0.5, "NaN"]]),
            ("all-nan-six", ["u", "v", "w", "x", "y", "z"], [0, 1, 2, 3, 4, 5], [["NaN", "NaN"], [0.5, "NaN"]])):
        C = len(legend)
        spec = nnmodel.ModelSpec([2, C], ["softmax"], [np.zeros((2, C), np.float32)], [np.array(bias, np.float32)],
                                 np.zeros(2), np.ones(2), legend)
        d = os.path.join(td, name)
        nnmodel.save_dir(spec, d)
        probes.append(dict(name=name, dir=d, rows=rows))
    return probes


def main():
    cases = [case_json(c) for c in fold_cases.CASES]
    with tempfile.TemporaryDirectory() as td:
        job = dict(ml5=os.path.join(REF, "dist/ml5.min.js"), prediction=os.path.join(REF, "src/prediction.js"), probes=probe_dirs(td), cases=cases)
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_fold_golden.js"), jp, op], check=True, timeout=1200)
        out = json.load(open(op))
    assert [c["name"] for c in out["cases"]] == [c["name"] for c in cases]
    for c, inp in zip(out["cases"], cases):
        assert len(c["callbacks"]) == len(inp["callbacks"])
        c["input"] = inp
    out["inputs"] = "tests/fold_cases.py: CASES"
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLD, "fold_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases,", sum(len(c["callbacks"]) for c in cases), "callbacks")


if __name__ == "__main__":
    sys.exit(main())
