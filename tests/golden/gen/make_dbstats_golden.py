#!/usr/bin/env python3
"""Regenerates tests/golden/dbstats_expected.json (the fixture that pins specification DS-1: DB prediction, the `pred` pairs and the
results table's text) by running the REFERENCE application's own storage / table code and its ml5 bundle under Node through
make_dbstats_golden.js.  Build-container only (needs /root/reference and node); nothing of the reference's source is written anywhere.

Scenarios (the rows' features are those of tests/golden/train_expected.json):
  a  its 50 rows with the shipped tests/golden/nn/1/cats_emotion and a regression model for V; heads: emotion, a '*' head (spkr), a head
     without predictions (sex), one ordinal (V).  The regression model is the one tests/golden/regress_expected.json's case
     a_53_16_1_sigmoid_b16 ends with — tfjs's own result of the run TR-2 pins K7 to — because the machine that generates fixtures has
     no GPU to train on; tests/dbstats_cases.regression_spec rebuilds it from that fixture.
  b  quirks: true labels outside the class list, rows without a `true` pair, true value 0 / predicted value 0 / missing and non-numeric
     values, negative-only ordinal values, a numeric true label against a string prediction, a predicted label that is no head's
     name, 28 classes ("Many"), a non-softmax classifier whose outputs are all below 0 (null predictions).
  c  an empty selection: NaN%, Range: Infinity - 0, RMSE: 0.000.

    python3 tests/golden/gen/make_dbstats_golden.py
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
sys.path.insert(0, ROOT)
from tests import dbstats_cases  # noqa: E402
from webspeechanalyzer_amd import nnmodel  # noqa: E402

REF = "/root/reference"
EMOTION = ["N", "A", "S", "H"]          # legend order of tests/golden/nn/1/cats_emotion


def seg_time(i):
    """two toFixed(3) strings, as level 13 stores them; durations from 0.05 s to 40 s so that the minutes differ"""
    return ["%.3f" % (0.25 * i), "%.3f" % (0.053 + 0.1371 * ((i * 7) % 11) + (41.27 if i % 17 == 3 else 0.0))]


def scenario_a(rows, values):
    out = []
    for i, f in enumerate(rows["feat"]):
        out.append(dict(file="clip%02d.wav" % (i // 5), seg=str(i % 5), time=seg_time(i), features=f, origin=None,
                        true=[{"emotion": EMOTION[rows["labels"][i]], "spkr": "s%d" % (i % 3), "sex": "MF"[i % 2]}, {"V": values[i]}], pred=None))
    return dict(name="a", class_labels=[{"emotion": EMOTION}, {"spkr": ["*"]}, {"sex": ["M", "F"]}], ordinal_labels=["V"], rows=out,
                value_tol={"V": dbstats_cases.VALUE_TOL * (max(values) - min(values))},
                predict=[dict(type="cats", label="emotion", model="cats_emotion"), dict(type="ords", label="V", model="ords_V")])


def scenario_b(rows):
    out = []
    for i in range(36):
        f = rows["feat"][(i * 3) % 50]
        cat = {"emotion": EMOTION[i % 4], "digit": 3 if i % 3 else 7, "word": "w%02d" % (i % 30), "flat": "xyz"[i % 3]}
        v = [0.5, 0, 0.25, None, "abc", 0.75, 1][i % 7]
        od = {"V": v, "A": -0.1 * (1 + i % 4)}
        pred_v = [0.5, 0.4, 0, 0.3, 0.2, None, 0.875][(i // 2) % 7]
        pred = [{"digit": "3"} if i % 2 else {}, {"V": pred_v, "A": -0.2}]
        true = None if i % 9 == 4 else [cat, od]
        out.append(dict(file="q%d.wav" % (i // 4), seg=str(i % 4), time=seg_time(i + 3), features=f, origin=None, true=true,
                        pred=pred if i % 5 else None))
    return dict(name="b", class_labels=[{"emotion": ["N", "A"]}, {"digit": [3, 7]}, {"word": ["*"]}, {"flat": ["x", "y"]}],
                ordinal_labels=["V", "A"], rows=out,
                predict=[dict(type="cats", label="emotion", model="cats_emotion"), dict(type="cats", label="flat", model="cats_null"),
                         dict(type="cats", label="nohead", model="cats_emotion")])


def scenario_c(rows):
    out = [dict(file="e.wav", seg=str(i), time=seg_time(i), features=rows["feat"][i], origin=None,
                true=[{"emotion": EMOTION[i % 4]}, {"V": 0.5}], pred=None) for i in range(6)]
    return dict(name="c", class_labels=[{"emotion": ["Z"]}], ordinal_labels=["D"], rows=out, predict=[])


def main():
    with open(os.path.join(GOLD, "train_expected.json")) as f:
        rows = json.load(f)
    with open(os.path.join(GOLD, "regress_expected.json")) as f:
        values = json.load(f)["values"]
    with tempfile.TemporaryDirectory() as tmp:
        dirs = {"cats_emotion": (os.path.join(GOLD, "nn", "1", "cats_emotion"), "classification")}
        for name, spec, task in (("ords_V", dbstats_cases.regression_spec(), "regression"), ("cats_null", dbstats_cases.null_classifier_spec(), "classification")):
            d = os.path.join(tmp, name)
            nnmodel.save_dir(spec, d)
            dirs[name] = (d, task)
        scenarios = [scenario_a(rows, values), scenario_b(rows), scenario_c(rows)]
        for sc in scenarios:
            for p in sc["predict"]:
                p["dir"], p["task"] = dirs[p["model"]]
        job, res = os.path.join(tmp, "job.json"), os.path.join(tmp, "out.json")
        with open(job, "w") as f:
            json.dump(dict(ml5=os.path.join(REF, "dist", "ml5.min.js"), src=os.path.join(REF, "src"), scenarios=scenarios), f)
        subprocess.run(["node", os.path.join(HERE, "make_dbstats_golden.js"), job, res], check=True)
        with open(res) as f:
            out = json.load(f)
    out["rows_from"] = "train_expected.json"
    out["models"] = {"cats_emotion": "tests/golden/nn/1/cats_emotion", "ords_V": "regress_expected.json case a_53_16_1_sigmoid_b16, last epoch",
                     "cats_null": "tests/dbstats_cases.null_classifier_spec"}
    path = os.path.join(GOLD, "dbstats_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, os.path.getsize(path), "bytes")
    for k, v in out["scenarios"].items():
        print(k, len(v["rows"]), "rows;", " | ".join(v["lines"]))


if __name__ == "__main__":
    main()
