#!/usr/bin/env python3
"""Regenerates tests/golden/wide_expected.json: tfjs's own results at the row widths of output levels 11 (264) and 12 (23), which pin
the width-generic float64 restatements (tests/train_ref.run, tests/regress_ref.run, tests/classify_ref.forward) there.

Build-container only (needs /root/reference and node).  Drives the three existing helpers, which load the REFERENCE application's ml5
bundle (tfjs 1.7.2, CPU backend) at run time: make_train_golden.js (wide_cases w264_one_layer, w23_stack), make_regress_golden.js
(r_w23) and make_classify_golden.js (one classifyMultiple each over the rows of wide_cases.FORWARD's 264-20-4 and 23-8-3 models, saved
with nnmodel.save_dir).  Only OUTPUTS are stored: per case and epoch the history and the weights (f32, base64), per forward model the
probabilities (f32, base64).  Every input is regenerated from tests/wide_cases.py's integer hash.  Nothing of the reference's source
is written anywhere.

    python3 tests/golden/gen/make_wide_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(GOLD)))
from tests import train_ref, wide_cases as wc  # noqa: E402
from webspeechanalyzer_amd import nnmodel  # noqa: E402

REF = "/root/reference"


def node(script, job, td):
    jp, op = os.path.join(td, script + ".job.json"), os.path.join(td, script + ".out.json")
    json.dump(job, open(jp, "w"))
    subprocess.run(["node", os.path.join(HERE, script), jp, op], check=True, timeout=900)
    return json.load(open(op))


def train_job(key):
    c, i = wc.CASES[key], wc.inputs(key)
    n_train = c["n"] - c["n_val"]
    job = dict(key=key, units=c["units"], activations=c["activations"], kernels=[k.astype(np.float64).tolist() for k in i["kernels"]],
               biases=[b.astype(np.float64).tolist() for b in i["biases"]], x=i["x"].tolist(), n_val=c["n_val"], batch=c["batch"], lr=c["lr"],
               validation_split=wc.validation_split(c), orders=[(np.arange(n_train) if o is None else o).tolist() for o in i["orders"]])
    if c["regression"]:
        job["t"] = i["t"].tolist()
    else:
        job["labels"] = i["labels"].tolist()
    return job


def epochs_of(key, got):
    c = wc.CASES[key]
    n_train = c["n"] - c["n_val"]
    assert got["key"] == key and len(got["epochs"]) == c["epochs"]
    out = []
    for e in got["epochs"]:
        out.append(dict(loss=e["loss"], acc=e["acc"], val_loss=e["val_loss"], val_acc=e["val_acc"],
                        correct=int(round(e["acc"] * n_train)), val_correct=int(round(e["val_acc"] * c["n_val"])),
                        kernels=[train_ref.pack(np.array(k, np.float32)) for k in e["kernels"]],
                        biases=[train_ref.pack(np.array(b, np.float32)) for b in e["biases"]]))
    return out


def main():
    ml5 = os.path.join(REF, "dist/ml5.min.js")
    tr_keys = [k for k in wc.FIXTURE_KEYS if not wc.CASES[k]["regression"]]
    rg_keys = [k for k in wc.FIXTURE_KEYS if wc.CASES[k]["regression"]]
    out = dict(generator="tests/golden/gen/make_wide_golden.py", cases={}, forward={})
    with tempfile.TemporaryDirectory() as td:
        got = node("make_train_golden.js", dict(ml5=ml5, cases=[train_job(k) for k in tr_keys]), td)
        out.update(node=got["node"], ml5=got["ml5"], tfjs=got["tfjs"], backend=got["backend"])
        for k, g in zip(tr_keys, got["cases"]):
            out["cases"][k] = dict(epochs=epochs_of(k, g))
        got = node("make_regress_golden.js", dict(ml5=ml5, cases=[train_job(k) for k in rg_keys]), td)
        for k, g in zip(rg_keys, got["cases"]):
            out["cases"][k] = dict(epochs=epochs_of(k, g), optimizer=g["optimizer"], epsilon=g["epsilon"])
        for name in wc.FORWARD:                      # one classifyMultiple over the model's rows: a job of its own per model (the rows differ in width)
            f = wc.forward_inputs(name)
            d = os.path.join(td, name)
            nnmodel.save_dir(nnmodel.ModelSpec(f["units"], f["activations"], f["kernels"], f["biases"], f["in_min"], f["in_max"], f["labels"]), d)
            n = len(f["feat"])
            clip = dict(key=name, callbacks=[dict(si=0, seg_time=[["0.000", "0.100"]] * n, feat=f["feat"].tolist())])
            got = node("make_classify_golden.js", dict(ml5=ml5, prediction=os.path.join(REF, "src/prediction.js"), models={name: d}, clips=[clip]), td)
            m = got["models"][name]
            assert m["legend"] == f["labels"]
            out["forward"][name] = dict(prob=train_ref.pack(np.array(m["prob"], np.float32)), rows=n)
    path = os.path.join(GOLD, "wide_expected.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
