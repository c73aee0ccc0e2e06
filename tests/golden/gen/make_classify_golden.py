#!/usr/bin/env python3
"""Regenerates tests/golden/classify_expected.json (the syllable classifier's fixture) by running the REFERENCE application's
own ml5 bundle and src/prediction.js under Node through make_classify_golden.js.

Build-container only (needs /root/reference and node).  Inputs are level-13 callbacks the reference produced (the committed
fixtures config1_expected.json and backend_expected.json) plus rows pushed outside the models' input ranges; outputs are what
ml5 / prediction.js returned on them.  The two model directories the tests use are copied to tests/golden/nn/ (weights and
settings: data).  Nothing of the reference's source is written anywhere.

    python3 tests/golden/gen/make_classify_golden.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.dirname(HERE)
REF = "/root/reference"
MODELS = ["1/cats_emotion", "2/cats_emotion"]
FILES = ["model.json", "model_meta.json", "model.weights.bin"]


def _num(x):
    return float(x) if isinstance(x, str) else x        # fixtures write non-finite numbers as strings (none occur at level 13)


def _clip(key, window_step, callbacks):
    return dict(key=key, window_step=window_step,
                callbacks=[dict(si=int(cb[0]), seg_time=[[str(a), str(b)] for a, b in cb[2]], feat=[[_num(v) for v in r] for r in cb[3]])
                           for cb in callbacks])


def inputs():
    """level-13 clips: the config-1 excerpt, every level-13 case of backend_expected.json, and two clips of rows outside the
    models' ranges (model_meta.json min / max): features scaled up / pushed below the minimum, single- and multi-syllable."""
    clips = []
    c1 = json.load(open(os.path.join(GOLD, "config1_expected.json")))
    clips.append(_clip("config1_excerpt", float(c1["settings"]["window_step"]), c1["excerpt"]["level13"]["callbacks"]))
    be = json.load(open(os.path.join(GOLD, "backend_expected.json")))
    for c in be["cases"]:
        if c["level"] == 13 and c["callbacks"]:
            clips.append(_clip(c["key"], float(c["settings"]["window_step"]), c["callbacks"]))
    meta = json.load(open(os.path.join(REF, "dist/nnmodel", MODELS[0], "model_meta.json")))
    lo = np.array([meta["inputs"][str(i)]["min"] for i in range(53)])
    hi = np.array([meta["inputs"][str(i)]["max"] for i in range(53)])
    rng = np.random.default_rng(17)
    base = clips[0]
    for name, f in (("outside_high", lambda r: list(np.asarray(r) * 3.0 + hi)),
                    ("outside_low", lambda r: list(lo - np.abs(np.asarray(r)) - rng.uniform(0, 50, 53)))):
        cbs = [dict(si=cb["si"], seg_time=cb["seg_time"], feat=[[float(v) for v in f(r)] for r in cb["feat"]]) for cb in base["callbacks"]]
        cbs.append(dict(si=cbs[-1]["si"] + 1, seg_time=[["9.000", "0.105"]], feat=[[float(v) for v in f(base["callbacks"][0]["feat"][0])]]))
        clips.append(dict(key=name, window_step=base["window_step"], callbacks=cbs))
    mid = [float(v) for v in (lo + hi) / 2]                # mid-range: tfjs returns A = 0 exactly on model 1
    clips.append(dict(key="mid_range", window_step=25.0, callbacks=[dict(si=0, seg_time=[["0.100", "0.200"]], feat=[mid]),
                                                                   dict(si=1, seg_time=[["1.000", "0.075"], ["1.100", "0.150"]], feat=[mid, mid])]))
    return clips


def main():
    clips = inputs()
    os.makedirs(os.path.join(GOLD, "nn"), exist_ok=True)
    for m in MODELS:
        dst = os.path.join(GOLD, "nn", m)
        os.makedirs(dst, exist_ok=True)
        for f in FILES:
            shutil.copyfile(os.path.join(REF, "dist/nnmodel", m, f), os.path.join(dst, f))
    job = dict(ml5=os.path.join(REF, "dist/ml5.min.js"), prediction=os.path.join(REF, "src/prediction.js"),
               models={m: os.path.join(REF, "dist/nnmodel", m) for m in MODELS}, clips=clips)
    with tempfile.TemporaryDirectory() as td:
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_classify_golden.js"), jp, op], check=True, timeout=600)
        out = json.load(open(op))
    out["clips"] = clips
    out["model_dirs"] = {m: "tests/golden/nn/" + m for m in MODELS}
    with open(os.path.join(GOLD, "classify_expected.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", os.path.join(GOLD, "classify_expected.json"), sum(len(cb["feat"]) for c in clips for cb in c["callbacks"]), "rows")


if __name__ == "__main__":
    sys.exit(main())
