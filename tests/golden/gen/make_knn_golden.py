#!/usr/bin/env python3
"""Regenerates tests/golden/knn_expected.json (the KNN classifier's fixture, specification KN-1) by running the REFERENCE application's
own ml5 bundle under Node through make_knn_golden.js.

Build-container only (needs /root/reference and node).  The rows come from tests/knn_cases.py (case key + seed); the fixture stores the
seed, not the rows, and what ml5 computed on them: its similarities (as f32, in insertion order), classify()'s label and confidences
per query and k, the neighbours tf.topk picks from those similarities, and the train_knn figure.  Nothing of the reference's source is
written anywhere.

The margin condition (so that no query ever has to be left out of a comparison): for every stored (query, k) every pair of a neighbour
and a non-neighbour whose ml5 similarities lie within MARGIN of each other must be the same unit row by construction (equal rows, or a
row and its double).  A case that fails it is redrawn with the next seed.  D = max |restatement - tfjs| over all stored similarities
is recorded: the tests' bounds refer to it.

    python3 tests/golden/gen/make_knn_golden.py
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
from tests import knn_cases, knn_ref  # noqa: E402

REF = "/root/reference"
MARGIN = 1e-5
SEED0, TRIES = 9001, 20


def run_node(cases, evals):
    job = dict(ml5=os.path.join(REF, "dist/ml5.min.js"), cases=cases, evals=evals)
    with tempfile.TemporaryDirectory() as td:
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_knn_golden.js"), jp, op], check=True, timeout=900)
        return json.load(open(op))


def margin_ok(built, sims, results):
    store = built["store"]
    n = len(store)
    for qi, per_k in enumerate(results):
        s = sims[qi].astype(np.float64)
        for k, r in per_k.items():
            inside = np.zeros(n, bool)
            inside[r["nbr"]] = True
            if inside.all():
                continue
            lo, hi = s[inside].min(), s[~inside].max()
            if lo - hi > MARGIN:
                continue
            for a in np.nonzero(inside & (s - hi <= MARGIN))[0]:
                for b in np.nonzero(~inside & (lo - s <= MARGIN))[0]:
                    if abs(s[a] - s[b]) <= MARGIN and not knn_cases.same_unit_row(store[a], store[b]):
                        return False
    return True


def one_case(key):
    for t in range(TRIES):
        seed = SEED0 + 1000 * t
        built = knn_cases.build(key, seed)
        out = run_node([dict(key=key, store=built["store"].tolist(), labels=built["labels"], queries=built["queries"].tolist(), ks=built["ks"])], [])
        got = out["cases"][0]
        grouped = np.array(got["grouped"])
        sims = np.zeros((len(built["queries"]), len(grouped)), np.float32)
        sims[:, grouped] = np.array(got["sims"], np.float32)              # ml5's grouped order -> insertion order
        if margin_ok(built, sims, got["results"]):
            return seed, built, got, sims, out
        print(f"{key}: seed {seed} misses the margin condition, redrawing")
    raise SystemExit(f"{key}: no seed in {TRIES} tries met the margin condition")


def eval_seed(classes):
    """the first seed at which every classified row of the evaluation DB keeps its k-th and (k + 1)-th neighbour more than MARGIN apart
    (exact cosines; the DB has no duplicate rows)"""
    from webspeechanalyzer_amd import knn
    for t in range(TRIES):
        seed = SEED0 + 1000 * t
        rows, labels = knn_cases.eval_db(seed)
        add, test = knn.evaluation_plan(labels, classes)
        s = -np.sort(-knn_ref.similarities(rows[add], rows[test]), axis=1)
        if (s[:, knn_cases.EVAL_K - 1] - s[:, knn_cases.EVAL_K] > MARGIN).all():
            return seed
        print(f"evaluate: seed {seed} misses the margin condition, redrawing")
    raise SystemExit("evaluate: no seed met the margin condition")


def main():
    fixture = dict(margin=MARGIN, cases={}, evals={})
    D = 0.0
    for key in knn_cases.CASES:
        seed, built, got, sims, out = one_case(key)
        for f in ("generator", "node", "ml5", "tfjs", "backend"):
            fixture[f] = out[f]
        D = max(D, float(np.abs(knn_ref.similarities(built["store"], built["queries"]) - sims.astype(np.float64)).max()))
        fixture["cases"][key] = dict(seed=seed, class_keys=got["class_keys"], class_names=got["class_names"], class_index=got["class_index"],
                                     sims=[[float(np.format_float_positional(v, unique=True, trim="-")) for v in row] for row in sims],
                                     results=[{k: dict(label=r["label"], conf=r["conf"], nbr=r["nbr"]) for k, r in per_k.items()} for per_k in got["results"]])
    for variant, classes in knn_cases.EVAL_VARIANTS.items():
        seed = eval_seed(classes)
        rows, labels = knn_cases.eval_db(seed)
        out = run_node([], [dict(key=variant, rows=rows.tolist(), labels=labels, classes=classes, k=knn_cases.EVAL_K)])
        fixture["evals"][variant] = dict(seed=seed, classes=classes, **{f: out["evals"][0][f] for f in ("samples", "correct", "all")})
    fixture["D"] = D
    path = os.path.join(GOLD, "knn_expected.json")
    with open(path, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes; D =", D)


if __name__ == "__main__":
    sys.exit(main())
