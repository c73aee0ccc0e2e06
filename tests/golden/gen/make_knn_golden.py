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

With --exact it writes tests/golden/knn_exact_expected.json instead: what ml5 computes on the hand-built exact rows of
tests/knn_exact_cases.py (every case marked ml5: no NaN rows, no out-of-range class, not the query-grid case), named by case key only —
the rows are rebuilt from the cases file.  A row's class index goes to ml5 as a NUMBER label, which ml5 takes as the class id itself.  Per
case: ml5's similarities [q, n] in insertion order, and per k classify()'s labels [q], its confidences [q, classes the store holds,
ascending] and the neighbours tf.topk picks [q, k_eff] in selection order — the tables as the bytes of little-endian f32 / f64 / i16
(zlib, base64: they are mostly zeros and repeats, and the file stays small).
There is no margin condition: the arithmetic on these rows is exact, for tfjs too (tests/test_knn_exact_reference.py asserts it).

    python3 tests/golden/gen/make_knn_golden.py --exact
"""
import base64
import json
import os
import subprocess
import sys
import tempfile
import zlib

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


def exact_main():
    from tests import knn_exact_cases as kc
    fixture = dict(cases={})
    for key, c in kc.CASES.items():
        if not c["ml5"]:
            continue
        out = run_node([dict(key=key, store=c["store"].tolist(), labels=[int(x) for x in c["cls"]], queries=c["queries"].tolist(), ks=list(c["ks"]))], [])
        got = out["cases"][0]
        for f in ("generator", "node", "ml5", "tfjs", "backend"):
            fixture[f] = out[f]
        assert got["class_index"] == [sorted(set(c["cls"].tolist())).index(int(x)) for x in c["cls"]], key
        grouped = np.array(got["grouped"])
        sims = np.zeros((len(c["queries"]), len(grouped)), np.float32)
        sims[:, grouped] = np.array(got["sims"], np.float32)              # ml5's grouped order -> insertion order
        def pack(a, dtype):
            return base64.b64encode(zlib.compress(np.asarray(a).astype(dtype).tobytes(), 9)).decode()
        res = got["results"]                                              # per query, per k -> per k: [q] labels, [q, classes] f64, [q, k_eff] i16
        fixture["cases"][key] = dict(class_keys=got["class_keys"], sims_f32_zlib_b64=pack(sims, "<f4"),
                                     results={str(k): dict(label=[int(r[str(k)]["label"]) for r in res], conf_f64_zlib_b64=pack([r[str(k)]["conf"] for r in res], "<f8"),
                                                           nbr_i16_zlib_b64=pack([r[str(k)]["nbr"] for r in res], "<i2")) for k in c["ks"]})
        print(key, sims.shape)
    path = os.path.join(GOLD, "knn_exact_expected.json")
    with open(path, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(exact_main() if "--exact" in sys.argv[1:] else main())
