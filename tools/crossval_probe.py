#!/usr/bin/env python3
"""The held-out pass of a cross-validation (K6f, spec CV-1) beside the only way to get the same column without it, and the whole
cross_validate call beside K sequential trainings (profiles/crossval.md).  A synthetic labelled DB of `--rows` x 53 (default 74 000,
about the shipped models' size), files of 10 .. 30 rows dealt to K folds by CV-1's rule, the default 53-8-C stack with seeded weights.

For every K of `--folds` (default 5 and 32), in one process, the three ways taking turns inside each repeat:
  folds      one wsa_dbstats_predict_classes_folds (zero the table, K6f, DS-1's decision), timed between device events around `--inner` calls
  whole_dev  K wsa_dbstats_predict_classes over the whole DB, device work only (the same events): K times the arithmetic, no merge
  whole      the same K calls, each followed by the copy of its probability table to the host, and the host merge of the K tables by fold:
             what a user of the parent commit has to do; a host clock around work that ends in a synchronise
and the merged table is compared with the fold-wise one, byte for byte.  With --whole-epochs N (> 0) also, once per K (after one warm-up at
2 epochs): crossval.cross_validate at N epochs against K sequential train.train runs, K whole-DB predictions and the merge.
Prints one JSON line; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times.

    python3 tools/crossval_probe.py [--rows 74000] [--classes 8] [--folds 5 32] [--repeats 12] [--inner 5] [--whole-epochs 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def files_of(n, rng):
    """file index of every row: files of 10 .. 30 rows"""
    import numpy as np
    out, r, f = np.zeros(n, np.int32), 0, 0
    while r < n:
        rows = min(int(rng.integers(10, 31)), n - r)
        out[r:r + rows] = f
        r, f = r + rows, f + 1
    return out, f


def stats(t):
    return {"min": round(min(t), 1), "median": round(statistics.median(t), 1), "max": round(max(t), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=74000)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--folds", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--whole-epochs", type=int, default=0)
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats is at least 10")
    import numpy as np
    import torch
    from webspeechanalyzer_amd import Analyzer, Config, crossval, dbstats, nnmodel, train
    an = Analyzer(Config(output_level=13))
    s = torch.cuda.current_stream()
    q = s.cuda_stream
    n, C = a.rows, a.classes
    rng = np.random.default_rng(n)
    feat = rng.uniform(0, 1, (n, 53))
    file_of_row, n_files = files_of(n, rng)
    labels = [f"c{c}" for c in range(C)]
    true = rng.integers(0, C, n)
    feat[np.arange(n), true] += 0.5                       # the class shows in the features
    units, acts = train.stack(train.DEFAULT_LAYERS, C)
    out = {"rows": n, "files": n_files, "classes": C, "stack": units, "repeats": a.repeats, "inner": a.inner, "k": {}}
    for K in a.folds:
        fold_of_row = (file_of_row % K).astype(np.int32)
        models = [an.load_model(nnmodel.ModelSpec(units, acts, *train.glorot_init(units, 2 * k), np.zeros(53), np.full(53, 1.5), labels)) for k in range(K)]
        db = an.feature_db(feat, np.full(n, 0.25), [C], 0)
        db.set_classes(0, true)
        db.set_folds(fold_of_row, K)
        ident = np.arange(C)

        def folds():
            db.predict_classes_folds(0, models, ident, q)

        def whole_dev():
            for m in models:
                db.predict_classes(0, m, ident, q)

        def whole():
            merged = np.zeros((n, C), np.float32)
            for k, m in enumerate(models):
                db.predict_classes(0, m, ident, q)
                p = db.probs(C, q)
                rows = fold_of_row == k
                merged[rows] = p[rows]
            return merged

        for fn in (folds, whole_dev, whole):             # every shape the timed windows use, once
            fn()
        s.synchronize()
        us = {"folds": [], "whole_dev": [], "whole": []}
        for _ in range(a.repeats):
            for name, fn in (("folds", folds), ("whole_dev", whole_dev)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(a.inner):
                    fn()
                e1.record(s)
                e1.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
            s.synchronize()
            t0 = time.perf_counter()
            merged = whole()
            us["whole"].append((time.perf_counter() - t0) * 1e6)
        folds()
        same = db.probs(C, q).tobytes() == merged.tobytes()
        rb = [4] * K                                      # 53-8-C: S = 68, four row blocks
        rec = {"us": {k: stats(v) for k, v in us.items()}, "same_bytes": same,
               "tiles": {"folds": crossval_tiles(np.bincount(fold_of_row, minlength=K), rb), "whole": K * ((n + 63) // 64)},
               "ratio_whole_dev_over_folds": round(statistics.median(us["whole_dev"]) / statistics.median(us["folds"]), 2),
               "ratio_whole_over_folds": round(statistics.median(us["whole"]) / statistics.median(us["folds"]), 2)}
        db.close()
        for m in models:
            m.close()
        if a.whole_epochs > 0:
            rows = [dict(file=f"f{file_of_row[i]}", seg="0", time=["0.000", "0.250"], features=feat[i], true=[{"emotion": labels[true[i]]}, {}], pred=None)
                    for i in range(n)]
            heads = ([{"emotion": labels}], [])

            def cv(epochs):
                t0 = time.perf_counter()
                r = crossval.cross_validate(an, rows, *heads, ["emotion"], K, epochs=epochs, per_file=False, keep_models=True, stream=q)
                s.synchronize()
                return time.perf_counter() - t0, r

            def sequential(epochs):
                t0 = time.perf_counter()
                data = crossval.fold_data(feat, [labels[c] for c in true], labels, fold_of_row, K)
                preds = [None] * n
                for k in range(K):
                    spec, _ = train.train(an, data[k], epochs=epochs, seed=2 * k, stream=q)
                    p = dbstats.predict_db(an, rows, heads, "cats", "emotion", spec, stream=q)
                    for i in np.flatnonzero(fold_of_row == k):
                        preds[i] = p[i]
                s.synchronize()
                return time.perf_counter() - t0, preds

            cv(2); sequential(2)
            t_cv, r = cv(a.whole_epochs)
            held = [x["pred"][0]["emotion"] for x in rows]
            t_seq, preds = sequential(a.whole_epochs)
            cat = r["rows"]["table"]["cats"][0]
            rec["whole_call"] = {"epochs": a.whole_epochs, "cross_validate_s": round(t_cv, 2), "sequential_s": round(t_seq, 2),
                                 "ratio": round(t_seq / t_cv, 2), "same_predictions": held == preds,
                                 "held_out_accuracy": round(cat["correct"] / max(cat["correct"] + cat["wrong"], 1), 4)}
        out["k"][str(K)] = rec
    an.close()
    print(json.dumps(out))


def crossval_tiles(rows_per_fold, rb):
    from webspeechanalyzer_amd import capi
    return capi.crossval_tiles(rows_per_fold, rb)


if __name__ == "__main__":
    main()
