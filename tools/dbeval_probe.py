#!/usr/bin/env python3
"""K8e's call times at the app's size, beside wsa_dbstats_table's in the same process (profiles/dbeval.md): a synthetic labelled DB of
`--rows` x 53 (default 376 634, the row count of dist/nnmodel/4/cats_emotion/details.txt), one categorical head of `--classes` classes (default 8, as the
app's cats_emotion; one Dense softmax layer with seeded weights over ords_V's input ranges) and three ordinal heads (ords_V's model on each), about 2 syllables per callback and about 20 rows per file.  After the
predictions each call is warmed up once and then timed `--repeats` times (>= 10) between device events around `--inner` calls; a call that
copies its result out synchronises, so these are call times, not kernel times.  Prints one JSON line with min / median per call in
microseconds; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times.

    python3 tools/dbeval_probe.py [--rows 376634] [--classes 8] [--repeats 12] [--inner 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def layout(n, rng):
    """(file_of_row, callback_of_row, n_files): files of 10 .. 30 rows, callbacks of 1 .. 3 rows"""
    import numpy as np
    file_of_row, callback_of_row = np.zeros(n, np.int32), np.zeros(n, np.int32)
    r = f = 0
    while r < n:
        rows = min(int(rng.integers(10, 31)), n - r)
        q = k = 0
        while q < rows:
            m = min(int(rng.integers(1, 4)), rows - q)
            callback_of_row[r + q:r + q + m] = k
            q, k = q + m, k + 1
        file_of_row[r:r + rows] = f
        r, f = r + rows, f + 1
    return file_of_row, callback_of_row, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=376634)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("--repeats is at least 10")
    import numpy as np
    import torch
    from webspeechanalyzer_amd import Analyzer, Config
    from tests import dbeval_cases, dbstats_cases
    an = Analyzer(Config(output_level=13))
    reg = an.load_model(dbstats_cases.model_spec("ords_V"))
    spec = dbeval_cases.model_spec(53, a.classes, 1)
    spec.in_min, spec.in_max = np.asarray(reg.spec.in_min, np.float64), np.asarray(reg.spec.in_max, np.float64)
    cls = an.load_model(spec)
    C = cls.n_classes
    s = torch.cuda.current_stream()
    q = s.cuda_stream
    n = a.rows
    rng = np.random.default_rng(n)
    lo, hi = np.asarray(reg.spec.in_min), np.asarray(reg.spec.in_max)
    feat = lo + (hi - lo) * rng.uniform(0, 1, (n, 53))
    file_of_row, callback_of_row, n_files = layout(n, rng)
    db = an.feature_db(feat, rng.integers(40, 600, n) / 1000.0, [C], 3)
    db.set_classes(0, rng.integers(-1, C, n))
    for o in range(3):
        db.set_values(o, rng.uniform(0.2, 0.8, n))
    db.set_files(file_of_row, callback_of_row, n_files)
    db.set_file_classes(0, rng.integers(-1, C, n_files))
    for o in range(3):
        db.set_file_values(o, rng.uniform(0.2, 0.8, n_files))
        db.predict_values(o, reg, stream=q)
    db.predict_classes(0, cls, np.arange(C), q)

    def folds():
        db.fold_files(0, q)
        for o in range(3):
            db.fold_file_values(o, q)

    calls = (("table", lambda: db.table(q)), ("confusion", lambda: db.confusion(0, q)), ("agreement", lambda: db.agreement(q)),
             ("fold_files", lambda: db.fold_files(0, q)), ("fold_file_values_x3", lambda: [db.fold_file_values(o, q) for o in range(3)]),
             ("file_table", lambda: db.file_table(q)), ("file_confusion", lambda: db.file_confusion(0, q)), ("file_agreement", lambda: db.file_agreement(q)))
    folds()
    for _, fn in calls:                                  # every shape the timed windows use, once: code objects, first allocations
        fn()
    s.synchronize()
    times = {name: [] for name, _ in calls}
    for _ in range(a.repeats):                           # the calls take turns inside each repeat, so that drift falls on all alike
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.inner):
                fn()
            e1.record(s)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    out = {"rows": n, "files": n_files, "classes": C, "ordinal_heads": 3, "repeats": a.repeats, "inner": a.inner,
           "us": {name: {"min": round(min(t), 1), "median": round(statistics.median(t), 1), "max": round(max(t), 1)} for name, t in times.items()}}
    cat, _, od = db.table(q)
    m = db.confusion(0, q)
    out["check"] = {"correct_wrong_blank": [int(cat["correct"][0]), int(cat["wrong"][0]), int(cat["blank"][0])], "matrix_sum": int(m.sum()),
                    "trace": int(np.trace(m[:, :C])), "pairs": [int(x) for x in db.agreement(q)["n"]], "pred_n": [int(x) for x in od["pred_n"]],
                    "files_with_a_class": int((db.file_classes(0, q) >= 0).sum())}
    db.close(); cls.close(); reg.close(); an.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
