#!/usr/bin/env python3
"""K8's time beside K6's on a labelled feature DB: for each row count a synthetic DB (features uniform inside the model's input ranges, four
true classes, one ordinal head), then `--iters` times predict classes (K6 + decide), predict values (K6 with the regression epilogue) and
the table (two passes), between events on one stream.  Prints one JSON line; run it under `rocprofv3 --kernel-trace --stats` for the
per-kernel times (profiles/dbstats.md).

    python3 tools/dbstats_probe.py [--rows 15907,1000000] [--iters 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="15907,1000000")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import numpy as np
    import torch
    from webspeechanalyzer_amd import Analyzer, Config
    from tests import dbstats_cases
    an = Analyzer(Config(output_level=13))
    cls, reg = an.load_model(dbstats_cases.model_spec("cats_emotion")), an.load_model(dbstats_cases.model_spec("ords_V"))
    s = torch.cuda.current_stream()
    out = {"iters": a.iters, "runs": []}
    for n in [int(x) for x in a.rows.split(",")]:
        rng = np.random.default_rng(n)
        lo, hi = np.asarray(reg.spec.in_min), np.asarray(reg.spec.in_max)
        feat = lo + (hi - lo) * rng.uniform(0, 1, (n, 53))
        db = an.feature_db(feat, rng.uniform(0.05, 1.5, n), [4], 1)
        db.set_classes(0, rng.integers(-1, 4, n))
        db.set_values(0, rng.uniform(0.2, 0.8, n))
        rec = {"rows": n}
        for name, fn in (("predict_classes_us", lambda: db.predict_classes(0, cls, np.arange(4), s.cuda_stream)),
                         ("predict_values_us", lambda: db.predict_values(0, reg, stream=s.cuda_stream)),
                         ("table_us", lambda: db.table(s.cuda_stream))):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.iters):
                fn()
            e1.record(s)
            e1.synchronize()
            rec[name] = e0.elapsed_time(e1) * 1e3 / a.iters
        cat, _, od = db.table(s.cuda_stream)
        rec["correct_wrong_blank"] = [int(cat["correct"][0]), int(cat["wrong"][0]), int(cat["blank"][0])]
        rec["pred_n"] = int(od["pred_n"][0])
        out["runs"].append(rec)
        db.close()
    cls.close(); reg.close(); an.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
