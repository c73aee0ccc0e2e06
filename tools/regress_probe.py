#!/usr/bin/env python3
"""Times one epoch of K7's regression kernels (a wsa_regress_trainer_create trainer, wsa_trainer_epoch) with events on the stream: median of
N epochs after warm-up, for the app's default regression stack (53-64-16-1, all sigmoid) on the fixture's case (b) (50 rows, batch 10)
and on 74 249 synthetic rows at batch 32 and 1024; beside each the classifier trainer on the same rows and stack widths (53-64-16-4,
softmax) for scale.  Prints one JSON line per configuration.

    python tools/regress_probe.py [--epochs 20] [--warmup 3] [--rows 74249]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, tr, order, warmup, epochs):
    s = torch.cuda.current_stream()
    ms = []
    for e in range(warmup + epochs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        tr.epoch(order, s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        if e >= warmup:
            ms.append(e0.elapsed_time(e1))
    st = tr.stats(s.cuda_stream)
    tr.close()
    return dict(epoch_ms_median=float(np.median(ms)), epoch_ms_min=float(min(ms)), epoch_ms_max=float(max(ms)), epochs_timed=len(ms), loss=st["loss"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=74249)
    a = ap.parse_args()
    import torch
    from tests import regress_ref
    from webspeechanalyzer_amd import capi, nnmodel, train
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    fx = regress_ref.load_fixture()
    case = next(c for c in fx["cases"] if c["key"].startswith("b_"))
    feat, _, y, _, ks, bs = regress_ref.case_inputs(fx, case)
    sets = [("fixture case b", feat, y, case["n_val"], [case["batch"]], (ks, bs), np.array(fx["in_min"]), np.array(fx["in_max"]), case["lr"])]
    rng = np.random.default_rng(1)
    big = rng.uniform(-1, 1, (a.rows, 53)) * 3
    yb = 0.5 + 0.3 * np.sin(big[:, 3]) + 0.05 * big[:, 17]
    sets.append((f"{a.rows} rows", big, yb, train.split(a.rows)[1], [32, 1024], train.glorot_init([53, 64, 16, 1], 2), big.min(axis=0), big.max(axis=0), 0.01))
    for name, f, v, n_val, batches, (k, b), mn, mx, lr in sets:
        n_train = len(f) - n_val
        order = train.epoch_orders(n_train, 1, 3)[0]
        for batch in batches:
            steps = -(-n_train // min(batch, n_train))
            spec = nnmodel.ModelSpec([53, 64, 16, 1], ["sigmoid"] * 3, k, b, mn, mx, [], float(v.min()), float(v.max()))
            rec = dict(set=name, stack="53-64-16-1 regression (mse, adam)", batch=batch, steps=steps, launches_per_epoch=9 * steps + 5,
                       **timed(torch, an.regress_trainer(spec, f, v, n_val, batch, lr), order, a.warmup, a.epochs))
            rec["us_per_step"] = rec["epoch_ms_median"] * 1e3 / steps
            print(json.dumps(rec), flush=True)
            k4, b4 = train.glorot_init([53, 64, 16, 4], 2)
            cls = nnmodel.ModelSpec([53, 64, 16, 4], ["sigmoid", "sigmoid", "softmax"], k4, b4, mn, mx, list("0123"))
            lab = (np.arange(len(f)) % 4).astype(np.int32)
            rec = dict(set=name, stack="53-64-16-4 classifier (cross-entropy, sgd)", batch=batch, steps=steps, launches_per_epoch=9 * steps + 5,
                       **timed(torch, an.trainer(cls, f, lab, n_val, batch, lr), order, a.warmup, a.epochs))
            rec["us_per_step"] = rec["epoch_ms_median"] * 1e3 / steps
            print(json.dumps(rec), flush=True)
    an.close()


if __name__ == "__main__":
    main()
