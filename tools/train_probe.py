#!/usr/bin/env python3
"""Times one K7 training epoch (wsa_trainer_epoch) with events on the stream: median of N epochs after warm-up, for the shape of the
app's model 1 (53-256-64-16-4) and the 512-wide shape (53-512-512-8), 74 249 rows, batch 32 and 1024; beside it one epoch of the
float64 numpy restatement (tests/train_ref.py) on the host's CPUs.  Prints one JSON line per configuration.

    python tools/train_probe.py [--epochs 20] [--warmup 3] [--rows 74249] [--no-cpu] [--only I]
    rocprofv3 --kernel-trace --stats -d DIR -o k7 -- python tools/train_probe.py --no-cpu --only 0 --epochs 3 --warmup 1   (then tools/rocprof_summary.py DB train_)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=74249)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", type=int, default=None, help="one configuration, 0 .. 3 in the order printed (for a kernel trace of its own)")
    a = ap.parse_args()
    import torch
    from tests import train_ref
    from webspeechanalyzer_amd import capi, nnmodel, train
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    rng = np.random.default_rng(1)
    index = -1
    for units in ([53, 256, 64, 16, 4], [53, 512, 512, 8]):
        C = units[-1]
        lab = (np.arange(a.rows) % C).astype(np.int32)
        centres = rng.uniform(-1, 1, (C, 53)) * 3
        feat = centres[lab] + rng.standard_normal((a.rows, 53))
        acts = ["relu"] * (len(units) - 2) + ["softmax"]
        ks, bs = train.glorot_init(units, 2)
        spec = nnmodel.ModelSpec(units, acts, ks, bs, feat.min(axis=0), feat.max(axis=0), [str(c) for c in range(C)])
        n_train, n_val = train.split(a.rows)
        for batch in (32, 1024):
            index += 1
            if a.only is not None and a.only != index:
                continue
            tr = an.trainer(spec, feat, lab, n_val, batch, 0.05)
            order = train.epoch_orders(n_train, 1, 3)[0]
            s = torch.cuda.current_stream()
            ms = []
            for e in range(a.warmup + a.epochs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                tr.epoch(order, s.cuda_stream)
                e1.record(s)
                e1.synchronize()
                if e >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
            st = tr.stats(s.cuda_stream)
            tr.close()
            L, steps = len(units) - 1, -(-n_train // batch)
            rec = dict(units=units, rows=a.rows, batch=batch, steps=steps, launches_per_step=3 * L, launches_per_epoch=3 * L * steps + L + 2,
                       epoch_ms_median=float(np.median(ms)), epoch_ms_min=float(min(ms)), epoch_ms_max=float(max(ms)), epochs_timed=len(ms),
                       us_per_step=float(np.median(ms)) * 1e3 / steps, loss=st["loss"], acc=st["acc"])
            if not a.no_cpu:
                t0 = time.perf_counter()
                train_ref.run(train_ref.normalise(feat, spec.in_min, spec.in_max), lab, ks, bs, acts, n_val, batch, 0.05, [order])
                rec["numpy_f64_epoch_ms"] = (time.perf_counter() - t0) * 1e3
            print(json.dumps(rec), flush=True)
    an.close()


if __name__ == "__main__":
    main()
