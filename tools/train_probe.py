#!/usr/bin/env python3
"""Times one K7 training epoch (wsa_trainer_epoch) with events on the stream: median of N epochs after warm-up, for the shape of the
app's model 1 (53-256-64-16-4) and the 512-wide shape (53-512-512-8), 74 249 rows, batch 32 and 1024; beside it one epoch of the
float64 numpy restatement (tests/train_ref.py) on the host's CPUs.  Prints one JSON line per configuration.

    python tools/train_probe.py [--epochs 20] [--warmup 3] [--rows 74249] [--no-cpu] [--only I]
    rocprofv3 --kernel-trace --stats -d DIR -o k7 -- python tools/train_probe.py --no-cpu --only 0 --epochs 3 --warmup 1   (then tools/rocprof_summary.py DB train_)

--group N[,N...]: training groups (K7g, wsa_train_group_epoch) instead.  For every configuration above and for a mixed set (configuration
4: one 53-256-64-16-4 classifier and three 53-64-16-1 Adam regression models, batch 32) and every N: N copies (of the mixed set: N sets,
while they fit the 32 members of a group) as ONE group epoch, beside the same trainers' N solo epochs enqueued one after another on the
same stream (the two timed in turns, epoch by epoch), and the ratio solo / group.  --which group|solo times only one of the two (for a kernel trace of its own).

    python tools/train_probe.py --group 1,2,4,8,16 [--only I]
    rocprofv3 --kernel-trace --stats -d DIR -o k7g -- python tools/train_probe.py --group 8 --only 0 --which group --epochs 3 --warmup 1
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_in_turns(torch, sides, warmup, epochs):
    """sides: {name: enqueue(stream)}; every round calls each side once, in turns, so both see the same machine; ms per side of the
    `epochs` rounds after `warmup` rounds, by events on the stream"""
    s = torch.cuda.current_stream()
    ms = {name: [] for name in sides}
    for e in range(warmup + epochs):
        for name, enqueue in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            enqueue(s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            if e >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return ms


def group_probe(a):
    import torch
    from webspeechanalyzer_amd import capi, nnmodel, train
    an = capi.Analyzer(capi.Config(output_level=13), device=0)
    rng = np.random.default_rng(1)
    n_train, n_val = train.split(a.rows)
    order = train.epoch_orders(n_train, 1, 3)[0]

    def classifier(units, batch):
        C = units[-1]
        lab = (np.arange(a.rows) % C).astype(np.int32)
        feat = (rng.uniform(-1, 1, (C, 53)) * 3)[lab] + rng.standard_normal((a.rows, 53))
        ks, bs = train.glorot_init(units, 2)
        spec = nnmodel.ModelSpec(units, ["relu"] * (len(units) - 2) + ["softmax"], ks, bs, feat.min(axis=0), feat.max(axis=0), [str(c) for c in range(C)])
        return lambda: an.trainer(spec, feat, lab, n_val, batch, 0.05)

    def regressor(units, batch):
        feat = rng.standard_normal((a.rows, 53))
        y = 1.0 / (1.0 + np.exp(-(feat[:, 3] + 0.5 * feat[:, 17] * feat[:, 40])))
        ks, bs = train.glorot_init(units, 2)
        spec = nnmodel.ModelSpec(units, ["sigmoid"] * (len(units) - 1), ks, bs, feat.min(axis=0), feat.max(axis=0), [], float(y.min()), float(y.max()))
        return lambda: an.regress_trainer(spec, feat, y, n_val, batch, 0.001)

    configs = [("53-256-64-16-4", b, [classifier([53, 256, 64, 16, 4], b)]) for b in (32, 1024)]
    configs += [("53-512-512-8", b, [classifier([53, 512, 512, 8], b)]) for b in (32, 1024)]
    configs.append(("mixed: 53-256-64-16-4 + 3 x 53-64-16-1 (Adam)", 32, [classifier([53, 256, 64, 16, 4], 32)] + [regressor([53, 64, 16, 1], 32) for _ in range(3)]))
    for index, (name, batch, makers) in enumerate(configs):
        if a.only is not None and a.only != index:
            continue
        for n in a.group:
            if n * len(makers) > capi.TRAIN_GROUP_MAX:
                continue
            trs = [m() for _ in range(n) for m in makers]
            g = an.train_group(trs)
            orders = [order] * len(trs)
            rec = dict(config=index, stack=name, batch=batch, copies=n, members=len(trs), group_launches_per_epoch=g.launches(), epochs_timed=a.epochs)

            def solo(stream):
                for t in trs:
                    t.epoch(order, stream)
            sides = {"solo": solo, "group": lambda stream: g.epoch(orders, stream)}
            for which, ms in timed_in_turns(torch, {k: v for k, v in sides.items() if a.which in (k, "both")}, a.warmup, a.epochs).items():
                rec.update({which + "_ms_median": float(np.median(ms)), which + "_ms_min": float(min(ms)), which + "_ms_max": float(max(ms))})
            if a.which == "both":
                rec["solo_over_group"] = rec["solo_ms_median"] / rec["group_ms_median"]
            g.close()
            for t in trs:
                t.close()
            print(json.dumps(rec), flush=True)
    an.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=74249)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", type=int, default=None, help="one configuration, 0 .. 3 in the order printed (for a kernel trace of its own)")
    ap.add_argument("--group", type=lambda v: [int(x) for x in v.split(",")], default=None, help="training groups of N copies (a list: 1,2,4,8,16) against N solo epochs")
    ap.add_argument("--which", choices=("both", "group", "solo"), default="both", help="with --group: time only the group epochs or only the solo epochs")
    a = ap.parse_args()
    if a.group:
        return group_probe(a)
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
