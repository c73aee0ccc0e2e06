#!/usr/bin/env python3
"""Regenerates tests/golden/regress_expected.json (the fixture that pins specification TR-2's mean-squared-error / Adam arithmetic) by
training the fixture's cases with the REFERENCE application's own ml5 bundle (tfjs 1.7.2, CPU backend) under Node through
make_regress_golden.js.

Build-container only (needs /root/reference and node).  The feature rows are those of tests/golden/train_expected.json, named by the
fixture and not copied; the targets are a smooth function of three normalised features, one decimal, clipped to 0.2 .. 0.8 so that
several rows sit exactly at the output range's ends (only those can count as "accurate", see tests/regress_ref.evaluate); the initial
weights come from tests/train_ref.case_weights (integer arithmetic; the fixture keeps their SHA-256); the orders are drawn here and
stored.  Per case a seed (orders and the weights' salt) is advanced until the float64 restatement keeps every row that can count at
least 1e-3 away from the 0.5 threshold in every evaluation, so correct counts can be compared exactly.  Nothing of the reference's
source is written anywhere.

    python3 tests/golden/gen/make_regress_golden.py
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
from tests import regress_ref, train_ref  # noqa: E402

REF = "/root/reference"
ROWS_FROM = "train_expected.json"
EPOCHS, VALIDATION_SPLIT, MIN_GAP = 4, 0.1, 1e-3

CASES = [
    # (a) 45 training rows in batches of 16: the last batch has 13
    dict(key="a_53_16_1_sigmoid_b16", units=[53, 16, 1], activations=["sigmoid", "sigmoid"], init=dict(salt=1), batch=16, lr=0.01),
    # (b) the app's own default stack and rate (nn_default_options_ords); only some rows of the wide kernels are kept
    dict(key="b_53_64_16_1_sigmoid_b10", units=[53, 64, 16, 1], activations=["sigmoid", "sigmoid", "sigmoid"], init=dict(salt=2), batch=10, lr=0.2,
         keep_rows={"0": [0, 7, 52], "1": [0, 15, 16, 63]}),
    # (c) relu then a linear output, batch 7 (45 = 6 x 7 + 3), one relu unit dead for every row: its gradients are exactly 0
    dict(key="c_53_8_1_relu_linear_dead_b7", units=[53, 8, 1], activations=["relu", "linear"], init=dict(salt=3, dead_unit=3), batch=7, lr=0.01),
    # (d) a batch larger than the training rows: one step per epoch; 272 = 17 blocks of 16 units
    dict(key="d_53_272_1_tanh_sigmoid_b64", units=[53, 272, 1], activations=["tanh", "sigmoid"], init=dict(salt=4), batch=64, lr=0.001,
         keep_rows={"0": [0, 7, 52], "1": [0, 15, 16, 255, 256, 271]}),
]


def values(x):
    y = 0.5 + 0.9 * (x[:, 3] - 0.5) + 0.7 * (x[:, 17] - 0.5) + 0.6 * (x[:, 40] - 0.5)
    return np.clip(np.round(y, 1), 0.2, 0.8)


def main():
    with open(os.path.join(GOLD, ROWS_FROM)) as f:
        rows = json.load(f)
    feat, in_min, in_max = np.array(rows["feat"], np.float64), np.array(rows["in_min"]), np.array(rows["in_max"])
    n_rows = len(feat)
    x = train_ref.normalise(feat, in_min, in_max)
    y = values(x)
    out_min, out_max = float(y.min()), float(y.max())
    t = regress_ref.normalise_target(y, out_min, out_max)
    n_val = n_rows - int(np.floor(n_rows * (1 - VALIDATION_SPLIT)))
    n_train = n_rows - n_val
    print("targets", sorted(set(y.tolist())), "at the ends: train", int(((t[:n_train] == 0) | (t[:n_train] == 1)).sum()),
          "val", int(((t[n_train:] == 0) | (t[n_train:] == 1)).sum()))
    job_cases, cases = [], []
    for c in CASES:
        seed = 100
        while True:
            assert seed < 400, "no seed gives the gap"
            c["init"]["salt"] = c["init"]["salt"] % 1000 + 1000 * (seed - 100)       # the seed moves the initial weights and the orders
            ks, bs = train_ref.case_weights(c)
            rng = np.random.default_rng(seed)
            orders = [rng.permutation(n_train).tolist() for _ in range(EPOCHS)]
            ref = regress_ref.run(x, t, ks, bs, c["activations"], n_val, c["batch"], c["lr"], orders)
            if min(e["min_gap"] for e in ref) >= MIN_GAP:
                break
            seed += 1
        if "dead_unit" in c["init"]:
            u = c["init"]["dead_unit"]
            assert np.all(x @ ks[0][:, u].astype(np.float64) + bs[0][u] < 0), "the dead unit is alive on some row"
            assert np.array_equal(ref[-1]["kernels"][0][:, u], ks[0][:, u]) and ref[-1]["biases"][0][u] == bs[0][u]
            for before, e in zip([dict(kernels=ks, biases=bs)] + ref[:-1], ref):        # the other units stay alive and keep moving
                alive = (x[:n_train] @ e["kernels"][0].astype(np.float64) + e["biases"][0] > 0).any(axis=0)
                assert alive.sum() >= 5 and not alive[u], "the live units died"
                assert not np.array_equal(before["kernels"][0], e["kernels"][0]) and not np.array_equal(before["kernels"][1], e["kernels"][1])
        print(c["key"], "order seed", seed, "min gap", min(e["min_gap"] for e in ref), "correct", [(e["correct"], e["val_correct"]) for e in ref],
              "loss", [round(e["loss"], 5) for e in ref])
        case = dict(c, n_val=n_val, validation_split=VALIDATION_SPLIT, orders=orders, order_seed=seed, init_sha256=train_ref.weights_digest(ks, bs))
        cases.append(case)
        job_cases.append(dict(key=c["key"], units=c["units"], activations=c["activations"], kernels=[k.astype(np.float64).tolist() for k in ks],
                              biases=[b.astype(np.float64).tolist() for b in bs], x=x.tolist(), t=t.tolist(), n_val=n_val, batch=c["batch"],
                              lr=c["lr"], validation_split=VALIDATION_SPLIT, orders=orders))
    job = dict(ml5=os.path.join(REF, "dist/ml5.min.js"), cases=job_cases)
    with tempfile.TemporaryDirectory() as td:
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_regress_golden.js"), jp, op], check=True, timeout=900)
        got = json.load(open(op))
    for case, g in zip(cases, got["cases"]):
        assert g["key"] == case["key"] and g["optimizer"] == "Adam" and g["epsilon"] == 1e-7, (g["optimizer"], g["epsilon"])
        eps = []
        for e in g["epochs"]:
            ks = [np.array(k, np.float32) for k in e["kernels"]]
            eps.append(dict(loss=e["loss"], acc=e["acc"], val_loss=e["val_loss"], val_acc=e["val_acc"],
                            correct=int(round(e["acc"] * n_train)), val_correct=int(round(e["val_acc"] * n_val)),
                            kernels=[train_ref.pack(train_ref.kept(case, l, k)) for l, k in enumerate(ks)],
                            biases=[train_ref.pack(np.array(b, np.float32)) for b in e["biases"]]))
        case["epochs"] = eps
    out = dict(generator="tests/golden/gen/make_regress_golden.py", node=got["node"], ml5=got["ml5"], tfjs=got["tfjs"], backend=got["backend"],
               rows_from=ROWS_FROM, values=y.tolist(), out_min=out_min, out_max=out_max, cases=cases)
    path = os.path.join(GOLD, "regress_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
