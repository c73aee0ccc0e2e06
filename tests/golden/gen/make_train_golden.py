#!/usr/bin/env python3
"""Regenerates tests/golden/train_expected.json (the fixture that pins specification TR-1's SGD arithmetic) by training the
fixture's cases with the REFERENCE application's own ml5 bundle (tfjs 1.7.2, CPU backend) under Node through make_train_golden.js.

Build-container only (needs /root/reference and node).  The rows are synthetic (four clusters in the 53 features, three decimals,
so the file stays small); the initial weights come from tests/train_ref.case_weights (integer arithmetic; the fixture keeps their
SHA-256); the orders are drawn here and stored.  Per case a seed (orders and the weights' salt) is advanced until the float64 restatement's top-two
probability gap is at least 1e-3 on every row of every evaluation, so correct counts can be compared exactly.  Nothing of the
reference's source is written anywhere.

    python3 tests/golden/gen/make_train_golden.py
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
from tests import train_ref  # noqa: E402

REF = "/root/reference"
N_ROWS, EPOCHS, VALIDATION_SPLIT, MIN_GAP = 50, 3, 0.1, 1e-3

CASES = [
    # (a) the app's default stack; 45 training rows in batches of 16: the last batch has 13
    dict(key="a_53_8_4_relu_b16", units=[53, 8, 4], activations=["relu", "softmax"], init=dict(salt=1), batch=16, lr=0.1, classes=4),
    # (b) sigmoid then tanh hidden layers, batch 7 (45 = 6 x 7 + 3)
    dict(key="b_53_20_12_3_sigmoid_tanh_b7", units=[53, 20, 12, 3], activations=["sigmoid", "tanh", "softmax"], init=dict(salt=2), batch=7, lr=0.1, classes=3),
    # (c) 272 = 17 blocks of 16 units; only some rows of the kernels are kept
    dict(key="c_53_272_4_relu_b16", units=[53, 272, 4], activations=["relu", "softmax"], init=dict(salt=3), batch=16, lr=0.05, classes=4,
         keep_rows={"0": [0, 7, 52], "1": [0, 15, 16, 255, 256, 271]}),
    # (d) lr 0.2, logits scaled and one class's output bias at -20 (the rows of that class have a true-class probability clipped at 1e-7 in
    # every epoch) and one relu unit dead for every row while the others stay alive and keep training
    dict(key="d_53_8_4_clip_dead_b16", units=[53, 8, 4], activations=["relu", "softmax"], init=dict(salt=4, dead_unit=3, last_scale=2.0, out_bias=[2, -20.0]), batch=16, lr=0.2, classes=4),
    # (e) a batch larger than the training rows: one step per epoch
    dict(key="e_53_8_4_relu_b64", units=[53, 8, 4], activations=["relu", "softmax"], init=dict(salt=5), batch=64, lr=0.1, classes=4),
]


def rows():
    rng = np.random.default_rng(2024)
    scale = np.round(10.0 ** rng.uniform(0, 3, 53), 0)
    centres = rng.uniform(0.2, 0.8, (4, 53))
    lab = rng.permutation(np.arange(N_ROWS) % 4)
    feat = np.round((centres[lab] + rng.standard_normal((N_ROWS, 53)) * 0.12) * scale, 3)
    return feat, lab


def main():
    feat, lab = rows()
    in_min, in_max = feat.min(axis=0), feat.max(axis=0)
    x = train_ref.normalise(feat, in_min, in_max)
    n_val = N_ROWS - int(np.floor(N_ROWS * (1 - VALIDATION_SPLIT)))
    n_train = N_ROWS - n_val
    job_cases, cases = [], []
    for c in CASES:
        y = lab % c["classes"]
        seed = 100
        while True:
            assert seed < 400, "no seed gives the top-two gap"
            c["init"]["salt"] = c["init"]["salt"] % 1000 + 1000 * (seed - 100)       # the seed moves the initial weights and the orders
            ks, bs = train_ref.case_weights(c)
            rng = np.random.default_rng(seed)
            orders = [rng.permutation(n_train).tolist() for _ in range(EPOCHS)]
            ref = train_ref.run(x, y, ks, bs, c["activations"], n_val, c["batch"], c["lr"], orders)
            if min(e["min_gap"] for e in ref) >= MIN_GAP:
                break
            seed += 1
        if "dead_unit" in c["init"]:
            u = c["init"]["dead_unit"]
            assert ref[0]["clipped"] >= 1, "case (d) needs a row clipped from below in epoch 1"
            assert np.all(x @ ks[0][:, u].astype(np.float64) + bs[0][u] < 0), "the dead unit is alive on some row"
            assert np.array_equal(ref[-1]["kernels"][0][:, u], ks[0][:, u])
            for before, e in zip([dict(kernels=ks, biases=bs)] + ref[:-1], ref):        # the other units stay alive and keep moving
                alive = (x[:n_train] @ e["kernels"][0].astype(np.float64) + e["biases"][0] > 0).any(axis=0)
                assert alive.sum() >= 5 and not alive[u], "case (d): the live units died"
                assert not np.array_equal(before["kernels"][0], e["kernels"][0]) and not np.array_equal(before["kernels"][1], e["kernels"][1])
        print(c["key"], "order seed", seed, "min gap", min(e["min_gap"] for e in ref), "clipped", [e["clipped"] for e in ref])
        case = dict(c, n_val=n_val, validation_split=VALIDATION_SPLIT, orders=orders, order_seed=seed, init_sha256=train_ref.weights_digest(ks, bs))
        cases.append(case)
        job_cases.append(dict(key=c["key"], units=c["units"], activations=c["activations"], kernels=[k.astype(np.float64).tolist() for k in ks],
                              biases=[b.astype(np.float64).tolist() for b in bs], x=x.tolist(), labels=y.tolist(), n_val=n_val, batch=c["batch"],
                              lr=c["lr"], validation_split=VALIDATION_SPLIT, orders=orders))
    job = dict(ml5=os.path.join(REF, "dist/ml5.min.js"), cases=job_cases)
    with tempfile.TemporaryDirectory() as td:
        jp, op = os.path.join(td, "job.json"), os.path.join(td, "out.json")
        json.dump(job, open(jp, "w"))
        subprocess.run(["node", os.path.join(HERE, "make_train_golden.js"), jp, op], check=True, timeout=900)
        got = json.load(open(op))
    for case, g in zip(cases, got["cases"]):
        assert g["key"] == case["key"]
        eps = []
        for e in g["epochs"]:
            ks = [np.array(k, np.float32) for k in e["kernels"]]
            eps.append(dict(loss=e["loss"], acc=e["acc"], val_loss=e["val_loss"], val_acc=e["val_acc"],
                            correct=int(round(e["acc"] * n_train)), val_correct=int(round(e["val_acc"] * n_val)),
                            kernels=[train_ref.pack(train_ref.kept(case, l, k)) for l, k in enumerate(ks)],
                            biases=[train_ref.pack(np.array(b, np.float32)) for b in e["biases"]]))
        case["epochs"] = eps
    out = dict(generator="tests/golden/gen/make_train_golden.py", node=got["node"], ml5=got["ml5"], tfjs=got["tfjs"], backend=got["backend"],
               feat=feat.tolist(), labels=lab.tolist(), in_min=in_min.tolist(), in_max=in_max.tolist(), cases=cases)
    path = os.path.join(GOLD, "train_expected.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
