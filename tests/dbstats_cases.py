"""Shapes, models and synthetic columns of the DS-1 / K8 tests (tests/test_gpu_dbstats.py, tests/test_dbstats_reference.py and the
fixture generator tests/golden/gen/make_dbstats_golden.py share them), as tests/train_cases.py holds K7's."""
import json
import os

import numpy as np

from webspeechanalyzer_amd import nnmodel

from . import train_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
R, MAX_CLASSES, MAX_HEADS = 256, 256, 8                         # WSA_DBSTATS_CHUNK_ROWS / _MAX_CLASSES / _MAX_HEADS
REGRESS_CASE = "a_53_16_1_sigmoid_b16"
# what tests/test_gpu_regress.py holds K6's regression values to: 1e-5 of the output range
VALUE_TOL = 1e-5

DECIDE_C = (1, 2, 4, 63, 64)
DECIDE_N = (1, 63, 64, 65, 257)
TABLE_N = (1, R - 1, R, R + 1, 2 * R + 1, 8 * R + 3)
TABLE_N_LARGE = 257 * R + 1                                     # more chunks than the chip has CUs
TABLE_V = (1, 2, 65, MAX_CLASSES)
TABLE_HEADS = ((1, 0), (0, 1), (MAX_HEADS, MAX_HEADS))


def load_fixture():
    with open(os.path.join(GOLD, "dbstats_expected.json")) as f:
        return json.load(f)


def regression_spec():
    """The regression model of fixture scenario (a): what tests/golden/regress_expected.json's case REGRESS_CASE ends with (tfjs's own
    weights after its last epoch), with the input ranges of the rows it was trained on."""
    with open(os.path.join(GOLD, "regress_expected.json")) as f:
        fx = json.load(f)
    with open(os.path.join(GOLD, fx["rows_from"])) as f:
        rows = json.load(f)
    case = next(c for c in fx["cases"] if c["key"] == REGRESS_CASE)
    u, last = case["units"], case["epochs"][-1]
    ks = [train_ref.unpack(last["kernels"][i], (u[i], u[i + 1])) for i in range(len(u) - 1)]
    bs = [train_ref.unpack(last["biases"][i], (u[i + 1],)) for i in range(len(u) - 1)]
    return nnmodel.ModelSpec(list(u), list(case["activations"]), ks, bs, np.array(rows["in_min"], np.float64), np.array(rows["in_max"], np.float64), [],
                             float(fx["out_min"]), float(fx["out_max"]))


def null_classifier_spec():
    """A classifier without softmax whose two outputs are negative for every row: the reference predicts null."""
    with open(os.path.join(GOLD, "train_expected.json")) as f:
        rows = json.load(f)
    k = np.zeros((53, 2), np.float32)
    k[3], k[17] = (-0.25, -0.5), (-0.125, -0.0625)              # normalised inputs are 0 .. 1: the outputs stay below the biases
    return nnmodel.ModelSpec([53, 2], ["linear"], [k], [np.array([-1.0, -2.0], np.float32)], np.array(rows["in_min"], np.float64),
                             np.array(rows["in_max"], np.float64), ["x", "y"])


def model_spec(name):
    if name == "cats_emotion":
        return nnmodel.load_dir(os.path.join(GOLD, "nn", "1", "cats_emotion"))
    return {"ords_V": regression_spec, "cats_null": null_classifier_spec}[name]()


def decide_table(n, C, seed):
    """(prob [n][C] f32, map [C]) with the decision's edge cases in the first rows: exact ties at the maximum (first, middle and last
    class), all zeros, all negative, one positive among negatives, a NaN beside a positive; the map permutes and drops one class."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 1.0, (n, C)).astype(np.float32)
    mid, last = C // 2, C - 1
    special = []
    for cols in ((0, mid), (mid, last), (0, last), (0, mid, last)):
        row = rng.uniform(0.0, 0.5, C).astype(np.float32)
        row[list(cols)] = np.float32(0.75)
        special.append(row)
    special.append(np.zeros(C, np.float32))
    special.append(-rng.uniform(0.1, 1.0, C).astype(np.float32))
    one = -rng.uniform(0.1, 1.0, C).astype(np.float32)
    one[last] = np.float32(1e-30)
    special.append(one)
    nan = rng.uniform(0.0, 0.5, C).astype(np.float32)
    nan[0] = np.nan
    special.append(nan)
    allnan = np.full(C, np.nan, np.float32)
    special.append(allnan)
    for i, row in enumerate(special):
        p[(i * 7) % n if n > len(special) else i % n] = row      # spread over waves where there is room; the last one wins on a clash
    m = rng.permutation(C).astype(np.int32)
    if C > 2:
        m[1] = -1
    return p, m


def table_columns(n, n_cat, n_ord, V, seed, variant="mixed"):
    """Synthetic columns: (durations [n], cats [(V, true_idx, pred_idx)], ords [(true_value, pred_value)]).  Durations span 12 orders of
    magnitude, so a sum taken in another order differs in its bits.  variant: "mixed"; "blank" (no predictions at all); "none" (no counted
    row); "late" (class V - 1 first appears in the last chunk)."""
    rng = np.random.default_rng(seed)
    dur = (10.0 ** rng.uniform(-6, 6, n)) * rng.uniform(1.0, 2.0, n)
    cats, ords = [], []
    for h in range(n_cat):
        hi = max(V - 1, 1) if variant == "late" else V
        t = rng.integers(-1, hi, n).astype(np.int32)
        p = np.where(rng.random(n) < 0.5, t, rng.integers(-1, V, n)).astype(np.int32)
        if variant == "blank":
            p[:] = -1
        if variant == "none":
            t[:] = -1
        if variant == "late" and V > 1:
            t[n - 1] = V - 1
        cats.append((V, t, p))
    for o in range(n_ord):
        t = rng.uniform(0.0, 1.0, n) * 10.0 ** rng.uniform(-3, 3, n)
        p = t + rng.normal(0, 0.1, n) * 10.0 ** rng.uniform(-3, 3, n)
        t[rng.random(n) < 0.1] = 0.0                           # true 0: does not count
        t[rng.random(n) < 0.1] = np.nan
        p[rng.random(n) < 0.1] = 0.0                           # predicted 0: counted as a sample, not as predicted
        p[rng.random(n) < 0.1] = np.nan
        if o % 2 == 1:
            t = -np.abs(t)                                     # negative-only: max stays at its start value 0
        if variant == "blank":
            p[:] = np.nan
        if variant == "none":
            t[:] = np.nan
        ords.append((t, p))
    return dur, cats, ords
