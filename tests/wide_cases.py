"""K7, K6 and K8 at the row widths of output levels 11 (264 features) and 12 (23 features) (test helper), in the manner of
tests/train_cases.py: one table of cases, rows and orders from its integer hash (no random generator, no libm, no stored data), initial
weights from train_ref.hash_init.  tests/test_wide_reference.py pins the float64 restatements (train_ref.run, regress_ref.run,
classify_ref.forward: all width-generic) to tfjs on the cases of tests/golden/wide_expected.json; tests/test_gpu_wide.py runs every case
on the GPU.

n counts all rows, the last n_val are validation; every case runs 2 epochs (a permutation, then the rows in order).  `tfjs` is the
distance (train_ref.distance: any weight, any per-epoch loss) between the float64 restatement and tfjs 1.7.2's CPU backend, for the
cases the fixture holds (None: not in the fixture); d32 is D32 of the case, the distance between the restatement and its f32-gradient
variant (grad_dtype=np.float32); both measured once on the CPU and recorded here.  bound(case) = max(the family's fixture bound,
4 x D32), train_cases.bound's rule: never taken from the device.  `device` is K7's distance from the restatement on an MI355X, measured
once (DESIGN.md "At the kernels' edges").

classification (softmax output, SGD)                                              what the case reaches
  w264_one_layer  264-4         n 60  n_val 5  batch 16   kp = 272 (17 K blocks); nl == 1: the update kernel reads the gathered rows at
                                                           stride 272
  w264_stack      264-64-16-4   n 81  n_val 0  batch 17   the app's widths behind 264 inputs; steps of 17, 17, 17, 17, 13; no validation
  w23_stack       23-8-3        n 38  n_val 5  batch 16   kp = 32 with 9 padded input columns; steps of 16, 16, 1
regression (one output, Adam)
  r_w264          264-64-16-1   n 60  n_val 5  batch 16   all sigmoid: the app's ordinal stack on level-11 rows
  r_w23           23-8-1        n 60  n_val 5  batch 16   tanh then linear

FORWARD: two models for one forward pass each (K6 alone): 264-20-4 and 23-8-3 over 40 rows of clusters()."""
import functools

import numpy as np

from tests import regress_ref, train_ref
from tests.train_cases import mix, permutation, unit
from tests.test_regress_reference import BOUND as BOUND_TR2     # 6.44e-6
from tests.test_train_reference import BOUND as BOUND_TR1       # 1.82e-6

WIDTHS = (264, 23)
EPOCHS = 2


def _case(key, units, activations, n, n_val, batch, lr, salt, tfjs, d32, device):
    return dict(key=key, units=units, activations=activations, n=n, n_val=n_val, batch=batch, lr=lr, epochs=EPOCHS, salt=salt, scale=1.0,
                tfjs=tfjs, d32=d32, device=device, regression=activations[-1] != "softmax")


CASES = {c["key"]: c for c in (
    _case("w264_one_layer", [264, 4], ["softmax"], 60, 5, 16, 0.1, 11, 2.661e-8, 1.49e-8, 2.980e-8),
    _case("w264_stack", [264, 64, 16, 4], ["relu", "tanh", "softmax"], 81, 0, 17, 0.1, 11, None, 2.98e-8, 5.960e-8),
    _case("w23_stack", [23, 8, 3], ["relu", "softmax"], 38, 5, 16, 0.1, 11, 5.933e-8, 2.98e-8, 2.980e-8),
    _case("r_w264", [264, 64, 16, 1], ["sigmoid"] * 3, 60, 5, 16, 0.02, 11, None, 7.302e-7, 8.084e-7),
    _case("r_w23", [23, 8, 1], ["tanh", "linear"], 60, 5, 16, 0.01, 11, 5.960e-8, 5.96e-8, 5.960e-8),
)}
FIXTURE_KEYS = ("w264_one_layer", "w23_stack", "r_w23")            # the cases tests/golden/wide_expected.json holds tfjs's results of
FORWARD = {"f264": dict(units=[264, 20, 4], activations=["relu", "softmax"], rows=40, salt=13),
           "f23": dict(units=[23, 8, 3], activations=["tanh", "softmax"], rows=40, salt=13)}


def bound(case):
    """max(the bound of the family's fixture test, 4 x D32): from the references alone, never from the device"""
    return max(BOUND_TR2 if case["regression"] else BOUND_TR1, 4.0 * case["d32"])


def validation_split(case):
    """a validationSplit for which tfjs's own split, floor(n (1 - split)) training rows, leaves exactly n_val rows (half a row of slack)"""
    return (case["n_val"] - 0.5) / case["n"] if case["n_val"] else 0.0


def _noise(n, width, salt):
    i = np.arange(n)[:, None]
    f = np.arange(width)[None, :]
    return unit(mix(i, f, salt + 2)), 1.0 + 10.0 * (f % 5)


def cluster_rows(n, width, classes, salt):
    """train_cases.cluster_rows at any width: `classes` clusters (centres in +-4, rows within +-1 of their centre, every feature on its
    own scale), labels i % classes; (feat, labels)"""
    u, fscale = _noise(n, width, salt)
    lab = np.arange(n) % classes
    centres = unit(mix(np.arange(classes)[:, None], np.arange(width)[None, :], salt + 1)) * 4.0
    return (centres[lab] + u) * fscale, lab.astype(np.int32)


def smooth_rows(n, width, salt):
    """train_cases.smooth_rows at any width of 18 or more: a smooth target of features 3, 5, 11 and 17; the rows with the smallest and the
    largest target moved to the front and to the end; (feat, values)"""
    u, fscale = _noise(n, width, salt)
    y = 0.5 + 0.3 * (u[:, 3] - u[:, 3] ** 3 / 3.0) + 0.15 * u[:, 17] * u[:, 11] + 0.1 * u[:, 5] ** 2
    feat = u * fscale
    order = list(range(n))
    lo, hi = int(np.argmin(y)), int(np.argmax(y))
    order[0], order[lo] = order[lo], order[0]
    hi = order.index(hi)
    order[n - 1], order[hi] = order[hi], order[n - 1]
    return feat[order], y[order]


def _ranges(feat):
    span = feat.max(axis=0) - feat.min(axis=0)
    return feat.min(axis=0) - 0.05 * span, feat.max(axis=0) + 0.05 * span


@functools.lru_cache(maxsize=None)
def inputs(key):
    """train_cases.inputs for a case of this table: feat, in_min, in_max, x, kernels, biases, orders, and labels or values / out_min /
    out_max / t.  Shared between the tests: treat as read-only."""
    c = CASES[key]
    n_train = c["n"] - c["n_val"]
    if c["regression"]:
        feat, values = smooth_rows(c["n"], c["units"][0], c["salt"])
    else:
        feat, labels = cluster_rows(c["n"], c["units"][0], c["units"][-1], c["salt"])
    in_min, in_max = _ranges(feat)
    ks, bs = train_ref.hash_init(c["units"], c["salt"], c["scale"])
    orders = [None if e % 2 else permutation(n_train, c["salt"] + e) for e in range(c["epochs"])]
    out = dict(feat=feat, in_min=in_min, in_max=in_max, x=train_ref.normalise(feat, in_min, in_max), kernels=ks, biases=bs, orders=orders)
    if c["regression"]:
        out.update(values=values, out_min=float(values.min()), out_max=float(values.max()))
        out["t"] = regress_ref.normalise_target(values, out["out_min"], out["out_max"])
    else:
        out["labels"] = labels
    return out


@functools.lru_cache(maxsize=None)
def forward_inputs(name):
    """a FORWARD model and its rows: dict(feat, in_min, in_max, kernels, biases, units, activations, labels); read-only"""
    f = FORWARD[name]
    feat, _ = cluster_rows(f["rows"], f["units"][0], f["units"][-1], f["salt"])
    in_min, in_max = _ranges(feat)
    ks, bs = train_ref.hash_init(f["units"], f["salt"])
    return dict(feat=feat, in_min=in_min, in_max=in_max, kernels=ks, biases=bs, units=list(f["units"]), activations=list(f["activations"]),
                labels=[f"c{j}" for j in range(f["units"][-1])])


def restate(key, lr=None, **kw):
    """the case through its family's restatement; kw: grad_dtype="""
    c, i = CASES[key], inputs(key)
    lr = c["lr"] if lr is None else lr
    if c["regression"]:
        return regress_ref.run(i["x"], i["t"], i["kernels"], i["biases"], c["activations"], c["n_val"], c["batch"], lr, i["orders"], **kw)
    return train_ref.run(i["x"], i["labels"], i["kernels"], i["biases"], c["activations"], c["n_val"], c["batch"], lr, i["orders"], **kw)


@functools.lru_cache(maxsize=None)
def restated(key):
    """the float64 run of the case, computed once and shared: treat as read-only"""
    return restate(key)


def d32(key):
    """D32 of the case, computed fresh"""
    return train_ref.distance(CASES[key], restate(key, grad_dtype=np.float32), restated(key))
