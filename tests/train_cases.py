"""The shapes at which K7's kernels (the stage bodies of csrc/train_stages.hpp, launched by csrc/train.hip and csrc/train_group.hip;
specifications TR-1 and TR-2) reach their tile, batch and width edges (test helper):
one table of cases, rows and orders made by integer arithmetic (no random generator, no libm: the same on every numpy build), initial
weights from train_ref.hash_init.  tests/test_train_shapes_reference.py proves from the float64 restatements alone that every case moves
every layer, has (nearly) no ambiguous counts and tells the wrong variants of train_ref.FAULTS apart; tests/test_gpu_train_shapes.py
runs them on the GPU.

n counts all rows, the last n_val are validation.  d32 is D32 of the case: the distance (train_ref.distance: any weight, any per-epoch
loss) between the float64 restatement and its f32-gradient variant (grad_dtype=np.float32), measured once on the CPU and recorded here;
bound(case) = max(the family's fixture bound, 4 x D32).  `device` is the distance of K7 on an MI355X from the float64 restatement,
measured once (DESIGN.md "At the kernels' edges").

classification (softmax output, SGD)                                                              what the case reaches
  one_layer     53-4                      n 60   n_val 5    batch 16    nl == 1: no backward kernel; the update reads the gathered rows
  width_edges   53-16-17-15-1-3           n 81   n_val 0    batch 17    widths of exactly 16, 17, 15 and 1; a hidden linear layer;
                                                                        n_val == 0; steps of 17, 17, 17, 17, 13
  eight_layers  53-24x7-5                 n 70   n_val 6    batch 16    the layer limit; the two dZ buffers ping-pong through 8 layers;
                                                                        steps of exactly 16
  widest        53-1024-64                n 400  n_val 40   batch 48    the width and class limits; np = 64 in the loss
  classes_33    53-40-33                  n 200  n_val 20   batch 32    np = 48 with 15 padded output columns
  big_batch     53-8-4                    n 3400 n_val 1030 batch 1100  the loss loop's second trip in steps (1100, 1100, 170) and in
                                                                        validation (1030); 69 row tiles per update owner
  batch_1       53-8-4                    n 340  n_val 40   batch 1     m = 1, mp = 16; 300 steps: the finish loop's second trip;
                                                                        n_val > batch (validation activations stale past a step's mp)
  last_of_1     53-20-3                   n 38   n_val 5    batch 16    steps of 16, 16, 1
regression (one output, Adam): the same edges through train_loss_mse_kernel and train_update_adam_kernel
  r_one_layer 53-1 | r_width_edges 53-16-17-15-1 (tanh output) | r_wide 53-1024-1 | r_relu_out 53-20-1 (relu output) |
  r_big_batch 53-64-16-1 (the app's stack) | r_batch_1 53-8-1 (600 Adam steps on the device-side accumulated betas)"""
import functools

import numpy as np

from tests import regress_ref, train_ref
from tests.test_regress_reference import BOUND as BOUND_TR2     # 6.44e-6
from tests.test_train_reference import BOUND as BOUND_TR1       # 1.82e-6

NFEAT = 53
_M32 = np.uint64(0xFFFFFFFF)


def _case(key, units, activations, n, n_val, batch, lr, epochs, salt, d32, device, scale=1.0, out_bias=None):
    return dict(key=key, units=units, activations=activations, n=n, n_val=n_val, batch=batch, lr=lr, epochs=epochs, salt=salt, scale=scale,
                out_bias=out_bias, d32=d32, device=device, regression=activations[-1] != "softmax")


CASES = {c["key"]: c for c in (
    _case("one_layer", [53, 4], ["softmax"], 60, 5, 16, 0.1, 2, 7, 2.98e-8, 4.470e-8),
    _case("width_edges", [53, 16, 17, 15, 1, 3], ["relu", "tanh", "sigmoid", "linear", "softmax"], 81, 0, 17, 0.3, 2, 7, 5.96e-8, 8.941e-8),
    _case("eight_layers", [53] + [24] * 7 + [5], ["relu", "linear", "tanh", "sigmoid", "relu", "tanh", "linear", "softmax"], 70, 6, 16, 0.3, 3, 7, 5.96e-8, 8.941e-8),
    _case("widest", [53, 1024, 64], ["relu", "softmax"], 400, 40, 48, 0.05, 2, 7, 1.453e-7, 1.417e-7, scale=4.0),
    _case("classes_33", [53, 40, 33], ["tanh", "softmax"], 200, 20, 32, 0.1, 2, 7, 1.192e-7, 1.788e-7, scale=4.0),
    _case("big_batch", [53, 8, 4], ["relu", "softmax"], 3400, 1030, 1100, 0.3, 2, 7, 5.96e-8, 5.960e-8),
    _case("batch_1", [53, 8, 4], ["sigmoid", "softmax"], 340, 40, 1, 0.05, 2, 7, 1.788e-7, 1.788e-7),
    _case("last_of_1", [53, 20, 3], ["relu", "softmax"], 38, 5, 16, 0.1, 2, 7, 1.49e-8, 2.980e-8),
    _case("r_one_layer", [53, 1], ["linear"], 60, 5, 16, 0.01, 2, 7, 1.49e-8, 5.366e-8),
    _case("r_width_edges", [53, 16, 17, 15, 1], ["relu", "tanh", "sigmoid", "tanh"], 81, 0, 17, 0.01, 2, 7, 5.96e-8, 5.960e-8),
    _case("r_wide", [53, 1024, 1], ["sigmoid", "tanh"], 200, 20, 48, 0.0015, 2, 7, 4.754e-7, 2.336e-6, scale=4.0),
    _case("r_relu_out", [53, 20, 1], ["tanh", "relu"], 60, 5, 16, 0.003, 2, 7, 2.98e-8, 5.960e-8, out_bias=0.5),
    _case("r_big_batch", [53, 64, 16, 1], ["sigmoid"] * 3, 3400, 1030, 1100, 0.02, 2, 7, 5.96e-8, 8.941e-8),
    _case("r_batch_1", [53, 8, 1], ["tanh", "linear"], 340, 40, 1, 0.002, 2, 7, 1.192e-7, 1.192e-7),
)}
TR1_KEYS = [k for k, c in CASES.items() if not c["regression"]]
TR2_KEYS = [k for k, c in CASES.items() if c["regression"]]


def bound(case):
    """max(the bound of the family's fixture test, 4 x D32): from the references alone, never from the device"""
    return max(BOUND_TR2 if case["regression"] else BOUND_TR1, 4.0 * case["d32"])


def mix(a, b, salt):
    """a 32-bit hash of two non-negative integers (arrays broadcast) in uint64 arithmetic: multiply, xor-shift, twice"""
    x = (np.asarray(a, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(b, np.uint64) * np.uint64(0x85EBCA77) + np.uint64(salt)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & _M32
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & _M32
    x ^= x >> np.uint64(15)
    return x


def unit(h):
    """a hash as a double in [-1, 1)"""
    return h.astype(np.float64) / 2147483648.0 - 1.0


def permutation(n, salt):
    return np.argsort(mix(np.arange(n), 0, salt), kind="stable").astype(np.uint32)


def _noise(n, salt):
    i = np.arange(n)[:, None]
    f = np.arange(NFEAT)[None, :]
    return unit(mix(i, f, salt + 2)), 1.0 + 10.0 * (f % 5)


def cluster_rows(n, classes, salt):
    """`classes` clusters in the 53 features (centres in +-4, rows within +-1 of their centre, every feature on its own scale), labels
    i % classes; (feat, labels)"""
    u, fscale = _noise(n, salt)
    lab = np.arange(n) % classes
    centres = unit(mix(np.arange(classes)[:, None], np.arange(NFEAT)[None, :], salt + 1)) * 4.0
    return (centres[lab] + u) * fscale, lab.astype(np.int32)


def smooth_rows(n, salt):
    """rows spread over the 53 features and a smooth (polynomial) target of four of them; the row with the smallest target is moved to
    the front (a training row) and the one with the largest to the end (a validation row if there are any): after normalising by the
    targets' own range those two are exactly 0 and 1, the only rows tfjs's binaryAccuracy can count; (feat, values)"""
    u, fscale = _noise(n, salt)
    y = 0.5 + 0.3 * (u[:, 3] - u[:, 3] ** 3 / 3.0) + 0.15 * u[:, 17] * u[:, 40] + 0.1 * u[:, 5] ** 2
    feat = u * fscale
    order = list(range(n))
    lo, hi = int(np.argmin(y)), int(np.argmax(y))
    order[0], order[lo] = order[lo], order[0]
    hi = order.index(hi)
    order[n - 1], order[hi] = order[hi], order[n - 1]
    return feat[order], y[order]


@functools.lru_cache(maxsize=None)
def inputs(key):
    """everything a run of the case takes: feat, in_min, in_max (the column extremes widened by 5 % of the range), x (normalised),
    kernels, biases, orders (a permutation, None, a permutation, ...), and labels or values / out_min / out_max / t (normalised targets).
    Shared between the tests: treat as read-only."""
    c = CASES[key]
    n_train = c["n"] - c["n_val"]
    if c["regression"]:
        feat, values = smooth_rows(c["n"], c["salt"])
    else:
        feat, labels = cluster_rows(c["n"], c["units"][-1], c["salt"])
    span = feat.max(axis=0) - feat.min(axis=0)
    in_min, in_max = feat.min(axis=0) - 0.05 * span, feat.max(axis=0) + 0.05 * span
    ks, bs = train_ref.hash_init(c["units"], c["salt"], c["scale"])
    if c["out_bias"] is not None:
        bs[-1][:] = np.float32(c["out_bias"])
    orders = [None if e % 2 else permutation(n_train, c["salt"] + e) for e in range(c["epochs"])]
    out = dict(feat=feat, in_min=in_min, in_max=in_max, x=train_ref.normalise(feat, in_min, in_max), kernels=ks, biases=bs, orders=orders)
    if c["regression"]:
        out.update(values=values, out_min=float(values.min()), out_max=float(values.max()))
        out["t"] = regress_ref.normalise_target(values, out["out_min"], out["out_max"])
    else:
        out["labels"] = labels
    return out


def restate(key, lr=None, **kw):
    """the case through its family's restatement; kw: grad_dtype=, fault="""
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
