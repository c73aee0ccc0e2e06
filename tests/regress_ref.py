"""Float64 restatement of specification TR-2: one training run of the app's ml5 REGRESSION model (ords_<label>: one output
unit, mean squared error, Adam) as a deterministic function of the rows, the real-valued targets and their range, the initial weights,
the learning rate, the batch size, the validation rows and one order of the training rows per epoch (test helper).  As in
tests/train_ref.py the weights are float32 values at every step and the gradients are double; Adam's two moments and the new weight are
rounded to f32 where tfjs rounds them (every tfjs intermediate is an f32 tensor), and its per-step scalars (the accumulated betas,
1 - accumulated beta) are the f32 chain tfjs keeps; everything else is double.  tests/test_regress_reference.py pins it to tfjs's own
results (tests/golden/regress_expected.json); on the GPU machine it is the yardstick for K7's regression kernels."""
import json
import os

import numpy as np

from tests import train_ref

F32 = np.float32
BETA1, BETA2 = F32(0.9), F32(0.999)                       # tf.train.adam's defaults, as the f32 scalars tfjs multiplies with
ONE_M_BETA1, ONE_M_BETA2 = F32(1 - 0.9), F32(1 - 0.999)   # `1 - this.beta` is a JavaScript double, then an f32 scalar
EPSILON = F32(1e-7)                                       # the CPU backend's epsilon()
LAST_ACTIVATIONS = ("linear", "relu", "sigmoid", "tanh")


def normalise_target(y, out_min, out_max):
    """ml5 normalizeData on the single output: (y - min) / (max - min) in double, then the f32 tensor."""
    return ((np.asarray(y, np.float64) - out_min) / (float(out_max) - float(out_min))).astype(np.float32).astype(np.float64)


def unnormalise(p, out_min, out_max):
    """ml5 unnormalizeValue on the f32 network output: t * (max - min) + min, JavaScript doubles, each operation rounded once."""
    return np.asarray(p, np.float32).astype(np.float64) * (float(out_max) - float(out_min)) + float(out_min)


def evaluate(p, t):
    """per-row squared error; hits of tfjs's binaryAccuracy (what "accuracy" resolves to for a one-unit output: the target equals
    1 if p > 0.5 else 0, so only rows whose normalised target is exactly 0 or 1 can ever hit); the smallest |p - 0.5| over those rows"""
    p, t = p[:, 0], np.asarray(t, np.float64)
    hit = t == (p > 0.5).astype(np.float64)
    can = (t == 0.0) | (t == 1.0)
    gap = float(np.abs(p[can] - 0.5).min()) if can.any() else 1.0
    return (p - t) ** 2, hit, gap


class Adam:
    """tfjs 1.7.2 AdamOptimizer.applyGradients, operation for operation.  bias_correction / eps_inside are WRONG variants."""

    def __init__(self, lr, shapes, bias_correction=True, eps_inside=False):
        self.neg_lr = F32(-float(lr))                     # `.mul(-this.learningRate)`: the negated double as an f32 scalar
        self.m = [np.zeros(s, F32) for s in shapes]
        self.v = [np.zeros(s, F32) for s in shapes]
        self.bias_correction, self.eps_inside = bias_correction, eps_inside
        self.reset()

    def reset(self):
        self.acc1, self.acc2 = BETA1, BETA2

    def begin(self):
        self.c1, self.c2 = F32(F32(1) - self.acc1), F32(F32(1) - self.acc2)       # sub(1, accBeta), f32
        if not self.bias_correction:
            self.c1 = self.c2 = F32(1)

    def apply(self, i, w, g):
        """w f32, g the double gradient; returns the new f32 weights"""
        d = np.float64
        m = (self.m[i].astype(d) * d(BETA1) + g * d(ONE_M_BETA1)).astype(F32)
        v = (self.v[i].astype(d) * d(BETA2) + (g * g) * d(ONE_M_BETA2)).astype(F32)
        self.m[i], self.v[i] = m, v
        mh, vh = m.astype(d) / d(self.c1), v.astype(d) / d(self.c2)
        den = np.sqrt(vh + d(EPSILON)) if self.eps_inside else np.sqrt(vh) + d(EPSILON)
        return ((mh / den) * d(self.neg_lr) + w.astype(d)).astype(F32)

    def end(self):
        self.acc1, self.acc2 = F32(self.acc1 * BETA1), F32(self.acc2 * BETA2)


def run(x, t, kernels, biases, acts, n_val, batch, lr, orders, bias_correction=True, carry_acc=True, eps_inside=False, own_batch_size=True,
        grad_dtype=np.float64, fault=None):
    """x [n][53] normalised rows, t [n] normalised targets, the last n_val rows validation; orders: one sequence of n_train indices
    (or None = 0, 1, 2, ...) per epoch.  Returns one dict per epoch: loss, acc, val_loss, val_acc, correct, val_correct, kernels, biases
    (f32 copies after the epoch), min_gap (smallest |p - 0.5| of any row that can hit, in any evaluation).
    The keyword arguments select the WRONG variants the reference test must tell apart: no bias correction, the accumulated betas
    reset at every epoch, epsilon inside the square root, means over the nominal batch size in a short last batch.
    grad_dtype=np.float32 (a model of a correct f32 implementation's gradients) and fault= (one wrong variant per kernel edge) are
    train_ref.run's."""
    assert fault is None or fault in train_ref.FAULTS
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    n = len(x)
    n_train = n - n_val
    ks = [np.array(k, np.float32) for k in kernels]
    bs = [np.array(b, np.float32) for b in biases]
    assert ks[-1].shape[1] == 1 and acts[-1] in LAST_ACTIVATIONS
    nl = len(ks)
    opt = Adam(lr, [k.shape for k in ks] + [b.shape for b in bs], bias_correction, eps_inside)
    b_eff = min(batch, n_train)
    out = []
    for order in orders:
        order = np.arange(n_train) if order is None else np.asarray(order, np.int64)
        if not carry_acc:
            opt.reset()
        loss_sum, correct, min_gap = 0.0, 0, np.inf
        for s in range(0, n_train, b_eff):
            rows = order[s:s + b_eff]
            m = len(rows)
            div = m if own_batch_size else b_eff
            a = train_ref.forward_all(x[rows], ks, bs, acts)
            se, hit, gap = evaluate(a[-1], t[rows])
            if fault == "rows_past_1024":
                se, hit = se[:train_ref.LOSS_ROWS], hit[:train_ref.LOSS_ROWS]
            if fault != "steps_past_256" or s // b_eff < train_ref.FINISH_STEPS:
                loss_sum += se.sum() / div * m        # the batch's mean loss, weighted by the batch's size
                correct += int(hit.sum())
            min_gap = min(min_gap, gap)
            dz = (2.0 * (a[-1][:, 0] - t[rows]) / div)[:, None] * train_ref._dact(a[-1], acts[-1])
            if fault == "last_row":
                dz[m - 1] = 0.0
            if fault == "rows_past_1024":
                dz[train_ref.LOSS_ROWS:] = 0.0
            if grad_dtype != np.float64:
                dz = train_ref.f32(dz)
            opt.begin()
            for l in range(nl - 1, -1, -1):
                dw, db = train_ref.gradient_sums(a[l], dz, grad_dtype)
                if l > 0:
                    dz = train_ref.gradient_back(dz, ks[l], a[l], acts[l - 1], grad_dtype)
                kept_bias = bs[l][-1]
                ks[l] = opt.apply(l, ks[l], dw)
                bs[l] = opt.apply(nl + l, bs[l], db)
                if fault == "last_unit":
                    bs[l][-1] = kept_bias
            opt.end()
        rec = dict(loss=loss_sum / n_train, acc=correct / n_train, correct=correct)
        if n_val:
            se, hit, gap = evaluate(train_ref.forward_all(x[n_train:], ks, bs, acts)[-1], t[n_train:])
            if fault == "rows_past_1024":
                se[train_ref.LOSS_ROWS:], hit[train_ref.LOSS_ROWS:] = 0.0, False
            rec.update(val_loss=float(se.mean()), val_acc=float(hit.mean()), val_correct=int(hit.sum()))
            min_gap = min(min_gap, gap)
        else:
            rec.update(val_loss=0.0, val_acc=0.0, val_correct=0)
        rec.update(min_gap=float(min_gap), kernels=[k.copy() for k in ks], biases=[b.copy() for b in bs])
        out.append(rec)
    return out


def predict(feat, kernels, biases, acts, in_min, in_max, out_min, out_max):
    """the float64 forward (classify_ref's: f32 inputs and weights, double arithmetic) and ml5's un-normalise; (p, value)"""
    x = train_ref.normalise(feat, np.asarray(in_min, np.float64), np.asarray(in_max, np.float64))
    p = train_ref.forward_all(x, [np.asarray(k, np.float32) for k in kernels], [np.asarray(b, np.float32) for b in biases], acts)[-1][:, 0]
    return p, p * (float(out_max) - float(out_min)) + float(out_min)


def smooth_target(n=800, seed=5):
    """The sanity data: a smooth function of three of the 53 features; (feat, values, in_min, in_max)."""
    rng = np.random.default_rng(seed)
    feat = rng.uniform(-1.0, 1.0, (n, 53)) * np.round(10.0 ** rng.uniform(0, 2, 53), 0)
    u = feat / np.abs(feat).max(axis=0)
    y = 0.5 + 0.3 * np.sin(2.0 * u[:, 3]) + 0.15 * u[:, 17] * u[:, 40]
    return feat, y, feat.min(axis=0), feat.max(axis=0)


# ---- reading the fixture

def load_fixture():
    """regress_expected.json with the 50 feature rows and their ranges taken from the file it names (train_expected.json)."""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(gold, "regress_expected.json")) as f:
        fx = json.load(f)
    with open(os.path.join(gold, fx["rows_from"])) as f:
        rows = json.load(f)
    fx.update(feat=rows["feat"], in_min=rows["in_min"], in_max=rows["in_max"])
    return fx


def case_inputs(fx, case):
    """(feat, x normalised, values, t normalised, initial kernels, initial biases) of one fixture case"""
    feat = np.array(fx["feat"], np.float64)
    x = train_ref.normalise(feat, np.array(fx["in_min"]), np.array(fx["in_max"]))
    y = np.array(fx["values"], np.float64)
    ks, bs = train_ref.case_weights(case)
    assert train_ref.weights_digest(ks, bs) == case["init_sha256"], "the initial weights are not the ones the fixture was trained from"
    return feat, x, y, normalise_target(y, fx["out_min"], fx["out_max"]), ks, bs


def run_case(fx, case, orders="fixture", raw_targets=False, **kw):
    """raw_targets=True is a WRONG variant: the targets are not normalised."""
    _, x, y, t, ks, bs = case_inputs(fx, case)
    return run(x, y if raw_targets else t, ks, bs, case["activations"], case["n_val"], case["batch"], case["lr"],
               case["orders"] if orders == "fixture" else orders, **kw)
