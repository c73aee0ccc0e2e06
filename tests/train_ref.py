"""Float64 restatement of specification TR-1: one training run of the app's ml5 classifier as a deterministic function of
the rows, the initial weights, the learning rate, the batch size, the validation rows and one order of the training rows per epoch
(test helper).  The weights are float32 values at every step (promoted to double for the arithmetic, as classify_ref.forward does;
the update is rounded to f32 once); everything else is double.  tests/test_train_reference.py pins it to tfjs's own results
(tests/golden/train_expected.json); on the GPU machine it is the yardstick for K7."""
import base64
import hashlib

import numpy as np

EPS = 1e-7          # tfjs-layers epsilon(): categoricalCrossentropy clips to [EPS, 1 - EPS]


def normalise(feat, in_min, in_max):
    """ml5 normalizeValue in double, then the f32 tensor (as K6)."""
    return ((np.asarray(feat, np.float64) - in_min) / (np.asarray(in_max, np.float64) - in_min)).astype(np.float32).astype(np.float64)


def _act(x, a):
    if a == "relu":
        return np.maximum(x, 0.0)
    if a == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if a == "tanh":
        return np.tanh(x)
    if a == "softmax":
        m = x.max(axis=1, keepdims=True)
        return np.exp(x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))))
    return x


def _dact(y, a):
    """tfjs's gradients, from the layer's output y."""
    if a == "relu":
        return (y > 0).astype(np.float64)
    if a == "sigmoid":
        return y * (1.0 - y)
    if a == "tanh":
        return 1.0 - y * y
    return np.ones_like(y)


def forward_all(x, kernels, biases, acts):
    outs = [x]
    for k, b, a in zip(kernels, biases, acts):
        outs.append(_act(outs[-1] @ k.astype(np.float64) + b.astype(np.float64), a))
    return outs


def evaluate(p, t):
    """per-row loss, hits (argmax, first maximum on a tie), clipped-from-below mask, smallest top-two gap"""
    q = p[np.arange(len(t)), t] / p.sum(axis=1)
    loss = -np.log(np.clip(q, EPS, 1.0 - EPS))
    hit = p.argmax(axis=1) == t
    top = np.sort(p, axis=1)
    gap = float((top[:, -1] - top[:, -2]).min()) if p.shape[1] > 1 else 1.0
    return loss, hit, q < EPS, gap


AMBIGUOUS = 1e-4      # a top-two probability gap below this makes a row's hit ambiguous: ten times the 1e-5 by which K6's f32 probabilities
                      # may differ from the float64 forward (tests/test_gpu_classify.py)
FAULTS = ("last_row", "rows_past_1024", "steps_past_256", "last_unit")
LOSS_ROWS, FINISH_STEPS = 1024, 256          # the strides of the loss kernels' row loop and of the finish kernel's loop over step partials


def ambiguous_rows(p):
    """how many rows of p have a top-two probability gap below AMBIGUOUS"""
    if p.shape[1] < 2:
        return 0
    top = np.sort(p, axis=1)
    return int((top[:, -1] - top[:, -2] < AMBIGUOUS).sum())


def f32(a):
    """rounded to f32, held as double (as the weights are)"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def gradient_sums(a_l, dz, grad_dtype=np.float64):
    """dW = a_l^T dz and db = 1^T dz.  grad_dtype=np.float32: both accumulated in f32 over ascending rows, four rows at a time (the
    four products of an element are summed exactly, rounded to f32 and added to the f32 accumulator); dz holds f32 values already."""
    if grad_dtype == np.float64:
        return a_l.T @ dz, dz.sum(axis=0)
    a32 = f32(a_l)
    dw = np.zeros((a_l.shape[1], dz.shape[1]), np.float32)
    db = np.zeros(dz.shape[1], np.float32)
    for r in range(0, len(dz), 4):
        dw = dw + (a32[r:r + 4].T @ dz[r:r + 4]).astype(np.float32)
        db = db + dz[r:r + 4].sum(axis=0).astype(np.float32)
    return dw.astype(np.float64), db.astype(np.float64)


def gradient_back(dz, k, a_l, act, grad_dtype=np.float64):
    """dZ of the layer below: (dz k^T) . act'(a_l).  grad_dtype=np.float32: the product accumulated in f32 over ascending columns of dz,
    four at a time, the derivative and the result in f32."""
    if grad_dtype == np.float64:
        return (dz @ k.astype(np.float64).T) * _dact(a_l, act)
    k64 = k.astype(np.float64)
    acc = np.zeros((len(dz), k.shape[0]), np.float32)
    for c in range(0, dz.shape[1], 4):
        acc = acc + (dz[:, c:c + 4] @ k64[:, c:c + 4].T).astype(np.float32)
    return (acc * _dact(a_l.astype(np.float32), act).astype(np.float32)).astype(np.float64)


def run(x, labels, kernels, biases, acts, n_val, batch, lr, orders, clip_rule=True, own_batch_size=True, grad_dtype=np.float64, fault=None):
    """x [n][53] normalised rows, labels [n] class indices, the last n_val rows validation; orders: one sequence of n_train indices (or
    None = 0, 1, 2, ...) per epoch.  Returns a list with one dict per epoch: loss, acc, val_loss, val_acc, correct, val_correct,
    kernels, biases (f32 copies after the epoch), clipped (rows whose true-class probability was clipped from below in a step),
    min_gap (smallest top-two probability gap of any evaluation), ambiguous / val_ambiguous (rows of the steps' / the validation's
    evaluations whose top-two gap is below AMBIGUOUS: a correct f32 implementation may count those the other way).
    clip_rule=False / own_batch_size=False are the two WRONG variants the reference test must tell apart: a gradient through clipped
    rows, and means over the nominal batch size in a short last batch.
    grad_dtype=np.float32 is a model of a CORRECT f32 implementation (not of K7's code): the layer outputs stay as they are, dZ is
    rounded to f32 at every layer, dW, db and the backward product are f32 sums (gradient_sums, gradient_back).
    fault= names one WRONG variant per kernel edge (tests/test_train_shapes_reference.py): "last_row" the last row of every step passes no
    gradient; "rows_past_1024" rows 1024 and up of a step or of the validation pass are left out of the loss and hit sums and pass no
    gradient; "steps_past_256" the partials of steps 256 and up are left out of the epoch's loss and count; "last_unit" the last unit of
    every layer keeps its bias."""
    assert fault is None or fault in FAULTS
    x = np.asarray(x, np.float64)
    y = np.asarray(labels, np.int64)
    n = len(x)
    n_train = n - n_val
    ks = [np.array(k, np.float32) for k in kernels]
    bs = [np.array(b, np.float32) for b in biases]
    C = ks[-1].shape[1]
    lr64 = float(np.float32(lr))                  # tf.train.sgd keeps the rate as an f32 scalar
    b_eff = min(batch, n_train)
    out = []
    for order in orders:
        order = np.arange(n_train) if order is None else np.asarray(order, np.int64)
        loss_sum, correct, clipped, min_gap, ambiguous, val_ambiguous = 0.0, 0, 0, np.inf, 0, 0
        for s in range(0, n_train, b_eff):
            rows = order[s:s + b_eff]
            m = len(rows)
            div = m if own_batch_size else b_eff
            t = y[rows]
            a = forward_all(x[rows], ks, bs, acts)
            loss, hit, low, gap = evaluate(a[-1], t)
            ambiguous += ambiguous_rows(a[-1])
            if fault == "rows_past_1024":
                loss, hit = loss[:LOSS_ROWS], hit[:LOSS_ROWS]
            if fault != "steps_past_256" or s // b_eff < FINISH_STEPS:
                loss_sum += loss.sum() / div * m  # the batch's mean loss, weighted by the batch's size
                correct += int(hit.sum())
            clipped += int(low.sum()); min_gap = min(min_gap, gap)
            dz = a[-1].copy()
            dz[np.arange(m), t] -= 1.0
            dz /= div
            if clip_rule:
                dz[low] = 0.0                     # tfjs's clipByValue passes no gradient below its minimum
            if fault == "last_row":
                dz[m - 1] = 0.0
            if fault == "rows_past_1024":
                dz[LOSS_ROWS:] = 0.0
            if grad_dtype != np.float64:
                dz = f32(dz)
            for l in range(len(ks) - 1, -1, -1):
                dw, db = gradient_sums(a[l], dz, grad_dtype)
                if l > 0:
                    dz = gradient_back(dz, ks[l], a[l], acts[l - 1], grad_dtype)
                if fault == "last_unit":
                    db[-1] = 0.0
                ks[l] = (ks[l].astype(np.float64) - lr64 * dw).astype(np.float32)
                bs[l] = (bs[l].astype(np.float64) - lr64 * db).astype(np.float32)
        rec = dict(loss=loss_sum / n_train, acc=correct / n_train, correct=correct, clipped=clipped)
        if n_val:
            p = forward_all(x[n_train:], ks, bs, acts)[-1]
            loss, hit, _, gap = evaluate(p, y[n_train:])
            val_ambiguous = ambiguous_rows(p)
            if fault == "rows_past_1024":
                rec.update(val_loss=float(loss[:LOSS_ROWS].sum() / n_val), val_acc=float(hit[:LOSS_ROWS].sum() / n_val), val_correct=int(hit[:LOSS_ROWS].sum()))
            else:
                rec.update(val_loss=float(loss.mean()), val_acc=float(hit.mean()), val_correct=int(hit.sum()))
            min_gap = min(min_gap, gap)
        else:
            rec.update(val_loss=0.0, val_acc=0.0, val_correct=0)
        rec.update(min_gap=float(min_gap), ambiguous=ambiguous, val_ambiguous=val_ambiguous, kernels=[k.copy() for k in ks], biases=[b.copy() for b in bs])
        out.append(rec)
    return out


# ---- what the fixture's cases are made of (shared by the generator and the tests, so the fixture stays small)

def hash_init(units, salt, scale=1.0):
    """Initial weights from integer arithmetic (no random generator, no libm): w[l][i][j] = (h / 1001 - 1) * limit, h = (7919 i +
    104729 j + 1299709 l + salt) mod 2003, limit = scale * sqrt(6 / (fan_in + fan_out)); biases (h' / 1001 - 1) / 10."""
    ks, bs = [], []
    for l in range(len(units) - 1):
        i = np.arange(units[l], dtype=np.int64)[:, None]
        j = np.arange(units[l + 1], dtype=np.int64)[None, :]
        h = (7919 * i + 104729 * j + 1299709 * l + salt) % 2003
        limit = scale * np.sqrt(6.0 / (units[l] + units[l + 1]))
        ks.append(((h / 1001.0 - 1.0) * limit).astype(np.float32))
        hb = (15485863 * j[0] + 32452843 * l + salt) % 2003
        bs.append(((hb / 1001.0 - 1.0) / 10.0).astype(np.float32))
    return ks, bs


def case_weights(case):
    """The initial weights of a fixture case: hash_init, then the case's edits (a column of the first kernel forced negative with a
    negative bias: a relu unit dead for every row; the last kernel scaled and one class's output bias pushed far down: the rows of that
    class have a true-class probability below the clip)."""
    ks, bs = hash_init(case["units"], case["init"]["salt"])
    e = case["init"]
    if "dead_unit" in e:
        u = e["dead_unit"]
        ks[0][:, u] = -np.abs(ks[0][:, u]) - np.float32(0.01)
        bs[0][u] = np.float32(-1.0)
    if "last_scale" in e:
        ks[-1] = (ks[-1].astype(np.float64) * e["last_scale"]).astype(np.float32)
    if "out_bias" in e:
        bs[-1][e["out_bias"][0]] = np.float32(e["out_bias"][1])
    return ks, bs


def weights_digest(ks, bs):
    h = hashlib.sha256()
    for k, b in zip(ks, bs):
        h.update(np.ascontiguousarray(k, "<f4").tobytes()); h.update(np.ascontiguousarray(b, "<f4").tobytes())
    return h.hexdigest()


def pack(a):
    return base64.b64encode(np.ascontiguousarray(a, "<f4").tobytes()).decode()


def unpack(s, shape):
    return np.frombuffer(base64.b64decode(s), "<f4").reshape(shape).copy()


def kept(case, l, k):
    """The part of kernel l the fixture keeps: all of it, or the rows case['keep_rows'][l] names."""
    rows = case.get("keep_rows", {}).get(str(l))
    return k if rows is None else k[np.asarray(rows, np.int64)]


def separable_clusters(n_per=200, classes=4, seed=11):
    """The sanity data: `classes` well separated clusters in the 53 features, rows interleaved; (feat, labels, in_min, in_max)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1.0, 1.0, (classes, 53)) * 4.0
    lab = np.tile(np.arange(classes), n_per)
    feat = centres[lab] + rng.standard_normal((len(lab), 53)) * 0.5
    return feat, lab.astype(np.int32), feat.min(axis=0), feat.max(axis=0)


# ---- reading the fixture

def load_fixture():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_expected.json")) as f:
        return json.load(f)


def case_inputs(fx, case):
    """(feat, x normalised, labels, initial kernels, initial biases) of one fixture case"""
    feat = np.array(fx["feat"], np.float64)
    x = normalise(feat, np.array(fx["in_min"]), np.array(fx["in_max"]))
    y = (np.array(fx["labels"], np.int64) % case["classes"]).astype(np.int32)
    ks, bs = case_weights(case)
    assert weights_digest(ks, bs) == case["init_sha256"], "the initial weights are not the ones the fixture was trained from"
    return feat, x, y, ks, bs


def run_case(fx, case, orders="fixture", **kw):
    _, x, y, ks, bs = case_inputs(fx, case)
    return run(x, y, ks, bs, case["activations"], case["n_val"], case["batch"], case["lr"], case["orders"] if orders == "fixture" else orders, **kw)


def expected_epochs(case):
    """the fixture's tfjs results with the weights unpacked: kernels are the kept rows only (see kept)"""
    u = case["units"]
    out = []
    for e in case["epochs"]:
        ks = [unpack(s, (-1, u[l + 1])) for l, s in enumerate(e["kernels"])]
        bs = [unpack(s, (u[l + 1],)) for l, s in enumerate(e["biases"])]
        out.append(dict(e, kernels=ks, biases=bs))
    return out


def distance(case, got, want, keys=("loss", "val_loss")):
    """largest absolute difference in any (kept) weight or per-epoch loss between two lists of epochs; `got` holds whole kernels, `want`
    whole kernels (want_kept=False is detected by shape) or the fixture's kept rows"""
    d = 0.0
    for g, w in zip(got, want):
        for k in keys:
            d = max(d, abs(float(g[k]) - float(w[k])))
        for l in range(len(g["kernels"])):
            gk = kept(case, l, g["kernels"][l]).astype(np.float64)
            wk = w["kernels"][l] if w["kernels"][l].shape == gk.shape else kept(case, l, w["kernels"][l])
            d = max(d, float(np.abs(gk - wk.astype(np.float64)).max()), float(np.abs(g["biases"][l].astype(np.float64) - w["biases"][l].astype(np.float64)).max()))
    return d
