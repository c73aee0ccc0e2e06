"""Training the app's syllable classifiers (specification TR-1, K7): what src/neuralmodel.js:163-403 (train_nn) does around
ml5.neuralNetwork(...).train — selecting and balancing the stored level-13 rows, the input ranges, the initial weights and the
per-epoch orders (both from numpy's generator: the reference draws them from Math.random, so they are ours) — and the epochs on the
GPU through capi.Trainer.  Classification only: the regression models (ords_*) and the '*' wildcard class are not supported.
(That holds for prepare / stack / train.  The regression models have their own entry points below, specification TR-2:
prepare_ordinal and train_regression.  train_many runs several of either kind at once as a training group, specification TG-1.)"""
import math

import numpy as np

from . import nnmodel

DEFAULT_LAYERS = [{"type": "dense", "units": 8, "activation": "relu"}, {"type": "dense", "activation": "softmax"}]   # src/neuralmodel_aux.js:106-124
DEFAULT_LEARNING_RATE = 0.2
# nn_default_options_ords, src/neuralmodel_aux.js:127-150 (task "regression", learningRate 0.2)
DEFAULT_LAYERS_ORDS = [{"type": "dense", "units": 64, "activation": "sigmoid"}, {"type": "dense", "units": 16, "activation": "sigmoid"},
                       {"type": "dense", "activation": "sigmoid"}]
ORDINAL_RANGES = (0.25, 0.5, 0.75, 1.0)              # neuralmodel.js:281: the bins the ordinal values are balanced over


def _rows_2d(features, n_labels, what):
    """features as [n][width] f64, width the row width of an ML level (nnmodel.WIDTHS), one label / value per row"""
    feat = np.asarray(features, np.float64)
    if feat.ndim != 2 or feat.shape[1] not in nnmodel.WIDTHS or n_labels != len(feat):
        raise ValueError(f"features {feat.shape} / {n_labels} {what}: expected [n][{nnmodel.NFEAT}] (or [n][264] at output_level 11, [n][23] at 12) and n {what}")
    return feat


def select(labels, classes):
    """The label-only half of prepare: which DB rows train_nn adds, in which order (neuralmodel.js:216-264).  labels: per row the label's
    value or None; classes: the label's class list.  Returns dict(rows, y, legend, counts) as prepare describes them; nothing here reads a
    feature, so the same selection serves host rows (prepare) and a device DB (prepare_db)."""
    classes = [str(c) for c in classes]
    if "*" in classes:
        raise ValueError("the '*' wildcard class is not supported")
    n = len(labels)
    cls = [classes.index(str(v)) if v is not None and str(v) in classes else -1 for v in labels]
    rows = [i for i, c in enumerate(cls) if c >= 0]
    count = [sum(1 for i in rows if cls[i] == c) for c in range(len(classes))]
    if len(rows) < 10:
        raise ValueError(f"Sample size {len(rows)}/{n} too small for training")
    max_n = max(count)
    for c in range(len(classes)):
        while 3 < count[c] < max_n:
            for i in range(n):
                if cls[i] == c and count[c] < max_n:
                    rows.append(i); count[c] += 1
                if count[c] >= max_n:
                    break
    legend = []
    for i in rows:
        if classes[cls[i]] not in legend:
            legend.append(classes[cls[i]])
    y = np.array([legend.index(classes[cls[i]]) for i in rows], np.int32)
    return dict(rows=rows, y=y, legend=legend, counts=count)


def prepare(features, labels, classes):
    """The selection and balancing loop of neuralmodel.js:216-264.  features [n][53] (or 264 / 23 wide: the rows of level 11 / 12); labels: per row the label's value or None;
    classes: the label's class list.  Rows whose label is one of `classes` are added in DB order; fewer than 10 of them is refused;
    then each class with more than 3 and fewer than the largest count is topped up by cycling through the DB in order until it
    reaches that count.  Returns dict(features, y, legend, in_min, in_max, counts, rows): y are indices into legend, which lists the
    labels in order of first appearance (ml5's uniqueValues); in_min / in_max are taken over the balanced set, duplicates included
    (ml5 normalizeData); rows are the DB indices in the order added."""
    if "*" in [str(c) for c in classes]:
        raise ValueError("the '*' wildcard class is not supported")
    feat = _rows_2d(features, len(labels), "labels")
    sel = select(labels, classes)
    x = feat[sel["rows"]]
    return dict(features=x, y=sel["y"], legend=sel["legend"], in_min=x.min(axis=0), in_max=x.max(axis=0), counts=sel["counts"], rows=sel["rows"])


def _db_data(db, n_labels, what, sel, stream):
    """sel with the DB and the ranges of its selected rows in place of host features (wsa_featdb_ranges)"""
    if n_labels != db.count:
        raise ValueError(f"{n_labels} {what} for a device DB of {db.count} rows")
    in_min, in_max = db.ranges(sel["rows"], stream)
    return dict(sel, db=db, in_min=in_min, in_max=in_max)


def prepare_db(db, labels, classes, stream=0):
    """prepare over a featdb.DeviceDB: the same selection, the features left on the device.  Returns dict(db, rows, y, legend, in_min,
    in_max, counts); train and train_many take it where they take prepare's."""
    return _db_data(db, len(labels), "labels", select(labels, classes), stream)


def glorot_init(units, seed):
    """tfjs's default Dense initialisers with numpy's generator: kernels truncated normal (redrawn beyond two standard deviations) with
    standard deviation sqrt(2 / (fan_in + fan_out)), zero biases."""
    rng = np.random.default_rng(seed)
    ks, bs = [], []
    for i in range(len(units) - 1):
        std = math.sqrt(2.0 / (units[i] + units[i + 1]))
        w = rng.standard_normal((units[i], units[i + 1]))
        while True:
            bad = np.abs(w) > 2.0
            if not bad.any():
                break
            w[bad] = rng.standard_normal(int(bad.sum()))
        ks.append((w * std).astype(np.float32)); bs.append(np.zeros(units[i + 1], np.float32))
    return ks, bs


def epoch_orders(n_train, epochs, seed):
    """One permutation of the training rows per epoch (tfjs shuffles the training indices every epoch)."""
    rng = np.random.default_rng(seed)
    return [rng.permutation(n_train).astype(np.uint32) for _ in range(epochs)]


def split(n, validation_split=0.1):
    """(n_train, n_val) as tfjs's fit splits: the last n - floor(n (1 - validationSplit)) rows are validation."""
    n_train = int(math.floor(n * (1 - validation_split)))
    return n_train, n - n_train


def stack(layers, n_classes, n_inputs=nnmodel.NFEAT):
    """(units, activations) of the app's options JSON `layers`; the last layer's units are the number of classes; n_inputs the width of
    the rows (ml5 infers it from them)."""
    units, acts = [int(n_inputs)], []
    for i, l in enumerate(layers):
        if l.get("type", "dense") != "dense":
            raise ValueError(f"layer {i} is {l.get('type')!r}; only dense layers are supported")
        units.append(n_classes if i == len(layers) - 1 else int(l["units"]))
        acts.append(l.get("activation", "linear"))
    if acts[-1] != "softmax":
        raise ValueError("training needs a softmax output layer")
    return units, acts


def _width(data):
    """the row width of prepare's or prepare_db's data"""
    return data["db"].width if "db" in data else np.shape(data["features"])[1]


def _trainer(an, data, layers, learning_rate, epochs, batch_size, validation_split, seed, init, orders):
    """(capi.Trainer, orders) of train's arguments"""
    units, acts = stack(layers or DEFAULT_LAYERS, len(data["legend"]), _width(data))
    ks, bs = init if init is not None else glorot_init(units, seed)
    n_train, n_val = split(len(data["rows"]) if "db" in data else len(data["features"]), validation_split)
    orders = orders if orders is not None else epoch_orders(n_train, epochs, seed + 1)
    spec = nnmodel.ModelSpec(units, acts, ks, bs, np.asarray(data["in_min"], np.float64), np.asarray(data["in_max"], np.float64), list(data["legend"]))
    if "db" in data:
        tr = data["db"].trainer(spec, data["rows"], data["y"], n_val, batch_size, learning_rate)
    else:
        tr = an.trainer(spec, data["features"], data["y"], n_val, batch_size, learning_rate)
    return tr, orders


def train(an, data, layers=None, learning_rate=DEFAULT_LEARNING_RATE, epochs=10, batch_size=32, validation_split=0.1, seed=0,
          init=None, orders=None, on_epoch=None, stream=0):
    """Trains on `an` (a capi.Analyzer) over data = prepare(...) or prepare_db(...) (a DeviceDB of `an`; its rows stay on the device).  init: (kernels, biases) instead of glorot_init(units, seed); orders:
    one order per epoch instead of epoch_orders(n_train, epochs, seed + 1).  on_epoch(epoch, stats) mirrors ml5's whileTraining (it
    synchronises every epoch; without it only the last epoch is waited for).  Returns (nnmodel.ModelSpec, history)."""
    tr, orders = _trainer(an, data, layers, learning_rate, epochs, batch_size, validation_split, seed, init, orders)
    try:
        history = []
        for e in range(epochs):
            tr.epoch(orders[e], stream)
            if on_epoch is not None or e == epochs - 1:
                st = tr.stats(stream)
                history.append(st)
                if on_epoch is not None:
                    on_epoch(e, st)
        return tr.spec_now(stream), history
    finally:
        tr.close()


def select_ordinal(values):
    """The label-only half of prepare_ordinal (neuralmodel.js:278-332): dict(rows, values, out_min, out_max, counts) as it describes them."""
    n = len(values)
    nb = len(ORDINAL_RANGES)

    def bin_of(v):
        if v is None:
            return -1
        b = 0
        while b < nb and not float(v) <= ORDINAL_RANGES[b]:
            b += 1
        return b if b < nb else -1

    bins = [bin_of(v) for v in values]
    rows = [i for i, b in enumerate(bins) if b >= 0]
    count = [sum(1 for i in rows if bins[i] == b) for b in range(nb)]
    if len(rows) < 10:
        raise ValueError(f"Sample size {len(rows)}/{n} too small for training")
    max_n = max(count)
    if max_n > 3:
        for b in range(nb):
            while 3 < count[b] < max_n:
                for i in range(n):
                    if bins[i] == b and count[b] < max_n:
                        rows.append(i); count[b] += 1
                    if count[b] >= max_n:
                        break
    y = np.array([float(values[i]) for i in rows], np.float64)
    return dict(rows=rows, values=y, out_min=float(y.min()), out_max=float(y.max()), counts=count)


def prepare_ordinal(features, values):
    """The selection and balancing loop of neuralmodel.js:278-332 for an ordinal label (V, A or D).  features [n][53] (or 264 / 23 wide); values: per row
    the label's value or None.  A row's bin is the first of (-inf, 0.25], (0.25, 0.5], (0.5, 0.75], (0.75, 1.0] that holds its value; rows
    with None or a value above 1.0 are dropped; the others are added in DB order; fewer than 10 of them is refused; then, only when the
    largest bin holds more than 3, each bin with more than 3 and fewer than the largest count is topped up by cycling through the DB in
    order until it reaches that count.  Returns dict(features, values, in_min, in_max, out_min, out_max, counts, rows): the ranges are
    taken over the balanced set, duplicates included (ml5 normalizeData); rows are the DB indices in the order added."""
    feat = _rows_2d(features, len(values), "values")
    sel = select_ordinal(values)
    x = feat[sel["rows"]]
    return dict(features=x, values=sel["values"], in_min=x.min(axis=0), in_max=x.max(axis=0), out_min=sel["out_min"], out_max=sel["out_max"],
                counts=sel["counts"], rows=sel["rows"])


def prepare_ordinal_db(db, values, stream=0):
    """prepare_ordinal over a featdb.DeviceDB: dict(db, rows, values, in_min, in_max, out_min, out_max, counts); train_regression and
    train_many take it where they take prepare_ordinal's."""
    return _db_data(db, len(values), "values", select_ordinal(values), stream)


def stack_regression(layers, n_inputs=nnmodel.NFEAT):
    """(units, activations) of the app's options JSON `layers` for a regression task: the last layer has one unit and is not softmax;
    n_inputs the width of the rows."""
    units, acts = [int(n_inputs)], []
    for i, l in enumerate(layers):
        if l.get("type", "dense") != "dense":
            raise ValueError(f"layer {i} is {l.get('type')!r}; only dense layers are supported")
        units.append(1 if i == len(layers) - 1 else int(l["units"]))
        acts.append(l.get("activation", "linear"))
    if acts[-1] not in ("linear", "relu", "sigmoid", "tanh"):
        raise ValueError(f"a regression model's last layer is linear, relu, sigmoid or tanh, not {acts[-1]}")
    return units, acts


def _regress_trainer(an, data, layers, learning_rate, epochs, batch_size, validation_split, seed, init, orders):
    """(capi.Trainer, orders) of train_regression's arguments"""
    units, acts = stack_regression(layers or DEFAULT_LAYERS_ORDS, _width(data))
    ks, bs = init if init is not None else glorot_init(units, seed)
    n_train, n_val = split(len(data["rows"]) if "db" in data else len(data["features"]), validation_split)
    orders = orders if orders is not None else epoch_orders(n_train, epochs, seed + 1)
    spec = nnmodel.ModelSpec(units, acts, ks, bs, np.asarray(data["in_min"], np.float64), np.asarray(data["in_max"], np.float64), [],
                             float(data["out_min"]), float(data["out_max"]))
    if "db" in data:
        tr = data["db"].regress_trainer(spec, data["rows"], data["values"], n_val, batch_size, learning_rate)
    else:
        tr = an.regress_trainer(spec, data["features"], data["values"], n_val, batch_size, learning_rate)
    return tr, orders


def train_regression(an, data, layers=None, learning_rate=DEFAULT_LEARNING_RATE, epochs=10, batch_size=32, validation_split=0.1, seed=0,
                     init=None, orders=None, on_epoch=None, stream=0):
    """train(...) for a regression model (specification TR-2) over data = prepare_ordinal(...): the app's nn_default_options_ords stack
    unless `layers` is given, Adam on the mean squared error of the normalised output.  Returns (nnmodel.ModelSpec with out_min /
    out_max, history)."""
    tr, orders = _regress_trainer(an, data, layers, learning_rate, epochs, batch_size, validation_split, seed, init, orders)
    try:
        history = []
        for e in range(epochs):
            tr.epoch(orders[e], stream)
            if on_epoch is not None or e == epochs - 1:
                st = tr.stats(stream)
                history.append(st)
                if on_epoch is not None:
                    on_epoch(e, st)
        return tr.spec_now(stream), history
    finally:
        tr.close()


_JOB_DEFAULTS = dict(layers=None, learning_rate=DEFAULT_LEARNING_RATE, epochs=10, batch_size=32, validation_split=0.1, seed=0, init=None,
                     orders=None, on_epoch=None)


def train_many(an, jobs, stream=0):
    """train / train_regression for several models at once (specification TG-1, K7g): jobs are dicts with those functions' arguments
    (data, layers, learning_rate, epochs, batch_size, validation_split, seed, init, orders, on_epoch); data from prepare_ordinal
    (it has "values") makes the job a regression model's.  The jobs' trainers step in lock step as one capi.TrainGroup, one launch per
    stage for all of them; a job with fewer epochs stops stepping (the group is re-formed from the rest); more than 32 jobs run as
    consecutive groups of 32.  Returns, in job order, exactly what train / train_regression return for the same arguments."""
    from . import capi
    out = [None] * len(jobs)
    for first in range(0, len(jobs), capi.TRAIN_GROUP_MAX):
        part = range(first, min(first + capi.TRAIN_GROUP_MAX, len(jobs)))
        runs = []                                       # per job of the part: index, arguments, trainer, orders, history
        try:
            for j in part:
                unknown = set(jobs[j]) - set(_JOB_DEFAULTS) - {"data"}
                if unknown or "data" not in jobs[j]:
                    raise ValueError(f"job {j}: " + (f"unknown arguments {sorted(unknown)}" if unknown else "no data"))
                a = dict(_JOB_DEFAULTS, **jobs[j])
                make = _regress_trainer if "values" in a["data"] else _trainer
                tr, orders = make(an, a["data"], a["layers"], a["learning_rate"], a["epochs"], a["batch_size"], a["validation_split"],
                                  a["seed"], a["init"], a["orders"])
                runs.append(dict(j=j, a=a, tr=tr, orders=orders, history=[]))
            e = 0
            while True:
                live = [r for r in runs if r["a"]["epochs"] > e]
                if not live:
                    break
                until = min(r["a"]["epochs"] for r in live)             # the members are the same up to this epoch
                group = an.train_group([r["tr"] for r in live])
                try:
                    for e in range(e, until):
                        group.epoch([r["orders"][e] for r in live], stream)
                        want = [r["a"]["on_epoch"] is not None or e == r["a"]["epochs"] - 1 for r in live]
                        if any(want):
                            for r, w, st in zip(live, want, group.stats(stream)):
                                if w:
                                    r["history"].append(st)
                                    if r["a"]["on_epoch"] is not None:
                                        r["a"]["on_epoch"](e, st)
                finally:
                    group.close()
                e = until
            for r in runs:
                out[r["j"]] = (r["tr"].spec_now(stream), r["history"])
        finally:
            for r in runs:
                r["tr"].close()
    return out
