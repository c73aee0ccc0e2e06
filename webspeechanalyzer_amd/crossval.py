"""Cross-validating the app's models on a labelled feature DB, folds by file: the host half of specification CV-1 (K6f
and include/wsa_crossval.h are the device half, capi.FeatureDBStats.predict_classes_folds / predict_values_folds).

dbstats.evaluate, like the reference application's Predict button (src/neuralmodel.js:410), runs a model over the rows it was trained
on.  Here every file is held out once: the files are dealt to K folds (assign_folds), model k of a head trains on the rows outside
fold k (fold_data; all heads x folds as training groups, train.train_many), and every row is predicted by the model that did not see
it, in one launch per head; the predictions are then evaluated as dbstats.evaluate evaluates any others.

The rules are deterministic on purpose (no shuffling, no stratifying): files in order of first appearance, groups (a speaker, a
session; by default the file itself) in order of first appearance, group g in fold g mod K."""
import numpy as np

from . import dbstats, train

MAX_FOLDS = 32                                        # WSA_CROSSVAL_MAX_FOLDS: the K models of a head are one training group


def assign_folds(db_rows, k, group_of=None, fold_of_file=None):
    """(fold_of_row [n] i32, fold_of_file [n_files], file names) of CV-1.  db_rows: records, or a featdb.DeviceDB.  Files are numbered as
    dbstats.file_columns numbers them; a file's group is group_of(file name) (default: the file itself), groups are numbered in order of
    first appearance and group g goes to fold g mod k, so k = the number of groups leaves one group out at a time; an explicit
    fold_of_file (one fold per file, in file order) overrides both.  A row's fold is its file's; a row without a file gets -1: it is
    never held out and never predicted, and trains every fold."""
    records = getattr(db_rows, "records", db_rows)
    k = int(k)
    if not 2 <= k <= MAX_FOLDS:
        raise ValueError(f"a cross-validation has 2 .. {MAX_FOLDS} folds, got {k}")
    file_of_row, _, names = dbstats.file_columns(records)
    if fold_of_file is not None:
        fof = [int(f) for f in fold_of_file]
        if len(fof) != len(names):
            raise ValueError(f"fold_of_file has {len(fof)} entries, the DB has {len(names)} files")
        for i, f in enumerate(fof):
            if not 0 <= f < k:
                raise ValueError(f"fold_of_file[{i}] = {f} ({names[i]!r}) is outside 0 .. {k - 1}")
    else:
        groups = {}
        for name in names:
            groups.setdefault(name if group_of is None else group_of(name), len(groups))
        if k > len(groups):
            raise ValueError(f"{k} folds for {len(groups)} groups ({len(names)} files): a fold would hold nothing out")
        fof = [groups[name if group_of is None else group_of(name)] % k for name in names]
    lookup = np.array(fof + [-1], np.int32)                  # file -1 (no file) -> fold -1
    return lookup[file_of_row].astype(np.int32), fof, names


def _fold_error(f, e):
    return ValueError(f"fold {f}: {e}")


def fold_data(db, labels_or_values, classes, fold_of_row, k, stream=0):
    """One train.prepare / prepare_db (classes given) or prepare_ordinal / prepare_ordinal_db (classes None) dict per fold, from the rows
    outside it.  db: features [n][width], or a featdb.DeviceDB (the rows stay on the device).  Fold f's selection is train.select /
    select_ordinal with the labels of fold f's rows replaced by None: the `< 10` refusal (naming the fold), the balancing by the app's
    rule — whose top-up loop then cycles over training rows only — and rows that stay DB indices.  The input ranges are those of the
    fold's balanced training rows, an ordinal head's out_min / out_max those of its training values.  Every fold of a classifier gets
    ONE legend, the one select gives over the whole DB (first appearance over all rows), with y re-indexed against it: a class without
    a training row in some fold keeps its output unit, so the K models share class count, legend_to_vocab and key ranks."""
    k = int(k)
    fold_of_row = np.asarray(fold_of_row)
    n = len(labels_or_values)
    if fold_of_row.shape != (n,):
        raise ValueError(f"fold_of_row has shape {fold_of_row.shape}, there are {n} labels")
    device = hasattr(db, "ranges")
    feat = None if device else train._rows_2d(db, n, "labels" if classes is not None else "values")
    legend = train.select(labels_or_values, classes)["legend"] if classes is not None else None
    out = []
    for f in range(k):
        kept = [None if fold_of_row[i] == f else v for i, v in enumerate(labels_or_values)]
        try:
            sel = train.select(kept, classes) if classes is not None else train.select_ordinal(kept)
        except ValueError as e:
            raise _fold_error(f, e) from None
        if classes is not None:
            own = sel["legend"]
            sel = dict(sel, y=np.array([legend.index(own[j]) for j in sel["y"]], np.int32), legend=list(legend))
        if device:
            out.append(train._db_data(db, n, "labels" if classes is not None else "values", sel, stream))
        else:
            x = feat[sel["rows"]]
            out.append(dict(sel, features=x, in_min=x.min(axis=0), in_max=x.max(axis=0)))
    return out


def _true_member(record, side, name):
    pair = dbstats._pair_member(record.get("true"), side)
    return None if pair is None else pair.get(name)


def head_labels(records, name, class_list):
    """Per row the string of categorical head `name`'s true label, None where the row has none or one outside class_list (what train.select takes)."""
    known = {dbstats.js_str(c) for c in class_list}
    out = []
    for r in records:
        v = _true_member(r, 0, name)
        s = dbstats.js_str(v) if dbstats.js_truthy(v) else None
        out.append(s if s in known else None)
    return out


def head_values(records, name):
    """Per row ordinal head `name`'s true value as a float, None where the row has none (or one that is no number)."""
    out = []
    for r in records:
        v = _true_member(r, 1, name)
        x = dbstats.js_number(v) if v is not None else float("nan")
        out.append(x if x == x else None)
    return out


def cross_validate(an, db_rows, class_labels, ordinal_labels, heads, k, group_of=None, fold_of_file=None, layers=None,
                   learning_rate=train.DEFAULT_LEARNING_RATE, epochs=10, batch_size=32, validation_split=0.1, seed=0, per_file=True,
                   keep_models=False, stream=0):
    """K-fold cross-validation of the heads named in `heads` on the GPU (spec CV-1).  db_rows: rows as for dbstats.evaluate, or a
    featdb.DeviceDB of `an` (its rows stay on the device for training and for prediction).  class_labels / ordinal_labels: the app's head
    settings; k, group_of, fold_of_file: assign_folds' arguments.  layers: None (the app's default stacks), a stack for every head, or
    {head: stack}.  Fold f of every head trains with seed + 2 f (initial weights glorot_init(units, seed + 2 f), orders
    epoch_orders(.., seed + 2 f + 1)), all heads x folds as training groups (train.train_many), so its model is what train.train /
    train_regression give for fold_data's dict f and that seed.  Every row with a fold is then predicted by its fold's model (K6f, one
    launch per head) and the held-out predictions are written into the rows' `pred` pairs by update_pred_label's rule; a row without a
    fold is left blank (None).  The heads not named are evaluated on the predictions the rows hold.
    Returns dbstats.evaluate's {rows, files} plus fold_of_row, fold_of_file and folds: per fold dict(files: the held-out file names,
    held_out: its row count, heads: {head: dict(train_rows: the balanced training rows, counts: per class / bin, history)}); with
    keep_models also models {head: [nnmodel.ModelSpec per fold]}."""
    from . import capi
    cats, ords = dbstats.head_settings(class_labels, ordinal_labels)
    heads = list(heads)
    for name in heads:
        if not (any(name == c for c, _ in cats) or name in ords):
            raise ValueError(f"heads names {name!r}; the settings have {[c for c, _ in cats] + ords}")
    records = getattr(db_rows, "records", db_rows)
    device = isinstance(db_rows, capi.FeatDB)
    if device and len(records) != db_rows.count:
        raise ValueError(f"the device DB holds {db_rows.count} rows and {len(records)} records")
    if len(records) < 1:
        raise ValueError("a feature DB has at least one row")
    fold_of_row, fof, names = assign_folds(records, k, group_of, fold_of_file)
    k = int(k)
    feat = db_rows if device else np.array([r["features"] for r in records], np.float64)
    class_of = dict(cats)
    data, jobs = {}, []
    for name in heads:
        stack = layers.get(name) if isinstance(layers, dict) else layers
        if name in class_of:
            data[name] = fold_data(feat, head_labels(records, name, class_of[name]), [dbstats.js_str(c) for c in class_of[name]], fold_of_row, k, stream)
        else:
            data[name] = fold_data(feat, head_values(records, name), None, fold_of_row, k, stream)
        jobs += [dict(data=d, layers=stack, learning_rate=learning_rate, epochs=epochs, batch_size=batch_size, validation_split=validation_split,
                      seed=seed + 2 * f) for f, d in enumerate(data[name])]
    trained = train.train_many(an, jobs, stream)
    specs = {name: [trained[i * k + f][0] for f in range(k)] for i, name in enumerate(heads)}
    history = {name: [trained[i * k + f][1] for f in range(k)] for i, name in enumerate(heads)}
    legends = {name: list(data[name][0]["legend"]) for name in heads if name in class_of}
    live = []                                            # the folds' models on the device, until the evaluation has synchronised

    def members(name):
        ms = [an.load_model(s) for s in specs[name]]
        live.extend(ms)
        return ms

    predict_cat = {name: (lambda db, h, legend_to_vocab, name=name: db.predict_classes_folds(h, members(name), legend_to_vocab, stream)) for name in legends}
    predict_ord = {name: (lambda db, o, name=name: db.predict_values_folds(o, members(name), None, stream)) for name in heads if name not in class_of}
    try:
        out = dbstats.evaluate_columns(an, records, feat, 0, class_labels, ordinal_labels, legends, predict_cat, predict_ord, per_file, stream,
                                       prepare=lambda db: db.set_folds(fold_of_row, k))
    finally:
        for m in live:
            m.close()
    out["fold_of_row"], out["fold_of_file"] = fold_of_row, fof
    out["folds"] = [dict(files=[n for n, g in zip(names, fof) if g == f], held_out=int((fold_of_row == f).sum()),
                         heads={name: dict(train_rows=len(data[name][f]["rows"]), counts=list(data[name][f]["counts"]), history=history[name][f])
                                for name in heads}) for f in range(k)]
    if keep_models:
        out["models"] = specs
    return out
