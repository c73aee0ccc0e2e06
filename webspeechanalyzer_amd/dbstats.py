"""Predicting a labelled feature DB and the app's results table: the host half of specification DS-1 (K8 is the device
half, capi.FeatureDBStats).  What the reference application's Predict button does around its models: src/neuralmodel.js:410-535
(predict_db_nn -> nn_db_results_handler), src/localstore.js:723-769 (update_pred_label) and :498-627 (shows_stats_table).

A DB is a list of rows {file, seg, time, features, true, pred} as js/featuredb.js exports them (`true` / `pred`: None or a pair
[categorical {name: value}, ordinal {name: value}]).  The head settings are the app's: class_labels, a list of one-key objects
{name: [classes]}, and ordinal_labels, a list of names.  Everything that is a string is resolved here (vocabularies, the class-list and
'*' rule, truthiness of labels); the device sees indices and values and applies the numeric rules itself.

Where this differs from the reference, on purpose: labels are compared AS STRINGS (String(3) == "3": the reference's loose == between a
true and a predicted label agrees on numbers and their decimal strings; its strict indexOf for first appearance would list 3 and "3"
as two classes that share one counter, which nothing here reproduces); ordinal values go through Number(), so the truthy string "0" does
not count; a row whose `true` pair lacks a member is treated as without that label (the reference throws)."""
import math
import re
from decimal import ROUND_HALF_UP, Decimal

import numpy as np

MAX_CLASSES, MAX_HEADS, CHUNK_ROWS = 256, 8, 256      # WSA_DBSTATS_MAX_CLASSES / _MAX_HEADS / _CHUNK_ROWS
MANY_CLASSES = 25                                     # localstore.js:560, 564: from 25 classes up the list prints as "Many"


# ---- JavaScript's view of a JSON value
def js_truthy(v):
    if v is None or v is False:
        return False
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return not (v == 0 or v != v)
    if isinstance(v, str):
        return v != ""
    return True


def js_number_str(x):
    """Number.prototype.toString: the shortest digits that round-trip (Python's repr finds the same ones), in JS's layout."""
    x = float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    if x == 0:
        return "0"
    sign, x = ("-", -x) if x < 0 else ("", x)
    mant, _, exp = repr(x).partition("e")
    ip, _, fp = mant.partition(".")
    fp = "" if fp == "0" else fp
    e = int(exp) if exp else 0
    digits = (ip + fp).lstrip("0")
    n = len(ip) + e if ip != "0" else e - (len(fp) - len(fp.lstrip("0")))       # value = 0.digits x 10^n
    digits = digits.rstrip("0") or "0"
    k = len(digits)
    if k <= n <= 21:
        return sign + digits + "0" * (n - k)
    if 0 < n <= 21:
        return sign + digits[:n] + "." + digits[n:]
    if -6 < n <= 0:
        return sign + "0." + "0" * (-n) + digits
    ee = n - 1
    return sign + digits[0] + ("." + digits[1:] if k > 1 else "") + "e" + ("+" if ee >= 0 else "-") + str(abs(ee))


def js_str(v):
    """String(v) of a label value."""
    if isinstance(v, str):
        return v
    if v is True:
        return "true"
    if v is False:
        return "false"
    if v is None:
        return "null"
    if isinstance(v, (int, float)):
        return js_number_str(v)
    return str(v)


def js_number(v):
    """Number(v) for the values an ordinal label can hold; None stays missing (NaN)."""
    if isinstance(v, bool):
        return 1.0 if v else 0.0
    if isinstance(v, (int, float)):
        return float(v)
    if isinstance(v, str):
        s = v.strip()
        if s == "":
            return 0.0
        try:
            return float(s) if re.fullmatch(r"[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|Infinity)", s) else math.nan
        except ValueError:
            return math.nan
    return math.nan


def parse_float(v):
    """parseFloat(v): the longest numeric prefix of String(v), NaN without one (localstore.js:534 on time[1])."""
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        return float(v)
    m = re.match(r"\s*([+-]?(?:Infinity|\d+\.?\d*(?:[eE][+-]?\d+)?|\.\d+(?:[eE][+-]?\d+)?))", js_str(v))
    return float(m.group(1).replace("Infinity", "inf")) if m else math.nan


def to_fixed(x, digits):
    """Number.prototype.toFixed: the n for which n / 10^digits - x is closest to zero on the EXACT binary value of x, the larger n on a
    tie (as tests/classify_ref does for timestamps; '%.2f' would round half to even)."""
    x = float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    if abs(x) >= 1e21:
        return js_number_str(x)
    q = Decimal(1).scaleb(-digits)
    d = Decimal(abs(x)).quantize(q, rounding=ROUND_HALF_UP)
    neg = x < 0 and d != 0
    if x < 0 and d == 0:
        neg = True                                   # (-0.001).toFixed(2) is "-0.00"
    if x == 0:
        neg = False
    return ("-" if neg else "") + format(d, "f")


def _strict_in(value, class_list):
    """Array.prototype.indexOf(value) >= 0: strict equality, so 3 is not "3"."""
    for c in class_list:
        if isinstance(value, str) != isinstance(c, str) or isinstance(value, bool) != isinstance(c, bool):
            continue
        if value == c:
            return True
    return False


def head_settings(class_labels, ordinal_labels):
    """([(name, class list)], [names]) of the app's two settings (check_label_heads, localstore.js:222-248)."""
    cats = []
    for h in class_labels or []:
        if not isinstance(h, dict) or len(h) < 1:
            raise ValueError(f"class_labels holds one-key objects {{name: [classes]}}, got {h!r}")
        name = next(iter(h))
        cats.append((name, list(h[name])))
    ords = [str(n) for n in (ordinal_labels or [])]
    if len(cats) > MAX_HEADS:
        raise ValueError(f"{len(cats)} categorical heads (limit {MAX_HEADS})")
    if len(ords) > MAX_HEADS:
        raise ValueError(f"{len(ords)} ordinal heads (limit {MAX_HEADS})")
    return cats, ords


def _pair_member(pair, side):
    if not js_truthy(pair) or not isinstance(pair, (list, tuple)) or len(pair) <= side or not isinstance(pair[side], dict):
        return None
    return pair[side]


def build_columns(db_rows, class_labels, ordinal_labels, legends=None):
    """The index and value columns K8 counts.  legends: {head name: the model's legend labels}, added to that head's vocabulary behind
    the labels found in the rows.  Returns dict(durations [n] f64, cats [dict(name, vocab, true_idx, pred_idx)], ords [dict(name,
    true_value, pred_value)]); vocab holds the labels as strings."""
    cats, ords = head_settings(class_labels, ordinal_labels)
    n = len(db_rows)
    if n < 1:
        raise ValueError("a feature DB has at least one row")
    out = dict(durations=np.array([parse_float(r["time"][1]) for r in db_rows], np.float64), cats=[], ords=[])
    for name, class_list in cats:
        vocab, index = [], {}

        def slot(label):
            key = js_str(label)
            if key not in index:
                index[key] = len(vocab)
                vocab.append(key)
            return index[key]

        wildcard = _strict_in("*", class_list)
        t_idx, p_idx = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        for i, r in enumerate(db_rows):
            t = _pair_member(r.get("true"), 0)
            v = t.get(name) if t is not None else None
            if js_truthy(v) and (wildcard or _strict_in(v, class_list)):                     # localstore.js:523
                t_idx[i] = slot(v)
        for label in (legends or {}).get(name, []):
            slot(label)
        for i, r in enumerate(db_rows):
            p = _pair_member(r.get("pred"), 0)
            v = p.get(name) if p is not None else None
            if js_truthy(v):                                                                 # localstore.js:537
                p_idx[i] = slot(v)
        if len(vocab) > MAX_CLASSES:
            raise ValueError(f"head {name!r} has {len(vocab)} distinct labels (limit {MAX_CLASSES})")
        out["cats"].append(dict(name=name, vocab=vocab or [""], true_idx=t_idx, pred_idx=p_idx))
    for name in ords:
        t_val, p_val = np.full(n, np.nan), np.full(n, np.nan)
        for i, r in enumerate(db_rows):
            t, p = _pair_member(r.get("true"), 1), _pair_member(r.get("pred"), 1)
            if t is not None and t.get(name) is not None:
                t_val[i] = js_number(t[name])
            if p is not None and p.get(name) is not None:
                p_val[i] = js_number(p[name])
        out["ords"].append(dict(name=name, true_value=t_val, pred_value=p_val))
    return out


def assemble_table(columns, cat, cls, ords):
    """The table as plain data from K8's counters (capi.FeatureDBStats.table, or the restatement's): classes in order of first appearance
    among the counted rows (ascending first_row), classes never counted left out."""
    table, off = dict(cats=[], ords=[]), 0
    for h, col in enumerate(columns["cats"]):
        V = len(col["vocab"])
        seen = sorted((int(cls["first_row"][off + v]), v) for v in range(V) if int(cls["count"][off + v]) > 0)
        table["cats"].append(dict(
            name=col["name"], correct=int(cat["correct"][h]), wrong=int(cat["wrong"][h]), blank=int(cat["blank"][h]),
            classes=[dict(label=col["vocab"][v], count=int(cls["count"][off + v]), duration=float(cls["duration"][off + v]),
                          correct=int(cls["correct"][off + v]), wrong=int(cls["wrong"][off + v])) for _, v in seen]))
        off += V
    for o, col in enumerate(columns["ords"]):
        pred_n, sq = int(ords["pred_n"][o]), float(ords["sq_sum"][o])
        table["ords"].append(dict(name=col["name"], min=float(ords["min"][o]), max=float(ords["max"][o]), true_n=int(ords["true_n"][o]),
                                  pred_n=pred_n, sq_sum=sq, rmse=math.sqrt(sq / pred_n if pred_n > 0 else 0.0)))   # localstore.js:602-603
    return table


def _percent(correct, wrong):
    return to_fixed(correct * 100 / (correct + wrong) if correct + wrong else math.nan, 2)


def stats_lines(table):
    """The text of the app's results panel, one item per <li> in its order, tags stripped and white space collapsed (localstore.js:558-610;
    the "Stats generated at" line is left out)."""
    lines = []
    for h in table["cats"]:
        k = len(h["classes"])
        lines.append(f"Label: {h['name']}, Type: Class")
        lines.append(f"Classes ({k}): " + (",".join(c["label"] for c in h["classes"]) if k < MANY_CLASSES else "Many"))
        lines.append(f"Accuracy: {_percent(h['correct'], h['wrong'])}%")
        lines.append(f"Correct: {h['correct']}, Wrong {h['wrong']}, NaN: {h['blank']}")
        if k < MANY_CLASSES:
            for c in h["classes"]:
                lines.append(f"{c['label']} : count: {c['count']}, minutes: {to_fixed(c['duration'] / 60, 2)} {c['correct']} {c['wrong']} "
                             f"{_percent(c['correct'], c['wrong'])}%")
    for o in table["ords"]:
        lines.append(f"Label: {o['name']}, Type: Ordinal")
        lines.append(f"Range: {js_number_str(o['min'])} - {js_number_str(o['max'])}")
        lines.append(f"Samples: {o['true_n']}")
        lines.append(f"Predicted: {o['pred_n']}")
        lines.append(f"RMSE: {to_fixed(o['rmse'], 3)}")
    return [" ".join(x.split()) for x in lines]


# ---- evaluation beyond the panel: specification EV-1 (K8e is the device half, capi.FeatureDBStats.confusion / .agreement)
def _ratio(a, b):
    return a / b if b else math.nan                  # 0 / 0 stays NaN, as the panel's Accuracy does


def confusion_metrics(matrix):
    """matrix [V][V + 1] integers, m[true][predicted] with the blank predictions in column V -> dict(recall [V], precision [V], uar).
    recall[t] = m[t][t] / (row t's sum, blanks included: a blank row is a missed row); precision[p] = m[p][p] / (column p's sum);
    uar = the unweighted mean of the recalls of the classes that have a counted row (NaN without one)."""
    m = [[int(x) for x in row] for row in matrix]
    V = len(m)
    rows = [sum(r) for r in m]
    recall = [_ratio(m[t][t], rows[t]) for t in range(V)]
    precision = [_ratio(m[p][p], sum(m[t][p] for t in range(V))) for p in range(V)]
    have = [recall[t] for t in range(V) if rows[t]]
    return dict(recall=recall, precision=precision, uar=_ratio(sum(have), len(have)))       # a plain in-order sum: js/dbstats.js adds the same way


def assemble_confusion(columns, matrices):
    """[{name, labels, matrix, recall, precision, uar}] per categorical head from K8e's matrices (plain lists; labels = the vocabulary,
    whose order is the panel's: first appearance among the counted rows, then legend and predicted-only labels)."""
    out = []
    for col, m in zip(columns["cats"], matrices):
        m = [[int(x) for x in row] for row in m]
        out.append(dict(name=col["name"], labels=list(col["vocab"]), matrix=m, **confusion_metrics(m)))
    return out


def assemble_agreement(columns, agree):
    """[{name, n, mean_true, mean_pred, var_true, var_pred, cov, ccc, pearson}] per ordinal head from K8e's records."""
    keys = ("mean_true", "mean_pred", "var_true", "var_pred", "cov", "ccc", "pearson")
    return [dict(name=col["name"], n=int(agree["n"][o]), **{k: float(agree[k][o]) for k in keys}) for o, col in enumerate(columns["ords"])]


def _pct(x):
    return to_fixed(x * 100, 2) + "%"


def confusion_lines(confusion):
    """Text in the style of stats_lines: per head the matrix over the classes that occur (a counted row or a prediction), one line per
    true class with its recall, then the precisions and the UAR; percentages through to_fixed, 0 / 0 printed as NaN as the panel does."""
    lines = []
    for h in confusion:
        m, V = h["matrix"], len(h["labels"])
        used = [v for v in range(V) if sum(m[v]) or sum(m[t][v] for t in range(V))]
        lines.append(f"Label: {h['name']}, Type: Class, Confusion")
        lines.append("True \\ Predicted: " + ",".join([h["labels"][v] for v in used] + ["NaN"]))
        for t in used:
            lines.append(f"{h['labels'][t]} : " + " ".join(str(m[t][p]) for p in used + [V]) + f" recall: {_pct(h['recall'][t])}")
        lines.append("Precision: " + ", ".join(f"{h['labels'][p]} {_pct(h['precision'][p])}" for p in used))
        lines.append(f"UAR: {_pct(h['uar'])}")
    return [" ".join(x.split()) for x in lines]


def agreement_lines(agreement):
    lines = []
    for o in agreement:
        lines.append(f"Label: {o['name']}, Type: Ordinal, Agreement")
        lines.append(f"Pairs: {o['n']}")
        lines.append(f"Mean: {to_fixed(o['mean_true'], 3)} true, {to_fixed(o['mean_pred'], 3)} predicted")
        lines.append(f"Variance: {to_fixed(o['var_true'], 3)} true, {to_fixed(o['var_pred'], 3)} predicted, covariance {to_fixed(o['cov'], 3)}")
        lines.append(f"CCC: {to_fixed(o['ccc'], 3)}")
        lines.append(f"Pearson: {to_fixed(o['pearson'], 3)}")
    return [" ".join(x.split()) for x in lines]


def file_columns(db_rows):
    """(file_of_row [n] i32, callback_of_row [n] i32, file names) from the rows' `file` and `seg`: files are numbered in order of first
    appearance, a row without a file name gets -1; the callback is the integer part of the `seg` tag (String(si) at level 5,
    String(si + k / 100) at levels 12 / 13), 0 where it is no number.  A file whose rows are not together makes file_of_row decrease,
    which wsa_dbstats_set_files refuses naming the row."""
    names, index = [], {}
    file_of_row, callback_of_row = np.full(len(db_rows), -1, np.int32), np.zeros(len(db_rows), np.int32)
    for i, r in enumerate(db_rows):
        f = r.get("file")
        if f is not None and f != "":
            key = js_str(f)
            if key not in index:
                index[key] = len(names)
                names.append(key)
            file_of_row[i] = index[key]
        si = parse_float(r.get("seg"))
        callback_of_row[i] = int(math.floor(si)) if si == si and abs(si) < 2 ** 31 else 0
    return file_of_row, callback_of_row, names


def file_truths(columns, file_of_row, n_files):
    """The host rule for a file's label: per head the label of the file's FIRST COUNTED row (true_idx >= 0; a true value that is neither
    0 nor NaN); -1 / NaN for a file without one.  Returns ([true_idx [n_files]] per categorical head, [true_value [n_files]] per ordinal head)."""
    cats = [np.full(n_files, -1, np.int32) for _ in columns["cats"]]
    ords = [np.full(n_files, np.nan) for _ in columns["ords"]]
    for h, c in enumerate(columns["cats"]):
        for i in range(len(file_of_row) - 1, -1, -1):
            if file_of_row[i] >= 0 and c["true_idx"][i] >= 0:
                cats[h][file_of_row[i]] = c["true_idx"][i]
    for o, c in enumerate(columns["ords"]):
        for i in range(len(file_of_row) - 1, -1, -1):
            v = c["true_value"][i]
            if file_of_row[i] >= 0 and v == v and v != 0:
                ords[o][file_of_row[i]] = v
    return cats, ords


def _level_result(col, cat, cls, od, matrices, agree):
    table = assemble_table(col, cat, cls, od)
    confusion = assemble_confusion(col, matrices)
    agreement = assemble_agreement(col, agree) if col["ords"] else []
    return dict(table=table, confusion=confusion, agreement=agreement,
                lines=stats_lines(table) + confusion_lines(confusion) + agreement_lines(agreement))


def evaluate(an, db_rows, class_labels, ordinal_labels, models=None, per_file=True, first_row=0, n_rows=None, stream=0):
    """The evaluation of a labelled DB on the GPU (spec EV-1), from ONE device object: DS-1's table, a confusion matrix per categorical
    head and the agreement (CCC, Pearson) per ordinal head, at row level and, with per_file, with a file as the row.
    db_rows: rows as for stats_table, or a featdb.DeviceDB (its rows stay on the device); first_row / n_rows select a run of consecutive
    rows of either (default: all; of a DeviceDB the run is copied device to device, wsa_featdb_dbstats_create).  models: {head name: a capi.Model, an
    nnmodel.ModelSpec or a model directory}; a named head is predicted on the device (every row, as predict_db does, and the rows' `pred`
    pairs are written by update_pred_label's rule); the other heads are evaluated on the predictions the rows hold.
    Per file: a categorical head WITH a model is folded as the app folds a launch (K6b over the file's callbacks; the file's class is the
    largest meter sum); one without a model has no probabilities to fold and its files stay blank.  An ordinal head's file value is RG-1's
    running value over the rows' predictions.  A file's true label is that of its first counted row (file_truths).
    Returns {rows: {table, confusion, agreement, lines}, files: the same over the files plus names, durations per file in the table's
    classes, sums {head: [n_files][C]}, classes {head: [label or None]}, values {head: [..]}, folded {head: bool} — False for a
    categorical head without a model: its file-level counts and matrix are all blank because nothing was folded, not because the model
    abstained} (files: None without per_file)."""
    from . import capi
    cats, ords = head_settings(class_labels, ordinal_labels)
    models = dict(models or {})
    for name in models:
        if not (any(name == c for c, _ in cats) or name in ords):
            raise ValueError(f"models names the head {name!r}; the settings have {[c for c, _ in cats] + ords}")
    records = getattr(db_rows, "records", db_rows)
    if isinstance(db_rows, capi.FeatDB) and len(records) != db_rows.count:
        raise ValueError(f"the device DB holds {db_rows.count} rows and {len(records)} records")
    first_row = int(first_row)
    n_rows = len(records) - first_row if n_rows is None else int(n_rows)
    if first_row < 0 or n_rows < 0 or first_row + n_rows > len(records):
        raise ValueError(f"rows {first_row} .. {first_row + n_rows} are outside the DB's {len(records)} rows")
    records = records[first_row:first_row + n_rows]
    if len(records) < 1:
        raise ValueError("a feature DB has at least one row")
    feat = None
    if models:
        if isinstance(db_rows, capi.FeatDB):
            feat = db_rows
        else:
            feat = np.array([r["features"] for r in records], np.float64)
    loaded = {name: _model_of(an, spec) for name, spec in models.items()}
    try:
        legends = {name: [js_str(x) for x in m.labels] for name, (m, _) in loaded.items() if any(name == c for c, _ in cats)}
        predict_cat = {name: (lambda db, h, legend_to_vocab, m=loaded[name][0]: db.predict_classes(h, m, legend_to_vocab, stream)) for name in legends}
        predict_ord = {name: (lambda db, o, m=loaded[name][0]: db.predict_values(o, m, None, None, stream)) for name in loaded if name in ords}
        return evaluate_columns(an, records, feat, first_row, class_labels, ordinal_labels, legends, predict_cat, predict_ord, per_file, stream)
    finally:
        for m, mine in loaded.values():
            if mine:
                m.close()


def evaluate_columns(an, records, feat, first_row, class_labels, ordinal_labels, legends, predict_cat, predict_ord, per_file=True, stream=0,
                     prepare=None):
    """What evaluate does once it knows who predicts a head, shared with crossval.cross_validate: the columns, ONE device object, the
    predictions, the per-file fold and both levels' results.  records: the rows evaluated; feat: their features (host array, a capi.FeatDB
    whose rows first_row .. are theirs, or None); legends {categorical head: legend labels}; predict_cat {head: f(db, h, legend_to_vocab)}
    and predict_ord {head: f(db, o)} enqueue a head's prediction on the capi.FeatureDBStats; prepare(db) runs once before them."""
    from . import capi
    cats, ords = head_settings(class_labels, ordinal_labels)
    col = build_columns(records, class_labels, ordinal_labels, legends)
    if not col["cats"] and not col["ords"]:
        empty = dict(table=dict(cats=[], ords=[]), confusion=[], agreement=[], lines=[])
        return dict(rows=empty, files=None)
    db = an.feature_db(feat, col["durations"], [len(c["vocab"]) for c in col["cats"]], len(col["ords"]),
                       first_row=first_row if isinstance(feat, capi.FeatDB) else 0)
    try:
        for h, c in enumerate(col["cats"]):
            db.set_classes(h, c["true_idx"], c["pred_idx"])
        for o, c in enumerate(col["ords"]):
            db.set_values(o, c["true_value"], c["pred_value"])
        files = None
        if per_file:
            file_of_row, callback_of_row, names = file_columns(records)
            if names:
                db.set_files(file_of_row, callback_of_row, len(names))
                t_cats, t_ords = file_truths(col, file_of_row, len(names))
                for h, t in enumerate(t_cats):
                    db.set_file_classes(h, t)
                for o, t in enumerate(t_ords):
                    db.set_file_values(o, t)
                files = dict(names=names, sums={}, classes={}, values={}, folded={c["name"]: c["name"] in predict_cat for c in col["cats"]})
        if prepare is not None:
            prepare(db)
        for h, c in enumerate(col["cats"]):
            if c["name"] not in predict_cat:
                continue
            legend = legends[c["name"]]
            predict_cat[c["name"]](db, h, [c["vocab"].index(x) for x in legend])
            if files is not None:
                db.fold_files(h, stream)
                files["sums"][c["name"]] = db.file_sums(h, len(legend), stream)
                files["classes"][c["name"]] = [c["vocab"][i] if i >= 0 else None for i in db.file_classes(h, stream)]
            for r, i in zip(records, db.pred_classes(h, stream)):
                update_pred_label(r, cats, ords, c["name"], c["vocab"][i] if i >= 0 else None)
        for o, c in enumerate(col["ords"]):
            if c["name"] in predict_ord:
                predict_ord[c["name"]](db, o)
                for r, v in zip(records, db.pred_values(o, stream)):
                    update_pred_label(r, cats, ords, c["name"], float(v))
            if files is not None:
                db.fold_file_values(o, stream)
                files["values"][c["name"]] = [float(v) for v in db.file_values(o, stream)]
        n_cat = len(col["cats"])
        rows = _level_result(col, *db.table(stream), [db.confusion(h, stream) for h in range(n_cat)], db.agreement(stream) if col["ords"] else None)
        if files is not None:
            files.update(_level_result(col, *db.file_table(stream), [db.file_confusion(h, stream) for h in range(n_cat)],
                                       db.file_agreement(stream) if col["ords"] else None))
    finally:
        db.close()
    return dict(rows=rows, files=files)


def update_pred_label(row, cats, ords, label, value):
    """localstore.js:723-769 on one row: slot 0 when `label` names a categorical head, else slot 1 when it names an ordinal head; the pair
    is stored in every case.  The value goes through JSON as the app's storage does: NaN / Infinity become null, -0 becomes 0."""
    pair = row.get("pred") if js_truthy(row.get("pred")) else [{}, {}]
    if isinstance(value, float):
        value = None if (value != value or math.isinf(value)) else (0.0 if value == 0 else value)
    if any(name == label for name, _ in cats):
        pair[0][label] = value
    elif label in ords:
        pair[1][label] = value
    row["pred"] = pair


def _model_of(an, spec_or_model):
    from . import capi
    if isinstance(spec_or_model, capi.Model):
        return spec_or_model, False
    return an.load_model(spec_or_model), True


def predict_db(an, db_rows, heads, label_type, label_name, spec, out_min=None, out_max=None, stream=0, return_raw=False):
    """predict_db_nn (neuralmodel.js:410-535) on the GPU: runs the model over EVERY row, with or without a true label, and writes each
    row's prediction into its `pred` pair by update_pred_label's rule.  heads = (class_labels, ordinal_labels); label_type 'cats' or
    'ords'; spec: a capi.Model, an nnmodel.ModelSpec or a model directory.  db_rows may be a featdb.DeviceDB of `an`: the model then runs over
    its rows where they are (a device-to-device copy, wsa_featdb_dbstats_create) and the predictions go into its records.  Returns the per-row predictions (labels or None for 'cats',
    values for 'ords'); return_raw adds the probabilities [n][C] / the values K8 used."""
    if label_type not in ("cats", "ords"):
        raise ValueError(f"label_type is 'cats' or 'ords', got {label_type!r}")
    cats, ords = head_settings(*heads)
    from . import capi, nnmodel
    if (db_rows.count if isinstance(db_rows, capi.FeatDB) else len(db_rows)) < 1:
        raise ValueError("a feature DB has at least one row")
    if isinstance(db_rows, capi.FeatDB):                 # the features stay on the device; the records are the rows
        if not hasattr(db_rows, "records"):
            raise TypeError("predict_db takes a featdb.DeviceDB (it keeps the rows' records); a bare capi.FeatDB has none")
        feat, width, db_rows = db_rows, db_rows.width, db_rows.records
        if len(db_rows) != feat.count:
            raise ValueError(f"the device DB holds {feat.count} rows and {len(db_rows)} records")
    else:
        feat = np.array([r["features"] for r in db_rows], np.float64)
        if feat.ndim != 2 or feat.shape[1] not in nnmodel.WIDTHS:
            raise ValueError(f"features {feat.shape}: the models take level-5 / level-13 rows of 53 features (or level-11 rows of 264, level-12 rows of 23)")
        width = feat.shape[1]
    dur = np.array([parse_float(r["time"][1]) for r in db_rows], np.float64)
    model, mine = _model_of(an, spec)
    try:
        if model.n_inputs != width:                      # before anything is uploaded or enqueued
            raise ValueError(f"the model takes {model.n_inputs} inputs; the DB's rows have {width} features")
        if label_type == "cats":
            legend = [js_str(x) for x in model.labels]
            if len(legend) != model.n_classes:
                raise ValueError(f"the model has {model.n_classes} classes and a legend of {len(legend)} labels")
            db = an.feature_db(feat, dur, [len(legend)], 0)
            try:
                db.predict_classes(0, model, np.arange(len(legend)), stream)
                idx = db.pred_classes(0, stream)
                raw = db.probs(len(legend), stream) if return_raw else None
            finally:
                db.close()
            preds = [legend[i] if i >= 0 else None for i in idx]
        else:
            db = an.feature_db(feat, dur, [], 1)
            try:
                db.predict_values(0, model, out_min, out_max, stream)
                raw = db.pred_values(0, stream)
            finally:
                db.close()
            preds = [float(v) for v in raw]
    finally:
        if mine:
            model.close()
    for r, p in zip(db_rows, preds):
        update_pred_label(r, cats, ords, label_name, p)
    return (preds, raw) if return_raw else preds


def stats_table(an, db_rows, class_labels, ordinal_labels, stream=0):
    """shows_stats_table's numbers (localstore.js:498-627) on the GPU, as plain data:
    {cats: [{name, correct, wrong, blank, classes: [{label, count, duration, correct, wrong}]}], ords: [{name, min, max, true_n, pred_n,
    sq_sum, rmse}]}; stats_lines(table) prints it as the app does.  db_rows may be a featdb.DeviceDB: its records are counted."""
    db_rows = getattr(db_rows, "records", db_rows)
    col = build_columns(db_rows, class_labels, ordinal_labels)
    if not col["cats"] and not col["ords"]:
        return dict(cats=[], ords=[])
    db = an.feature_db(None, col["durations"], [len(c["vocab"]) for c in col["cats"]], len(col["ords"]))
    try:
        for h, c in enumerate(col["cats"]):
            db.set_classes(h, c["true_idx"], c["pred_idx"])
        for o, c in enumerate(col["ords"]):
            db.set_values(o, c["true_value"], c["pred_value"])
        cat, cls, od = db.table(stream)
    finally:
        db.close()
    return assemble_table(col, cat, cls, od)
