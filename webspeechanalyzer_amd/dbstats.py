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
