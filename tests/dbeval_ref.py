"""A Python restatement of specification EV-1 (DESIGN.md §3, K8e in csrc/dbeval.hip): the confusion matrix (Python integers), the
agreement of an ordinal head (f64, in EV-1's order: rows of a chunk of R consecutive rows in row order, then chunks in chunk order; no
product fused into its addition) and the per-file results (the app's fold over a file's callbacks, a file's class, RG-1's running
value).  Plain loops over numpy float64 scalars: every operation is one IEEE double operation, as on the device.  ARMS counts the arms
taken."""
import collections
import math

import numpy as np

from . import classify_ref

R = 256                       # WSA_DBSTATS_CHUNK_ROWS
U = 2.0 ** -53                # the unit roundoff of a double
ARMS = collections.Counter()
F = np.float64
KEYS = ("mean_true", "mean_pred", "var_true", "var_pred", "cov", "ccc", "pearson")


def counted(v):
    """DS-1's device rule for an ordinal value: truthy and not NaN"""
    return v == v and v != 0.0


# ---- part 1
def confusion(V, true_idx, pred_idx):
    """[V][V + 1] Python integers: m[t][p] over the rows with true_idx >= 0; column V collects the blank predictions."""
    m = [[0] * (V + 1) for _ in range(V)]
    for t, p in zip(true_idx, pred_idx):
        t, p = int(t), int(p)
        if t < 0:
            ARMS["row.not_counted"] += 1
            continue
        if p < 0:
            ARMS["pred.blank"] += 1
            m[t][V] += 1
        else:
            ARMS["pred.correct" if p == t else "pred.wrong"] += 1
            m[t][p] += 1
    return m


# ---- part 2
def _chunked(n, chunk_rows):
    return [(a, min(a + chunk_rows, n)) for a in range(0, n, chunk_rows)]


def agreement(true_value, pred_value, chunk_rows=R):
    """dict(n, mean_true, mean_pred, var_true, var_pred, cov, ccc, pearson) of one head in EV-1's order, and under "bound" the running-error
    bound of every figure against the exact value of its definition (error_bounds)."""
    t_val, p_val = np.asarray(true_value, F), np.asarray(pred_value, F)
    take = [counted(t) and counted(p) for t, p in zip(t_val, p_val)]
    with np.errstate(all="ignore"):
        n, st, sp = 0, F(0.0), F(0.0)
        for a, b in _chunked(len(t_val), chunk_rows):
            pt, pp = F(0.0), F(0.0)                         # every partial starts at +0 in every chunk
            for i in range(a, b):
                if not take[i]:
                    ARMS["pair.left_out"] += 1
                    continue
                ARMS["pair.taken"] += 1
                n += 1
                pt, pp = pt + t_val[i], pp + p_val[i]
            st, sp = st + pt, sp + pp
        ARMS["n.zero" if n == 0 else "n.positive"] += 1
        mt, mp = st / F(n), sp / F(n)
        sa, sb, sc = F(0.0), F(0.0), F(0.0)
        for a, b in _chunked(len(t_val), chunk_rows):
            pa, pb, pc = F(0.0), F(0.0), F(0.0)
            for i in range(a, b):
                if not take[i]:
                    continue
                dt, dp = t_val[i] - mt, p_val[i] - mp
                tt, pp, tp = dt * dt, dp * dp, dt * dp      # each product is rounded, then added: not fused
                pa, pb, pc = pa + tt, pb + pp, pc + tp
            sa, sb, sc = sa + pa, sb + pb, sc + pc
        vt, vp, cov = sa / F(n), sb / F(n), sc / F(n)
        d = mp - mt
        ccc = (F(2.0) * cov) / ((vt + vp) + d * d)
        pearson = cov / np.sqrt(vt * vp)
    if n and (vt == 0 or vp == 0):
        ARMS["variance.zero"] += 1
    out = dict(n=n, mean_true=float(mt), mean_pred=float(mp), var_true=float(vt), var_pred=float(vp), cov=float(cov), ccc=float(ccc),
               pearson=float(pearson))
    out["bound"] = error_bounds([t for t, k in zip(t_val, take) if k], [p for p, k in zip(p_val, take) if k], out)
    return out


def error_bounds(t, p, got):
    """How far a two-pass evaluation in doubles — this one or the reference's in-order one — can lie from the exact value of each figure:
    a sum of n terms carries at most n u sum|terms| (u = 2^-53 per addition, each partial sum at most sum|terms| in magnitude); the mean adds
    its division's rounding; a central term (x - mean)(y - mean) inherits the means' errors e, its subtractions' and its product's
    roundings (two units: Math.pow(x, 2) need not be x * x to the last bit); the quotients follow.  Two evaluations are therefore within
    TWICE these of each other; tests/test_dbeval_reference.py asserts the single bound, which is tighter and what EV-1 states.  Valid for finite input with n >= 1; every bound is NaN otherwise."""
    n = len(t)
    nan = {k: math.nan for k in KEYS}
    if n == 0 or not all(math.isfinite(x) for x in list(t) + list(p)):
        return nan
    t, p = [float(x) for x in t], [float(x) for x in p]

    def mean_err(x, m):
        return n * U * math.fsum(abs(v) for v in x) / n + U * abs(m)

    mt, mp = got["mean_true"], got["mean_pred"]
    et, ep = mean_err(t, mt), mean_err(p, mp)

    def central_err(x, mx, ex, y, my, ey, value):
        terms = term_err = 0.0
        for a, b in zip(x, y):
            da, db = abs(a - mx), abs(b - my)
            ea, eb = ex + U * da, ey + U * db                # the difference against the exact mean: the mean's error, the subtraction's rounding
            term_err += da * eb + db * ea + ea * eb + 2 * U * da * db
            terms += da * db
        terms += term_err
        return (term_err + n * U * terms) / n + U * abs(value)

    evt, evp = central_err(t, mt, et, t, mt, et, got["var_true"]), central_err(p, mp, ep, p, mp, ep, got["var_pred"])
    ec = central_err(t, mt, et, p, mp, ep, got["cov"])
    out = dict(mean_true=et, mean_pred=ep, var_true=evt, var_pred=evp, cov=ec)
    d = abs(mp - mt)
    den = got["var_true"] + got["var_pred"] + d * d
    e_den = evt + evp + 2 * d * (et + ep) + (et + ep) ** 2 + 4 * U * abs(den)
    out["ccc"] = (2 * ec + abs(got["ccc"]) * e_den) / (den - e_den) + 3 * U * abs(got["ccc"]) if den > e_den and got["ccc"] == got["ccc"] else math.nan
    prod = got["var_true"] * got["var_pred"]
    e_prod = got["var_true"] * evp + got["var_pred"] * evt + evt * evp + U * prod
    if prod > e_prod and got["pearson"] == got["pearson"]:
        e_root = e_prod / (2 * math.sqrt(prod - e_prod)) + U * math.sqrt(prod)
        out["pearson"] = (ec + abs(got["pearson"]) * e_root) / (math.sqrt(prod) - e_root) + 2 * U * abs(got["pearson"])
    else:
        out["pearson"] = math.nan
    return out


def in_order_agreement(true_value, pred_value):
    """The reference's own forms on the pairs that take part (src/stats.js:80-113 only_mean, variance, covariance and the expression of
    calc_ccc, src/neuralmodel.js:488, with covariance(y1, y2)): plain in-order sums."""
    pairs = [(F(t), F(p)) for t, p in zip(true_value, pred_value) if counted(t) and counted(p)]
    n = len(pairs)
    with np.errstate(all="ignore"):
        def only_mean(x):
            s = F(0.0)
            for v in x:
                s = s + v
            return s / F(n)

        t, p = [a for a, _ in pairs], [b for _, b in pairs]
        mt, mp = only_mean(t), only_mean(p)

        def cov(x, mx, y, my):
            s = F(0.0)
            for a, b in zip(x, y):
                s = s + (a - mx) * (b - my)
            return s / F(n)

        vt, vp, c = cov(t, mt, t, mt), cov(p, mp, p, mp), cov(t, mt, p, mp)
        ccc = (F(2.0) * c) / (vt + vp + (mp - mt) * (mp - mt))
        pearson = c / np.sqrt(vt * vp)
    return dict(n=n, mean_true=float(mt), mean_pred=float(mp), var_true=float(vt), var_pred=float(vp), cov=float(c), ccc=float(ccc), pearson=float(pearson))


# ---- part 3
def check_files(file_of_row, durations, n_files):
    """wsa_dbstats_set_files' refusals: None, or (kind, row) of the first offending row."""
    last = -1
    for r, (f, d) in enumerate(zip(file_of_row, durations)):
        f = int(f)
        if f < -1 or f >= n_files:
            return "outside", r
        if f < 0:
            continue
        if f < last:
            return "decreasing", r
        k = round(float(d) * 1000.0) if d == d and abs(d) < 1e12 else -1
        if not d >= 0 or k > 2147483647 or k / 1000.0 != d:
            return "milliseconds", r
        last = f
    return None


def file_rows(file_of_row, callback_of_row, n_files):
    """per file: its callbacks, each a list of rows — consecutive rows OF THE FILE with the same callback value (rows without a file
    are not there)"""
    files = [[] for _ in range(n_files)]
    last = {}
    for r, (f, c) in enumerate(zip(file_of_row, callback_of_row)):
        f, c = int(f), int(c)
        if f < 0:
            ARMS["file.none"] += 1
            continue
        if files[f] and last[f] == c:
            files[f][-1].append(r)
        else:
            files[f].append([r])
        last[f] = c
    return files


def file_durations(file_of_row, durations, n_files):
    out = np.zeros(n_files, F)
    for f, d in zip(file_of_row, durations):
        if f >= 0:
            out[f] = out[f] + F(d)
    return out


def fold_files(file_of_row, callback_of_row, durations, prob, labels, legend_to_vocab, n_files):
    """(sums [n_files][C] f64 = Label_conf_all at each file's end (0 for a label that never got a key), classes [n_files] vocabulary
    indices).  The fold is the app's (classify_ref.fold_clip, held to src/prediction.js by tests/test_classify_reference.py), fed the
    stored durations; the class is EV-1's: Object.keys order, strict > from 0."""
    C = len(labels)
    sums, classes = np.zeros((n_files, C), F), np.full(n_files, -1, np.int32)
    for f, cbs in enumerate(file_rows(file_of_row, callback_of_row, n_files)):
        for cb in cbs:
            ARMS["callback.one_syllable" if len(cb) == 1 else "callback.several"] += 1
        _, acc = classify_ref.fold_clip([([float(durations[r]) for r in cb], [prob[r] for r in cb]) for cb in cbs], labels)
        best, mx = None, 0.0
        for k in classify_ref._keys(acc):
            if acc[k] > mx:
                best, mx = k, acc[k]
            elif mx > 0 and acc[k] == mx:
                ARMS["file.tie"] += 1
        for c, lab in enumerate(labels):
            sums[f][c] = acc.get(lab, 0.0)
        ARMS["file.blank" if best is None else "file.class"] += 1
        classes[f] = -1 if best is None else legend_to_vocab[labels.index(best)]
    return sums, classes


def fold_file_values(file_of_row, callback_of_row, durations, values, n_files):
    """[n_files] f64: RG-1's running value at each file's end — sum v sqrt(d) / sum sqrt(d) over the file's rows with a finite v, in row
    order, a callback whose durations sum to 0 adding nothing; NaN when nothing was added."""
    out = np.full(n_files, np.nan, F)
    for f, cbs in enumerate(file_rows(file_of_row, callback_of_row, n_files)):
        A = B = 0.0
        for cb in cbs:
            seg_weight = 0.0
            for r in cb:
                seg_weight = seg_weight + float(durations[r])
            if not seg_weight > 0:
                ARMS["value.callback_skipped"] += 1
                continue
            for r in cb:
                v, w = float(values[r]), math.sqrt(float(durations[r]))
                if not math.isfinite(v):
                    ARMS["value.not_finite"] += 1
                    continue
                t = v * w
                A, B = A + t, B + w
        out[f] = A / B if B != 0 else math.nan
    return out


def same_f64(a, b):
    """bit for bit, with one NaN: the device writes the quiet NaN 0x7ff8000000000000 for every NaN"""
    a, b = np.asarray(a, F).ravel(), np.asarray(b, F).ravel()
    return a.shape == b.shape and all((x != x and y != y) or x.tobytes() == y.tobytes() for x, y in zip(a, b))
