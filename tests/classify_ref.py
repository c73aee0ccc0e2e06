"""Float64 restatement of the app's prediction path (test helper): ml5 normalisation + tfjs Dense network, and the fold of
src/prediction.js:86-169 (one model DB).  The network is the yardstick for K6 within a tolerance; the fold is exact double
arithmetic, so K6b must equal it bit for bit when fed the same f32 probabilities."""
import math
import os
from collections import Counter
from decimal import ROUND_FLOOR, ROUND_HALF_UP, Decimal, localcontext

import numpy as np


def forward(spec, feat):
    """feat [n, 53] f64 -> probabilities [n, C] (f64): (x - min) / (max - min) in double, rounded to f32 (the tensor), then
    act(x W + b) per layer in f64 with the f32 weights, softmax on the last layer."""
    x = ((np.asarray(feat, np.float64) - spec.in_min) / (spec.in_max - spec.in_min)).astype(np.float32).astype(np.float64)
    for k, b, a in zip(spec.kernels, spec.biases, spec.activations):
        x = x @ k.astype(np.float64) + b.astype(np.float64)
        if a == "relu":
            x = np.maximum(x, 0.0)
        elif a == "sigmoid":
            x = 1.0 / (1.0 + np.exp(-x))
        elif a == "tanh":
            x = np.tanh(x)
        elif a == "softmax":
            m = x.max(axis=1, keepdims=True)
            x = np.exp(x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))))
    return x


# How often each arm of the fold's comparisons was taken (tests/test_fold_reference.py asserts that the hand-built cases of
# tests/fold_cases.py reach every one; ensemble_ref counts the ensemble's).  "seg" / "all": the segment and the launch accumulator.
FOLD_ARM_NAMES = (
    "fixed3.down", "fixed3.up", "fixed3.tie", "skip.zero", "skip.positive", "syllables.one", "syllables.several",
    "seg.absent", "seg.zero", "seg.nan", "seg.added", "all.absent", "all.zero", "all.nan", "all.added",
    "rank_tie.yes", "rank_tie.no", "rank_tie.all_nan", "key.index", "key.string",
    "sum_tie.index_index", "sum_tie.string_string", "sum_tie.index_string", "label.found", "label.null",
    "winner.replaced", "winner.tie_kept", "winner.none", "min_db.raised", "min_db.tie_kept", "min_db.skipped", "min_db.none",
    "all_sum.legend_order", "all_sum.key_order_differs")
FOLD_ARMS = Counter()


def fixed3(x):
    """parseFloat(x.toFixed(3)): toFixed takes the n for which n / 1000 - x is closest to zero on the EXACT binary value of x, the larger
    n on a tie — and ties do occur (every odd multiple of 1/2000 that is a binary fraction, e.g. 0.0625 -> "0.063"), so round half up on
    the exact value (Decimal(x) is exact), not '%.3f' (half even)."""
    with localcontext() as ctx:
        ctx.prec = 1200                           # exact: a double has at most 1074 fractional digits
        k = Decimal(x) * 1000
        frac = k - k.to_integral_value(rounding=ROUND_FLOOR)
    FOLD_ARMS["fixed3.tie" if frac == Decimal("0.5") else ("fixed3.up" if frac > Decimal("0.5") else "fixed3.down")] += 1
    return float(Decimal(x).quantize(Decimal("0.001"), rounding=ROUND_HALF_UP))


def _array_index(label):
    s = str(label)
    return int(s) if s.isascii() and s.isdigit() and (s == "0" or s[0] != "0") and int(s) <= 2 ** 32 - 2 else None      # V8's array indices end at 2^32 - 2


def _keys(acc):
    """Object.keys order: array-index keys ascending, then the rest in insertion order."""
    ks = list(acc.keys())
    for k in ks:
        FOLD_ARMS["key.index" if _array_index(k) is not None else "key.string"] += 1
    idx = sorted((k for k in ks if _array_index(k) is not None), key=_array_index)
    return idx + [k for k in ks if _array_index(k) is None]


def _add(acc, label, w, arm="all"):
    v = acc.get(label)              # `if(!acc[label]) acc[label] = wconf; else acc[label] += wconf;` (absent / 0 / NaN: assign)
    FOLD_ARMS[arm + (".absent" if v is None else ".zero" if v == 0 else ".nan" if v != v else ".added")] += 1
    if v is None or v == 0 or v != v:
        acc[label] = w
    else:
        acc[label] += w


def classify_multiple(prob_row, labels):
    """ml5 classifyMultiple's per-input result: {label, confidence} sorted by confidence descending (`b.confidence - a.confidence` under
    V8's stable sort), ties in legend order.  A row that is NaN throughout (K6's output for a non-finite feature) stays in legend order:
    every comparison answers NaN, which the sort reads as "not before" (recorded from ml5 itself in tests/golden/fold_expected.json,
    ml5_order).  A row that mixes NaN and numbers has no specified order (an inconsistent comparator) and is refused."""
    p = [float(v) for v in prob_row]
    n_nan = sum(1 for v in p if v != v)
    if n_nan:
        if n_nan != len(p):
            raise ValueError("a row that mixes NaN and finite confidences has no specified order")
        FOLD_ARMS["rank_tie.all_nan"] += 1
        return [(labels[c], p[c]) for c in range(len(labels))]
    FOLD_ARMS["rank_tie.yes" if len(set(p)) < len(p) else "rank_tie.no"] += 1
    order = sorted(range(len(labels)), key=lambda c: -p[c])
    return [(labels[c], p[c]) for c in order]


def fold_segment(acc_all, durs, probs, labels):
    """nn_prediction's call_back_x4 (ref prediction.js:89-115) for one model DB: adds the callback's syllables to acc_all, returns
    Label_conf_seg."""
    acc_seg = {}
    FOLD_ARMS["syllables.one" if len(durs) == 1 else "syllables.several"] += 1
    for d, p in zip(durs, probs):
        w = math.sqrt(d)
        res = classify_multiple(p, labels)
        for lab, conf in (res[:1] if len(durs) == 1 else res):
            _add(acc_all, lab, conf * w, "all")
            _add(acc_seg, lab, conf * w, "seg")
    return acc_seg


def segment_label(acc_all, acc_seg):
    """The segment's label and maximum as seg_confidence_sort finds them (ref prediction.js:134-151): Label_conf_all's keys in
    Object.keys order, strict > from 0 — so equal sums go to the earlier key."""
    best, mx = None, 0.0
    for k in _keys(acc_all):
        if k in acc_seg and acc_seg[k] > mx:
            mx, best = acc_seg[k], k
        elif k in acc_seg and mx > 0 and acc_seg[k] == mx:
            a, b = _array_index(best) is not None, _array_index(k) is not None
            FOLD_ARMS["sum_tie.index_index" if a and b else "sum_tie.index_string" if a else "sum_tie.string_string"] += 1
    FOLD_ARMS["label.null" if best is None else "label.found"] += 1
    return best, mx


def fold_clip(callbacks, labels):
    """callbacks: [(durations [f64 per syllable] = parseFloat(seg_time[ph][1]), probabilities [n_syl][C])] of one launch.
    Returns ([(label or None or 'skip', confidence)], Label_conf_all as an ordered dict)."""
    acc_all = {}
    out = []
    for durs, probs in callbacks:
        seg_weight = 0.0
        for d in durs:
            seg_weight += d
        FOLD_ARMS["skip.positive" if seg_weight > 0 else "skip.zero"] += 1
        if not seg_weight > 0:
            out.append(("skip", 0.0))
            continue
        acc_seg = fold_segment(acc_all, durs, probs, labels)
        best, mx = segment_label(acc_all, acc_seg)
        out.append((best, mx / seg_weight))
    return out, acc_all


def fold_rows(meta, prob, labels, step_s):
    """The fold over a batch's compacted level-13 rows (meta [n, 8]: clip, si, t_start, t_len, ...) as the device does it:
    returns (callbacks [(clip, si, first row, rows, label index (-1 null, -2 skipped), conf)], {clip: Label_conf_all})."""
    cbs, accs = [], {}
    by_clip = {}
    r = 0
    while r < len(meta):
        e = r + 1
        while e < len(meta) and meta[e][0] == meta[r][0] and meta[e][1] == meta[r][1]:
            e += 1
        by_clip.setdefault(int(meta[r][0]), []).append((r, e))
        r = e
    for clip, runs in by_clip.items():
        items = [([fixed3((int(meta[q][3]) + 1) * step_s) for q in range(a, b)], [prob[q] for q in range(a, b)]) for a, b in runs]
        res, acc = fold_clip(items, labels)
        accs[clip] = acc
        for (a, b), (lab, conf) in zip(runs, res):
            li = -2 if lab == "skip" else (-1 if lab is None else labels.index(lab))
            cbs.append((clip, int(meta[a][1]), a, b - a, li, conf))
    return cbs, accs


def seeded_spec(seed=5, widths=(512, 512, 8), labels=None):
    """A Dense classifier with weights drawn from a seed and the input ranges of the app's model 1 (tests/golden/nn/1/cats_emotion):
    53 -> 512 -> 512 -> 8 by default, the shape of the app's models 4 .. 7 (whose 1.18 MB weight files are not committed)."""
    from webspeechanalyzer_amd import nnmodel
    rng = np.random.default_rng(seed)
    m1 = nnmodel.load_dir(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn", "1", "cats_emotion"))
    units = [53] + list(widths)
    ks = [(rng.standard_normal((units[i], units[i + 1])) * np.sqrt(2.0 / (units[i] + units[i + 1]))).astype(np.float32) for i in range(len(widths))]
    bs = [(rng.standard_normal(units[i + 1]) * 0.05).astype(np.float32) for i in range(len(widths))]
    acts = ["relu"] * (len(widths) - 1) + ["softmax"]
    return nnmodel.ModelSpec(units, acts, ks, bs, m1.in_min, m1.in_max, labels or [f"c{i}" for i in range(widths[-1])])
