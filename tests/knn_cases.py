"""The rows the KNN tests run on (test helper): one table of cases for specification KN-1 / kernel K9, every row made from (case, seed)
by integer arithmetic (no random generator, no libm: the same on every numpy build).  tests/golden/knn_expected.json names its rows by
case key and seed only; tests/golden/gen/make_knn_golden.py, tests/test_knn_reference.py and tests/test_gpu_knn.py rebuild them here.

T and QT are the tile sizes the shapes were placed by (K9 streams the store T rows at a time and keeps QT query rows per workgroup);
tests/test_gpu_knn.py checks them against what the library reports.  The cases keep to a few queries each, so that the fixture stays
small: the query counts at the tile edges (1, QT - 1, QT + 1) are tests/test_gpu_knn.py's shape sweep, held to the restatement.

case            width  store  queries  what it reaches
  main53          53    2T+1     4     three store tiles with a last tile of one row; k 1, 3, 10, 64
  small53         53     40      5     k = n and k > n (clamped to the 40 examples)
  w23             23    T+1      4     the k remainder of 23 (padding of 1), a store tile of one row; two classes
  w264           264     T       3     the wide rows; 64 classes, one row each, first appearance out of suffix order
  one / two       53   1 / 2   2 / 1   the smallest stores (one class; k > n)
  tm1             53    T-1      1     a store of one row less than a tile, one query
  dup3            53     20      2     one row stored under three labels: the grouped rank decides (k 1, 2, 3)
  straddle        53     70      2     a duplicate pair on both sides of the first tile boundary; the LATER one has the lower rank and
                                       must displace its equal from a full list (k 1)
  late            53    130      2     a duplicate in the third tile whose equal in the first has the lower rank and must stay (k 1), and
                                       a doubled copy, which normalises to the same unit row
  ties            53     30     16     vote ties at k = 2 and k = 4: the first class in key order wins
  keyorder_str    53     40      4     labels "10", "b", "2", "a" interleaved: ml5 numbers string labels by first appearance
  keyorder_num    53     40      4     labels 10, 7, 2, 3 as numbers: each is its own class id, scanned ascending, not by appearance
  evaluate        53    160      -     a labelled DB for train_knn's procedure (rows without the label, labels outside the class list)
"""
import json
import os

import numpy as np

T, QT = 64, 64
_M32 = np.uint64(0xFFFFFFFF)
_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mix(a, b, salt):
    """a 32-bit hash of two non-negative integers (arrays broadcast) in uint64 arithmetic: multiply, xor-shift, twice"""
    x = (np.asarray(a, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(b, np.uint64) * np.uint64(0x85EBCA77) + np.uint64(salt)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & _M32
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & _M32
    x ^= x >> np.uint64(15)
    return x


def ranges(width):
    """(lo, hi) per feature: at 53 the input ranges of the shipped model 1 (tests/golden/nn: model_meta.json), else a made-up ladder"""
    if width == 53:
        meta = json.load(open(os.path.join(_GOLD, "nn", "1", "cats_emotion", "model_meta.json")))["inputs"]
        return (np.array([float(meta[str(j)]["min"]) for j in range(53)]), np.array([float(meta[str(j)]["max"]) for j in range(53)]))
    j = np.arange(width)
    return np.zeros(width), 1.0 + 10.0 * (j % 7)


def draw(width, n, salt, first=0):
    """n rows inside ranges(width): row first + i, feature j from mix(first + i, j, salt) / 2^32"""
    lo, hi = ranges(width)
    u = mix(np.arange(first, first + n)[:, None], np.arange(width)[None, :], salt).astype(np.float64) / 4294967296.0
    return lo + u * (hi - lo)


def _case(key, width, n, q, ks, labels, dup=()):
    return dict(key=key, width=width, n=n, q=q, ks=list(ks), labels=labels, dup=list(dup))


_FIVE = ["ang", "hap", "neu", "sad", "sur"]
# labels: a function (row index, seed) -> label; dup: (target row, source row, factor): store[target] = factor * store[source]
CASES = {c["key"]: c for c in (
    _case("main53", 53, 2 * T + 1, 4, (1, 3, 10, 64), lambda i, s: _FIVE[int(mix(i, 1, s + 5)) % 5]),
    _case("small53", 53, 40, 5, (10, 40, 50), lambda i, s: _FIVE[int(mix(i, 2, s + 5)) % 3]),
    _case("w23", 23, T + 1, 4, (3, 10, 64), lambda i, s: ("x", "y")[int(mix(i, 3, s + 5)) % 2]),
    _case("w264", 264, T, 3, (1, 10, 64), lambda i, s: "c%d" % ((i * 37) % 64)),
    _case("one", 53, 1, 2, (1, 3), lambda i, s: "only"),
    _case("two", 53, 2, 1, (1, 2), lambda i, s: ("a", "b")[i]),
    _case("tm1", 53, T - 1, 1, (1, 10), lambda i, s: _FIVE[int(mix(i, 4, s + 5)) % 4]),
    _case("dup3", 53, 20, 2, (1, 2, 3), lambda i, s: {3: "A", 7: "B", 11: "C"}.get(i, "ABC"[i % 3]), dup=((7, 3, 1.0), (11, 3, 1.0))),
    _case("straddle", 53, 70, 2, (1, 2), lambda i, s: "q" if i in (0, T) else "p", dup=((T, T - 1, 1.0),)),
    _case("late", 53, 130, 2, (1, 2, 3), lambda i, s: {0: "a", 1: "b", 5: "a", 100: "b", 120: "a"}.get(i, "ab"[int(mix(i, 6, s + 5)) % 2]),
          dup=((100, 5, 1.0), (120, 5, 2.0))),
    _case("ties", 53, 30, 16, (2, 4), lambda i, s: "b" if i == 0 else "a" if i == 1 else "ba"[int(mix(i, 7, s + 5)) % 2]),
    _case("keyorder_str", 53, 40, 4, (4, 10), lambda i, s: ("10", "b", "2", "a")[(i + i // 4) % 4]),
    _case("keyorder_num", 53, 40, 4, (4, 10), lambda i, s: (10, 7, 2, 3)[(i + i // 4) % 4]),
)}
# queries that ARE a stored row (the duplicated one), so the duplicates tie at the top: case -> {query index: store row}
QUERY_IS = {"dup3": {0: 3}, "straddle": {0: T - 1}, "late": {0: 5}}


def build(key, seed):
    """dict(store [n, width] f64, labels [n], queries [q, width] f64, ks) of a case at a seed"""
    c = CASES[key]
    store = draw(c["width"], c["n"], seed)
    for target, source, factor in c["dup"]:
        store[target] = factor * store[source]
    queries = draw(c["width"], c["q"], seed + 1, first=100000)
    for qi, row in QUERY_IS.get(key, {}).items():
        queries[qi] = store[row]
    return dict(store=store, labels=[c["labels"](i, seed) for i in range(c["n"])], queries=queries, ks=c["ks"])


def same_unit_row(a, b):
    """rows that normalise to the same unit row by construction: equal, or one the double of the other"""
    return bool(np.array_equal(a, b) or np.array_equal(a, 2.0 * b) or np.array_equal(2.0 * a, b))


# ---- the labelled DB of the `evaluate` case: train_knn's procedure (ref src/neuralmodel.js:761-828)
EVAL_N, EVAL_K = 160, 10
EVAL_VARIANTS = {"listed": ["hap", "sad", "neu"], "star": ["hap", "*"]}


def eval_db(seed):
    """(rows [160, 53], true labels [160]): labels of four kinds (one outside the `listed` classes), every eleventh row without a label;
    rows of one label lean towards that label's own centre, so the classifier has something to find"""
    rows = draw(53, EVAL_N, seed + 2)
    centres = draw(53, 4, seed + 3, first=200000)
    names = ["hap", "sad", "neu", "ang"]
    labels = []
    for i in range(EVAL_N):
        c = int(mix(i, 8, seed + 5)) % 4
        rows[i] = 0.5 * rows[i] + 0.5 * centres[c]
        labels.append(None if i % 11 == 10 else names[c])
    return rows, labels
