"""numpy restatement of specification FD-1: which rows of a run the device feature DB keeps, what it stores for them, and
the per-column ranges.  Written from the specification's sentences, not from csrc/featdb.hip or webspeechanalyzer_amd/featdb.py."""
import numpy as np

WIDTH = {5: 53, 13: 53, 11: 264, 12: 23}


def keep(level, meta=None, feat=None, off=None, n=None):
    """the kept source rows in source order.  levels 5 / 13: every row (n of them); level 12: row r unless some r' <= r with the same
    (meta[r'][0], meta[r'][1]) has a slot 23 that is not equal to 0; level 11: off[c + 1] - 1 of every clip with off[c + 1] > off[c]"""
    if level in (5, 13):
        return list(range(len(feat) if n is None else n))
    if level == 11:
        return [int(off[c + 1]) - 1 for c in range(len(off) - 1) if int(off[c + 1]) > int(off[c])]
    assert level == 12
    slot = np.asarray(feat)[:, 23] if len(feat) else np.zeros(0)
    marked_from = {}
    out = []
    for r in range(len(slot)):
        key = (int(meta[r][0]), int(meta[r][1]))
        if not (slot[r] == 0):                           # NaN != 0: marked
            marked_from.setdefault(key, r)
        if key not in marked_from:
            out.append(r)
    return out


def append(level, db_rows, meta=None, feat=None, off=None):
    """(kept, the DB's rows after the append as an array [n][width]); columns bit for bit"""
    feat = np.asarray(feat, np.float64)
    k = keep(level, meta, feat, off)
    new = feat[k, :WIDTH[level]] if len(k) else np.zeros((0, WIDTH[level]))
    return np.array(k, np.int32), np.concatenate([db_rows, new]) if len(db_rows) else new.copy()


def ranges(rows):
    """per column (min, max) over rows [n][width]: NaN for both where the column holds a NaN, else exact with -0 below +0"""
    rows = np.asarray(rows, np.float64)
    mn, mx = np.zeros(rows.shape[1]), np.zeros(rows.shape[1])
    for k in range(rows.shape[1]):
        col = rows[:, k]
        if np.isnan(col).any():
            mn[k] = mx[k] = np.nan
            continue
        lo, hi = col.min(), col.max()
        if lo == 0 and np.signbit(col[col == 0]).any():
            lo = -0.0
        if hi == 0:
            hi = -0.0 if np.signbit(col[col == 0]).all() else 0.0
        mn[k], mx[k] = lo, hi
    return mn, mx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
