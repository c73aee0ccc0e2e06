"""A Python restatement of the device half of specification DS-1 (DESIGN.md §3, K8 in csrc/dbstats.hip): the decision over a row's
probabilities and the results table's counters, with the chunked order of every f64 sum (rows of a chunk of R consecutive rows in row
order, then chunks in chunk order).  Plain loops over numpy scalars: every addition is one IEEE double operation, as on the device."""
import numpy as np

R = 256                       # WSA_DBSTATS_CHUNK_ROWS
CAT = np.dtype([("correct", "<u8"), ("wrong", "<u8"), ("blank", "<u8")])
CLASS = np.dtype([("count", "<u8"), ("correct", "<u8"), ("wrong", "<u8"), ("duration", "<f8"), ("first_row", "<u4"), ("reserved", "<u4")])
ORD = np.dtype([("true_n", "<u8"), ("pred_n", "<u8"), ("min", "<f8"), ("max", "<f8"), ("sq_sum", "<f8")])


def decide(prob, legend_to_vocab):
    """[n][C] f32 -> [n] i32: `>` in legend order against a maximum that starts at 0 (ref neuralmodel.js nn_db_results_handler over ml5's
    stably sorted result); NaN never wins; -1 is the reference's null."""
    prob = np.asarray(prob, np.float32)
    out = np.full(len(prob), -1, np.int32)
    for r, row in enumerate(prob):
        best, top = np.float32(0), -1
        for c, p in enumerate(row):
            if p > best:
                best, top = p, c
        out[r] = legend_to_vocab[top] if top >= 0 else -1
    return out


def counted(v):
    """the reference's "truthy and not NaN" of an ordinal value"""
    return v == v and v != 0.0


def table(durations, cats, ords, chunk_rows=R):
    """cats: [(V, true_idx [n], pred_idx [n])], ords: [(true_value [n], pred_value [n])] -> (cat, cls, ord) records as
    capi.FeatureDBStats.table returns them."""
    dur = np.asarray(durations, np.float64)
    n = len(dur)
    chunks = [(a, min(a + chunk_rows, n)) for a in range(0, n, chunk_rows)]
    cat, od = np.zeros(len(cats), CAT), np.zeros(len(ords), ORD)
    cls = np.zeros(sum(V for V, _, _ in cats), CLASS)
    off = 0
    for h, (V, t_idx, p_idx) in enumerate(cats):
        t_idx, p_idx = np.asarray(t_idx, np.int64), np.asarray(p_idx, np.int64)
        total = np.zeros(V, np.float64)
        first = np.full(V, 0xFFFFFFFF, np.uint64)
        for a, b in chunks:
            part = np.zeros(V, np.float64)                  # every entry's partial starts at +0 in every chunk
            for i in range(a, b):
                v = t_idx[i]
                if v < 0:
                    continue
                e = cls[off + v]
                if first[v] == 0xFFFFFFFF:
                    first[v] = i
                e["count"] += 1
                part[v] = part[v] + dur[i]
                if p_idx[i] >= 0:
                    e["correct" if p_idx[i] == v else "wrong"] += 1
            total = total + part                            # chunk order; entries without a row in the chunk add +0
        cls["duration"][off:off + V] = total
        cls["first_row"][off:off + V] = first
        sl = cls[off:off + V]
        cat[h] = (sl["correct"].sum(), sl["wrong"].sum(), sl["count"].sum() - sl["correct"].sum() - sl["wrong"].sum())
        off += V
    for o, (t_val, p_val) in enumerate(ords):
        t_val, p_val = np.asarray(t_val, np.float64), np.asarray(p_val, np.float64)
        true_n = pred_n = 0
        mn, mx, sq = np.float64(np.inf), np.float64(0.0), np.float64(0.0)
        for a, b in chunks:
            part = np.float64(0.0)
            for i in range(a, b):
                t = t_val[i]
                if not counted(t):
                    continue
                true_n += 1
                mn, mx = (t if t < mn else mn), (t if t > mx else mx)
                p = p_val[i]
                if counted(p):
                    pred_n += 1
                    d = p - t
                    part = part + d * d
            sq = sq + part
        od[o] = (true_n, pred_n, mn, mx, sq)
    return cat, cls, od


def in_order_sums(durations, cats, ords):
    """the reference's own plain in-order sums (localstore.js:534, 596) and the sum of |terms| the summation bound needs:
    ([per head: (duration [V], abs [V])], [per head: (sq_sum, abs)])"""
    dur = np.asarray(durations, np.float64)
    out_c, out_o = [], []
    for V, t_idx, _ in cats:
        s, a = np.zeros(V), np.zeros(V)
        for i, v in enumerate(t_idx):
            if v >= 0:
                s[v] = s[v] + dur[i]
                a[v] = a[v] + abs(dur[i])
        out_c.append((s, a))
    for t_val, p_val in ords:
        s = np.float64(0.0)
        for t, p in zip(np.asarray(t_val, np.float64), np.asarray(p_val, np.float64)):
            if counted(t) and counted(p):
                s = s + (p - t) * (p - t)
        out_o.append((float(s), float(s)))                  # the terms are squares: the sum of their magnitudes is the sum itself
    return out_c, out_o


def sum_bound(n_terms, abs_sum):
    """|chunked - in-order| <= 2 (n - 1) 2^-53 sum|terms|: each order is within (n - 1) u sum|terms| of the exact sum (DS-1)."""
    return 2.0 * max(n_terms - 1, 0) * 2.0 ** -53 * abs_sum
