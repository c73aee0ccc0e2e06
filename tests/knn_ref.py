"""A numpy restatement of specification KN-1: the app's ml5 KNN classifier (ref src/neuralmodel.js:729-837 over
dist/ml5.min.js addExample / similarities / predictClass / calculateTopClass).  Test helper.

similarities() is the exact figure — rows rounded to f32 as ml5's tensors are, cosines in float64 — that both tfjs's f32 matMul and the
device's f32 MFMA chain approximate.  select() is everything after the similarities, and it is exact: given the same similarities it
must give the same neighbours, votes, confidences and label, bit for bit.

For the hand-built exact rows of tests/knn_exact_cases.py: exact_similarities() is the similarity from integers, which the device and ml5
must both give bit for bit, and stream_select() replays the device's own streamed selection (csrc/knn.hip) with every arm counted.
"""
from collections import Counter

import numpy as np

from webspeechanalyzer_amd.knn import label_order


def similarities(store, queries):
    """[q, n] float64 cosines of the f32-rounded rows"""
    a = np.asarray(store, np.float64).astype(np.float32).astype(np.float64)
    b = np.asarray(queries, np.float64).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = a / np.sqrt((a * a).sum(axis=1))[:, None]
        b = b / np.sqrt((b * b).sum(axis=1))[:, None]
    return b @ a.T


def grouped_rank(class_index):
    """a row's position in ml5's train matrix: the per-class matrices concatenated in class order, insertion order inside a class"""
    class_index = np.asarray(class_index)
    order = np.argsort(class_index, kind="stable")
    rank = np.empty(len(class_index), np.int64)
    rank[order] = np.arange(len(class_index))
    return rank


def select(sim, class_index, n_classes, k):
    """The selection and the vote on given similarities sim [q, n] (any float type): k_eff = min(k, n); neighbours by similarity
    descending, then grouped rank ascending (tfjs topk is a stable descending sort over the grouped matrix); a NaN similarity is lower
    than every number and ranks decide among NaNs (the device's rule: ml5 is not pinned there); confidence = votes / k_eff in double; the
    label is the first class whose confidence exceeds a maximum that starts at 0.
    -> dict(nbr [q, k_eff] insertion indices in selection order, conf [q, C] f64, label [q], stats)"""
    sim = np.asarray(sim)
    class_index = np.asarray(class_index)
    q, n = sim.shape
    k_eff = min(int(k), n)
    rank = grouped_rank(class_index)
    nbr = np.zeros((q, k_eff), np.int64)
    conf = np.zeros((q, n_classes), np.float64)
    label = np.zeros(q, np.int64)
    stats = dict(clamped=int(k_eff < k), rank_ties=0, vote_ties=0, vote_tie_not_top=0)
    for i in range(q):
        key = np.where(np.isnan(sim[i]), -np.inf, sim[i].astype(np.float64))
        order = np.lexsort((rank, -key))
        top = order[:k_eff]
        nbr[i] = top
        if k_eff < n and key[order[k_eff - 1]] == key[order[k_eff]]:
            stats["rank_ties"] += 1                                   # the grouped rank decided who is in
        votes = np.bincount(class_index[top], minlength=n_classes)
        conf[i] = votes / float(k_eff)
        best, mx = -1, 0.0
        for c in range(n_classes):
            if conf[i, c] > mx:
                best, mx = c, conf[i, c]
        label[i] = best
        if (votes == votes.max()).sum() > 1:
            stats["vote_ties"] += 1
            if class_index[top[0]] != best:
                stats["vote_tie_not_top"] += 1
    return dict(nbr=nbr, conf=conf, label=label, stats=stats)


def classify(store, labels, queries, k, sim=None):
    """KN-1 end to end: label_order, the exact similarities (or the given ones), the selection.  Adds `classes` (ml5's label per class)
    and `labels` (the predicted label per query)."""
    classes, index = label_order(labels)
    s = similarities(store, queries) if sim is None else sim
    out = select(s, index, len(classes), k)
    out.update(classes=classes, index=index, sim=s, labels=[classes[c] for c in out["label"]])
    return out


class RefKnn:
    """The restatement behind the interface of webspeechanalyzer_amd.knn.Knn, for knn.evaluate(make_knn=...)"""

    def __init__(self, width, capacity):
        self.width, self.rows, self.labels = width, np.zeros((0, width)), []

    def add(self, rows, labels):
        self.rows = np.concatenate([self.rows, np.asarray(rows, np.float64).reshape(-1, self.width)])
        self.labels += list(labels)

    def classify(self, rows, k=10):
        r = classify(self.rows, self.labels, np.asarray(rows, np.float64).reshape(-1, self.width), k)
        return dict(label=r["labels"], index=r["label"], conf=r["conf"], nbr=r["nbr"], classes=r["classes"])


# ---- The device's own form (csrc/knn.hip), replayed step by step with every comparison counted in KNN_ARMS (as classify_ref.FOLD_ARMS
# and peak_ref.ARMS are): exact rows, whose similarities are integers over powers of two, and the streamed selection — tiles of T store
# rows, blocks of BLOCK, the pass order (i, then lane), `key >= thr` against the threshold read at the block's start, knn_insert with its
# outcomes, the re-read after a walked block, K9s's partial lists and their merge.  `fault` turns one line into a plausible wrong one
# (FAULTS); tests/test_knn_exact_reference.py shows that each changes the output of a case of tests/knn_exact_cases.py.

T, QT, BLOCK, MAX_K, MAX_CLASSES = 64, 64, 16, 64, 64
HOTS = {1: 0, 4: 1, 16: 2, 64: 3, 256: 4}          # non-zeros of an exact row -> m: its unit row holds 0 and +-2^-m

KNN_ARMS = Counter()
KNN_ARM_NAMES = (
    # knn_add_kernel, knn_within_kernel, knn_rank_kernel
    "add.class_ok", "add.class_below", "add.class_above",
    "within.first", "within.call_carry", "within.chunk_carry",      # a class's first row of a 64-row chunk: count 0 / rows of earlier calls / of earlier chunks of this call
    "rank.none_moved", "rank.some_moved", "rank.all_moved",         # what a later add does to the ranks of the rows already stored
    # the query grid and the store's tiles
    "qtile.full", "qtile.partial", "grid.first_trip", "grid.second_trip",
    "tile.full", "tile.partial", "tile.one_row", "tile.only_last_block",
    # the pass test of one (query, store row) pair
    "key.number", "key.nan",
    "pass.above", "pass.equal", "pass.below", "reread.refuses",     # reread.refuses: below the threshold now, not below the one the tile began with
    "cv.refuses_filling", "cv.refuses_full", "cv.idle",             # a padding row of the last tile: would pass (list filling / full), would not
    "block.skipped", "block.walked", "block.one_i", "block.several_i",
    # knn_insert
    "insert.filling", "insert.fills", "insert.full_first", "insert.full_middle", "insert.full_last",
    "insert.refused_equal", "insert.refused_stale",
    "thr.ck", "thr.up", "up.index_0", "up.index_k_minus_2",
    "tie.behind", "tie.ahead", "kth.displaced_equal", "nan.pushed_out",
    "keff.1", "keff.2", "keff.63", "keff.64", "keff.other",
    # knn_epilogue
    "vote.unique", "vote.tie_top", "vote.tie_not_top", "vote.tie_three", "label.class_63", "classes.one", "classes.several",
    "clamp.k_above_n", "clamp.none", "sim.nan", "sim.number",
    # K9s: slices and knn_merge_kernel
    "slice.rows", "slice.empty", "slice.short", "slice.full",
    "merge.pass", "merge.pass_refuses", "merge.refused_stale", "merge.refused_equal", "merge.tie_ahead", "merge.tie_behind", "merge.nan",
)
# arms of the device form that no input reaches, with the argument (as tracker_rule_cases.UNREACHABLE)
UNREACHABLE = {
    "stale.other_i": "a query's four thresholds sit in ONE register slot: query 16 wave + 4 (lane >> 4) + i is read by thr[i] alone, so two "
                     "candidates of one query always share i (and differ in lane & 15); passes at several i are several queries (block.several_i)",
    "stale.other_block": "thr[] is re-read from s_thr after every walked block, so a candidate of a later block meets the raised threshold in "
                         "the pass test (reread.refuses), never inside knn_insert; only a candidate of the SAME block can be stale",
}
FAULTS = {
    "pass_gt": "`key[i] > thr[i]` for `>=` in the pass test",
    "merge_pass_gt": "`ck > s_thr[w]` for `>=` in the merge's pass test",
    "rank_gt": "`er > crank` for `er < crank` in knn_insert",
    "thr_ck_always": "`s_thr[q] = ck` whatever pos is",
    "shift_le": "the shift bound `lane + 1 <= k_eff`",
    "cv_dropped": "`cv &&` dropped from the pass test",
    "nan_pos_inf": "a NaN similarity keyed as +inf",
    "sim_nan_dropped": "`key != NEG_INF` dropped: sim written as the key",
    "vote_key_lane": "vote key `lane` for `63 - lane`",
    "conf_over_k": "`votes / k` for `votes / k_eff`",
    "within_no_carry": "knn_within_kernel without the chunk's carry (`mine` as the call began)",
    "rank_no_soff": "knn_rank_kernel without s_off",
    "merge_reads_empty": "the merge reading a slice that holds no rows",
    "no_list_reset": "s_cnt / s_thr not reset on a workgroup's second trip through the query tiles",
}
# one-line changes that cannot show in the output, with the argument; the test asserts that they do not, and what they do change
EQUIVALENT = {
    "rank_le": "`er <= crank`: ranks are unique and no row reaches a list twice, so er == crank never happens",
    "no_reread": "the threshold not re-read after a block: a stale threshold only lets candidates through to knn_insert, which refuses them by "
                 "position (pos >= k_eff); the output stands, reread.refuses becomes insert.refused_stale",
}
_POISON = (np.float32(2.0), -5, -5)                # what a scratch entry that no workgroup wrote is taken to hold (key, rank, index)


def exact_similarities(store, queries):
    """[q, n] f32 similarities of exact rows, from integers: a row rounded to f32 holds 0 and +-2^e at 1, 4, 16, 64 or 256 places (asserted),
    so its unit row holds +-2^-m (4^m places) and a similarity is overlap / 2^(m1 + m2), overlap the sum of the sign products — what any
    f32 summation of the products gives, in any order, fused or not.  A row of zeros has no unit row: its similarities are NaN."""
    def decode(rows):
        x = np.asarray(rows, np.float64).astype(np.float32).astype(np.float64)
        sign = np.sign(x).astype(np.int64)
        m = np.zeros(len(x), np.int64)
        zero = np.zeros(len(x), bool)
        for r, row in enumerate(x):
            nz = np.nonzero(row)[0]
            if not len(nz):
                zero[r] = True
                continue
            mant, e = np.frexp(np.abs(row[nz]))
            assert (mant == 0.5).all() and (e == e[0]).all() and -60 <= e[0] <= 60, f"row {r}: entries must be 0 or +-2^e"
            assert len(nz) in HOTS, f"row {r}: {len(nz)} non-zeros, not one of {sorted(HOTS)}"
            m[r] = HOTS[len(nz)]
        return sign, m, zero
    ss, ms, zs = decode(store)
    sq, mq, zq = decode(queries)
    sim = np.ldexp((sq @ ss.T).astype(np.float64), -(mq[:, None] + ms[None, :])).astype(np.float32)
    sim[zq, :] = np.nan
    sim[:, zs] = np.nan
    return sim


def store_ranks(class_index, n_classes, adds=None, fault=None):
    """knn_add_kernel's class clamp, knn_within_kernel and knn_rank_kernel over a sequence of add calls (`adds`: rows per call; None: one
    call).  -> dict(cls, within, rank [n], counts [n_classes], bad: wsa_knn_count's `row + 1` of the worst call-local row, 0 if none)"""
    ci = np.asarray(class_index, np.int64)
    n = len(ci)
    adds = [n] if adds is None else [int(a) for a in adds]
    assert sum(adds) == n and all(a > 0 for a in adds)
    A = Counter()
    cls, within, rank = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    count, bad, base = [0] * MAX_CLASSES, 0, 0
    for na in adds:
        for r in range(na):
            c = int(ci[base + r])
            A["add.class_below" if c < 0 else "add.class_above" if c >= n_classes else "add.class_ok"] += 1
            if c < 0 or c >= n_classes:
                bad, c = max(bad, r + 1), 0
            cls[base + r] = c
        start, mine = list(count), list(count)
        for r0 in range(0, na, 64):
            chunk = cls[base + r0:base + min(r0 + 64, na)]
            before = list(start if fault == "within_no_carry" else mine)
            seen = Counter()
            for lane, c in enumerate(int(c) for c in chunk):
                if not seen[c]:
                    A["within.chunk_carry" if mine[c] > start[c] else "within.call_carry" if start[c] else "within.first"] += 1
                within[base + r0 + lane] = before[c] + seen[c]
                seen[c] += 1
            for c, v in seen.items():
                mine[c] += v
        count, total = mine, base + na
        off = np.concatenate([[0], np.cumsum(count)[:-1]])
        old = rank[:base].copy()
        rank[:total] = (0 if fault == "rank_no_soff" else off[cls[:total]]) + within[:total]
        if base:
            moved = rank[:base] != old
            A["rank.all_moved" if moved.all() else "rank.some_moved" if moved.any() else "rank.none_moved"] += 1
        base = total
    KNN_ARMS.update(A)
    return dict(cls=cls, within=within, rank=rank, counts=count[:n_classes], bad=bad, arms=A)


class _Lists:
    """the lists of one workgroup as they lie in LDS: entry j of query q at q * MAX_K + j, so a write one past a list's end lands in
    the next query's first entry (the last query's in a spill row nobody reads)"""

    def __init__(self):
        self.key = np.full((QT + 1) * MAX_K, np.nan, np.float32)
        self.rk = np.full((QT + 1) * MAX_K, -7, np.int64)
        self.ix = np.full((QT + 1) * MAX_K, -7, np.int64)
        self.thr = np.full(QT, -np.inf, np.float32)
        self.cnt = np.zeros(QT, np.int64)

    def reset(self, nq):
        self.cnt[:] = 0
        self.thr[:nq] = -np.inf
        self.thr[nq:] = np.inf                     # rows past the end take no part


_LANES = np.arange(MAX_K)


def _insert(L, q, ck, cidx, crank, k_eff, fault, A, merge=False):
    """knn_insert.  Counts its outcome; -> True if the candidate went in"""
    cnt, b = int(L.cnt[q]), q * MAX_K
    if fault is None and cnt == k_eff:
        # a short cut for the replay's speed, not a device form: without a fault the list is sorted, so every entry beats the candidate
        # exactly when the last one does, and an entry equal to it can only be that last one's run
        lk, lr = L.key[b + k_eff - 1], L.rk[b + k_eff - 1]
        if lk > ck or (lk == ck and lr < crank):
            if lk == ck:
                A["merge.tie_behind" if merge else "tie.behind"] += 1
            A[("merge." if merge else "insert.") + ("refused_stale" if ck < L.thr[q] else "refused_equal")] += 1
            return False
    ek, er, ei = L.key[b:b + MAX_K].copy(), L.rk[b:b + MAX_K].copy(), L.ix[b:b + MAX_K].copy()
    valid = _LANES < cnt
    by_rank = er <= crank if fault == "rank_le" else er > crank if fault == "rank_gt" else er < crank
    with np.errstate(invalid="ignore"):
        equal = valid & (ek == ck)
        beats = valid & ((ek > ck) | (equal & by_rank))
    pos = int(beats.sum())
    if (equal & beats).any():
        A["merge.tie_behind" if merge else "tie.behind"] += 1
    if (equal & ~beats).any():
        A["merge.tie_ahead" if merge else "tie.ahead"] += 1
    if pos >= k_eff:
        stale = ck < L.thr[q]
        A[("merge." if merge else "insert.") + ("refused_stale" if stale else "refused_equal")] += 1
        return False
    if cnt == k_eff:
        if ek[k_eff - 1] == ck:
            A["kth.displaced_equal"] += 1
        if ek[k_eff - 1] == -np.inf and ck > -np.inf:
            A["nan.pushed_out"] += 1
    bound = k_eff + 1 if fault == "shift_le" else k_eff
    for lane in np.nonzero(valid & (_LANES >= pos) & (_LANES + 1 < bound))[0]:
        L.key[b + lane + 1], L.rk[b + lane + 1], L.ix[b + lane + 1] = ek[lane], er[lane], ei[lane]
    ncnt = min(cnt + 1, k_eff)
    up = ek[k_eff - 2 if k_eff >= 2 else 0]
    A["up.index_k_minus_2" if k_eff >= 2 else "up.index_0"] += 1
    L.key[b + pos], L.rk[b + pos], L.ix[b + pos], L.cnt[q] = ck, crank, cidx, ncnt
    if ncnt == k_eff:
        last = pos == k_eff - 1
        L.thr[q] = ck if last or fault == "thr_ck_always" else up
        A["thr.ck" if last else "thr.up"] += 1
    if not merge:
        A["insert.filling" if cnt + 1 < k_eff else "insert.fills" if cnt < k_eff else
          "insert.full_last" if pos == k_eff - 1 else "insert.full_first" if pos == 0 else "insert.full_middle"] += 1
        A["keff.%d" % k_eff if k_eff in (1, 2, 63, 64) else "keff.other"] += 1
    return True


def _epilogue(L, ql, cls_ext, C, k, k_eff, fault, A, out, q):
    b = ql * MAX_K
    idx, key = L.ix[b:b + k_eff], L.key[b:b + k_eff]
    votes = np.bincount(cls_ext[np.clip(idx, 0, len(cls_ext) - 1)], minlength=MAX_CLASSES)
    lanes = np.arange(C)
    if fault == "vote_key_lane":
        label = int(((votes[:C] << 6) | lanes).max() & 63)
    else:
        label = 63 - int(((votes[:C] << 6) | (63 - lanes)).max() & 63)
    tied = int((votes[:C] == votes[:C].max()).sum())
    A["vote.unique" if tied == 1 else "vote.tie_top" if cls_ext[np.clip(idx[0], 0, len(cls_ext) - 1)] == label else "vote.tie_not_top"] += 1
    if tied >= 3:
        A["vote.tie_three"] += 1
    if label == 63:
        A["label.class_63"] += 1
    A["classes.one" if C == 1 else "classes.several"] += 1
    A["clamp.k_above_n" if k_eff < k else "clamp.none"] += 1
    out["label"][q] = label
    out["conf"][q] = votes[:C] / float(k if fault == "conf_over_k" else k_eff)
    out["nbr"][q, :k_eff] = idx
    nan = key == -np.inf
    A["sim.nan"] += int(nan.sum())
    A["sim.number"] += int((~nan).sum())
    out["sim"][q, :k_eff] = key if fault == "sim_nan_dropped" else np.where(nan, np.float32(np.nan), key)


def _walk(L, sim, q0, nq, lo, hi, n, rank, k_eff, fault, A):
    """knn_body's store loop for the query tile q0 .. q0 + nq - 1 over the store rows lo .. hi - 1 (whole tiles but for the store's end)"""
    key_all = np.where(np.isnan(sim[q0:q0 + nq]), np.float32(np.inf if fault == "nan_pos_inf" else -np.inf), sim[q0:q0 + nq])
    pad_key = np.where(np.isnan(sim[q0:q0 + nq]).all(axis=1), np.float32(np.inf if fault == "nan_pos_inf" else -np.inf), np.float32(0.0))
    A["key.nan"] += int(np.isnan(sim[q0:q0 + nq, lo:hi]).sum())
    A["key.number"] += int((~np.isnan(sim[q0:q0 + nq, lo:hi])).sum())
    thr = L.thr.copy()                                        # the registers: read after the queries' unit rows are in place
    for t0 in range(lo, hi, T):
        rows = min(T, n - t0)
        A["tile.full" if rows == T else "tile.one_row" if rows == 1 else "tile.partial"] += 1
        key = np.empty((nq, T), np.float32)
        key[:, :rows] = key_all[:, t0:t0 + rows]
        key[:, rows:] = pad_key[:, None]
        trank = np.zeros(T, np.int64)
        trank[:rows] = rank[t0:t0 + rows]
        thr_tile = L.thr.copy()
        for wave in range((nq + 15) // 16):
            w0, w1 = wave * 16, min(wave * 16 + 16, nq)
            walked = []
            for cb in range(T // BLOCK):
                c0 = cb * BLOCK
                cv = t0 + c0 + np.arange(BLOCK) < n
                k_ = key[w0:w1, c0:c0 + BLOCK]
                th = thr[w0:w1, None]
                ge = k_ >= th if fault not in ("pass_gt",) else k_ > th
                full = (L.cnt[w0:w1] == k_eff)[:, None]
                A["pass.above"] += int((cv & (k_ > th)).sum())
                A["pass.equal"] += int((cv & (k_ == th)).sum())
                A["pass.below"] += int((cv & (k_ < th)).sum())
                A["reread.refuses"] += int((cv & (k_ < th) & (k_ >= thr_tile[w0:w1, None])).sum())
                A["cv.refuses_full"] += int((~cv & ge & full).sum())
                A["cv.refuses_filling"] += int((~cv & ge & ~full).sum())
                A["cv.idle"] += int((~cv & ~ge).sum())
                ps = ge if fault == "cv_dropped" else ge & cv
                if not ps.any():
                    A["block.skipped"] += 1
                    continue
                A["block.walked"] += 1
                walked.append(cb)
                A["block.one_i" if len({int(r) % 4 for r in np.nonzero(ps.any(axis=1))[0]}) == 1 else "block.several_i"] += 1
                for i in range(4):                            # the pass order: i, then lane = 16 (query row / 4) + store row of the block
                    for g in range(4):
                        r = 4 * g + i
                        if r >= w1 - w0:
                            continue
                        for c in np.nonzero(ps[r])[0]:
                            tl = c0 + int(c)
                            _insert(L, w0 + r, key[w0 + r, tl], t0 + tl, int(trank[tl]), k_eff, fault, A)
                if fault != "no_reread":
                    thr[w0:w1] = L.thr[w0:w1]
            if walked == [T // BLOCK - 1]:
                A["tile.only_last_block"] += 1


def stream_select(sim, class_index, k, slices=None, *, n_classes=None, adds=None, grid=None, fault=None):
    """K9 (slices None) or K9s (`slices` slices) on given f32 similarities sim [q, n], in the device's own form.  grid: workgroups of
    the K9 launch (None: one per query tile; fewer: a workgroup takes tile b, b + grid, ...).  -> dict(label [q] i32, conf [q, C] f64,
    nbr [q, k] i32 with -1 past k_eff, sim [q, k] f32 with NaN past k_eff and for NaN similarities, rank, bad, arms) — the four tables
    as wsa_knn_classify_rows writes them."""
    sim = np.asarray(sim, np.float32)
    q, n = sim.shape
    C = int(n_classes if n_classes is not None else max(int(np.max(class_index)) + 1, 1))
    assert 1 <= k <= MAX_K and n >= 1 and 1 <= C <= MAX_CLASSES
    st = store_ranks(class_index, C, adds, fault)
    A = Counter()
    rank, k_eff = st["rank"], min(int(k), n)
    tiles, q_tiles = (n + T - 1) // T, (q + QT - 1) // QT
    cls_ext = np.concatenate([st["cls"], np.zeros(tiles * T - n + 1, np.int64)])
    out = dict(label=np.full(q, -9, np.int32), conf=np.full((q, C), -9.0), nbr=np.full((q, k), -1, np.int32), sim=np.full((q, k), np.nan, np.float32))
    if slices is None:
        grid = q_tiles if grid is None else min(int(grid), q_tiles)
        for b in range(grid):
            L = _Lists()
            for trip, qt in enumerate(range(b, q_tiles, grid)):
                q0, nq = qt * QT, min(QT, q - qt * QT)
                A["qtile.full" if nq == QT else "qtile.partial"] += 1
                A["grid.second_trip" if trip else "grid.first_trip"] += 1
                if not (trip and fault == "no_list_reset"):
                    L.reset(nq)
                _walk(L, sim, q0, nq, 0, n, n, rank, k_eff, fault, A)
                for ql in range(nq):
                    _epilogue(L, ql, cls_ext, C, k, k_eff, fault, A, out, q0 + ql)
    else:
        per = max(1, (tiles + slices - 1) // slices) * T
        scratch = {}
        for qt in range(q_tiles):
            q0, nq = qt * QT, min(QT, q - qt * QT)
            A["qtile.full" if nq == QT else "qtile.partial"] += 1
            for sl in range(slices):
                lo, hi = sl * per, min(n, (sl + 1) * per)
                if lo >= n:
                    A["slice.empty"] += 1
                    continue
                A["slice.rows"] += 1
                L = _Lists()
                L.reset(nq)
                _walk(L, sim, q0, nq, lo, hi, n, rank, k_eff, fault, A)
                for ql in range(nq):
                    c, b = int(L.cnt[ql]), ql * MAX_K
                    scratch[q0 + ql, sl] = (L.key[b:b + c].copy(), L.rk[b:b + c].copy(), L.ix[b:b + c].copy())
        for qi in range(q):                                   # knn_merge_kernel: one wave per query, its lists in slice order
            L = _Lists()
            L.reset(1)
            for sl in range(slices):
                if sl * per >= n and fault != "merge_reads_empty":
                    continue
                keys, rks, ixs = scratch.get((qi, sl), ([_POISON[0]], [_POISON[1]], [_POISON[2]]))
                A["slice.short" if len(keys) < k_eff else "slice.full"] += 1
                thr = L.thr[0]
                for ck, cr, cx in zip(keys, rks, ixs):
                    if ck == -np.inf:
                        A["merge.nan"] += 1
                    if ck > thr if fault == "merge_pass_gt" else ck >= thr:
                        A["merge.pass"] += 1
                        _insert(L, 0, ck, int(cx), int(cr), k_eff, fault, A, merge=True)
                    else:
                        A["merge.pass_refuses"] += 1
            _epilogue(L, 0, cls_ext, C, k, k_eff, fault, A, out, qi)
    KNN_ARMS.update(A)                                        # store_ranks has counted its own
    A.update(st["arms"])
    out.update(rank=rank, cls=st["cls"], bad=st["bad"], counts=st["counts"], arms=A)
    return out
