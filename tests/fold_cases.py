"""Hand-built rows for the class fold K6b / K6b-e (csrc/classify_fold.hpp), and the tables that carry them to the test entry
wsa_debug_class_fold (tests/test_gpu_fold.py) and to the reference's own src/prediction.js (tests/golden/gen/make_fold_golden.py,
tests/test_fold_reference.py).  No audio and no model: a case is ONE launch of the app, a list of callbacks, each a list of syllables with
their length t_len (the duration is parseFloat(((t_len + 1) * step_s).toFixed(3))) and, per member of the ensemble, one row of
confidences.  Each case sits on one equality of the fold from both sides; together they reach every arm classify_ref.FOLD_ARMS counts.

Confidences are exact in the type the case names: "f32" cases hold float32 values (K6's probabilities; they also run through the double
kernels, a float being a double), "f64" cases hold doubles a float cannot (KNN's votes / k) and run through fold_kernel<double> /
stream_knn_kernel only.

Rows that mix NaN with numbers are left out on purpose: ml5 sorts with `b.confidence - a.confidence`, an inconsistent comparator on such a
row, so V8's order is unspecified — and K6 cannot produce one (a non-finite feature makes the whole softmax row NaN).
classify_ref.classify_multiple refuses them."""
import numpy as np

from tests import classify_ref, ensemble_ref

NAN = float("nan")
NASH = ["N", "A", "S", "H"]
IDX4 = ["0", "1", "2", "3"]


def f32(rows):
    return np.asarray(rows, np.float32).astype(np.float64)


def _rand_rows(seed, n, C):
    """n rows of C distinct softmax-like float32 confidences"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, C))
    return f32(np.exp(x) / np.exp(x).sum(1, keepdims=True))


def _cb(t_len, *conf, dtype="f32"):
    """one callback: t_len per syllable, conf[d] [n_syl][C_d] per member"""
    return dict(t_len=[int(t) for t in t_len],
                conf=[f32(c) if dtype == "f32" else np.asarray(c, np.float64) for c in conf])


def _case(name, step_s, legends, callbacks, dtype="f32"):
    for cb in callbacks:
        assert len(cb["conf"]) == len(legends)
        for leg, c in zip(legends, cb["conf"]):
            assert c.shape == (len(cb["t_len"]), len(leg)), (name, c.shape)
    return dict(name=name, step_s=step_s, legends=[list(l) for l in legends], callbacks=callbacks, dtype=dtype)


def _named_cases():
    out = []
    R = _rand_rows(11, 40, 4)
    R2 = _rand_rows(12, 40, 2)

    # ---- fixed3 on its ties.  5 x 0.0125 is the double 0.0625 exactly: "0.063" (the larger n on a tie); 4 and 6 round down / up plainly
    out.append(_case("fixed3-ties-12.5ms", 0.0125, [NASH], [
        _cb([3], R[0:1]), _cb([4], R[1:2]), _cb([5], R[2:3]), _cb([3, 4, 5], R[3:6]), _cb([4, 4], R[6:8])]))
    # 0.1 ms: 4 steps are "0.000" (a lone syllable: the callback is skipped), 5 steps sit beside 0.0005 (no double is 0.0005), 6 are "0.001"
    out.append(_case("fixed3-ties-0.1ms", 0.0001, [NASH], [
        _cb([3], R[8:9]), _cb([4], R[9:10]), _cb([5], R[10:11]), _cb([3, 4, 5], R[11:14]), _cb([3, 3], R[14:16]), _cb([9], R[16:17]),
        # 95 and 115 steps: the double 1000 * x ROUNDS to 9.5 / 11.5 from below, so floor(1000 x + 0.5) alone would answer "0.010" / "0.012";
        # the exact value is under the tie: "0.009" / "0.011" (what fixed3's fma correction is for)
        _cb([94], R[17:18]), _cb([94, 114, 104], R[18:21])]))

    # ---- a skipped callback (label -2 for every member) between two real ones: nothing is inserted, nothing else moves
    out.append(_case("skip-then-count", 0.0001, [NASH, ["x", "y"]], [
        _cb([99, 149], R[0:2], R2[0:2]), _cb([0, 1, 2], R[2:5], R2[2:5]), _cb([199], R[5:6], R2[5:6]), _cb([3], R[6:7], R2[6:7]),
        _cb([120, 80, 99], R[7:10], R2[7:10])]))

    # ---- `if(!acc[l]) acc[l] = w; else acc[l] += w` on a present 0: N and H enter both accumulators with 0 in the first syllable (keys in
    # Object.keys order A, S, N, H), the second syllable ASSIGNS; then the launch sum of H is a present 0 while the segment's is absent; the
    # last callback ties N and H exactly: N, inserted earlier by its zero, takes it
    out.append(_case("present-zero", 0.0125, [NASH], [
        _cb([7, 7], [[0, 0.75, 0.25, 0], [0.5, 0.25, 0.25, 0]]),
        _cb([7], [[0, 0.125, 0.125, 0.75]]),
        _cb([9, 9], [[0.5, 0.0625, 0.0625, 0.375], [0.375, 0.0625, 0.0625, 0.5]])]))
    # the same on a present NaN: an all-NaN first syllable leaves NaN under every key, the second syllable assigns; then a lone all-NaN
    # syllable leaves NaN under N in the launch sums only, and the next callback's N assigns there while its segment sum starts absent
    nan4 = [[NAN] * 4]
    out.append(_case("present-nan", 0.0125, [NASH], [
        _cb([7, 7], np.vstack([nan4, R[20:21]])),
        _cb([7], R[21:22]),
        _cb([7], nan4),
        _cb([5, 6], [[0.5, 0.25, 0.125, 0.125], [0.625, 0.125, 0.125, 0.125]])]))

    # ---- all confidences 0: label null (-1), confidence 0, and the keys are inserted all the same (one key for a lone syllable)
    z4, z2 = np.zeros((1, 4)), np.zeros((1, 2))
    out.append(_case("all-zero-row", 0.0125, [NASH, ["x", "y"]], [
        _cb([7], z4, z2), _cb([7, 3], np.vstack([z4, z4]), np.vstack([z2, z2])), _cb([7], R[22:23], R2[22:23]),
        _cb([4, 4], np.vstack([z4, R[23:24]]), np.vstack([z2, R2[23:24]]))]))

    # ---- a row that is NaN throughout (K6's answer to a non-finite feature): ml5's sort leaves it in legend order, so a lone syllable adds
    # NaN under the FIRST legend label only; several syllables add NaN under every label, inserted in legend order
    out.append(_case("all-nan-row-single", 0.0125, [NASH], [_cb([7], nan4), _cb([7], R[24:25]), _cb([3, 3], R[25:27])]))
    out.append(_case("all-nan-row-single-index", 0.0125, [["10", "2", "x", "0"]], [_cb([7], nan4), _cb([3, 3], R[25:27]), _cb([7], nan4)]))
    out.append(_case("all-nan-row-multi", 0.0125, [NASH], [_cb([7, 5], np.vstack([nan4, nan4])), _cb([7], R[27:28]), _cb([3, 3], R[28:30])]))
    out.append(_case("all-nan-row-ensemble", 0.0125, [NASH, ["x", "y"]], [
        _cb([7], nan4, [[NAN, NAN]]), _cb([7], nan4, R2[24:25]), _cb([3, 3], R[25:27], [[NAN, NAN], [NAN, NAN]])]))

    # ---- equal confidences in a row: classifyMultiple's stable sort keeps legend order (pj == pf && j < lane)
    q4, p2 = [[0.25, 0.25, 0.25, 0.25]], [[0.375, 0.125, 0.375, 0.125]]
    out.append(_case("rank-ties", 0.0125, [NASH], [
        _cb([7], p2), _cb([7], q4), _cb([7, 5], np.vstack([q4, p2])), _cb([3], [[0.125, 0.375, 0.125, 0.375]]),
        _cb([4, 4, 4], [[0.125, 0.375, 0.125, 0.375], [0.25] * 4, [0.375, 0.125, 0.375, 0.125]])]))
    out.append(_case("rank-ties-reversed-keys", 0.0125, [["3", "2", "1", "0"]], [_cb([7], q4), _cb([7, 5], np.vstack([p2, q4])), _cb([7], p2)]))
    # KNN's votes / k_eff tie all the time; doubles a float cannot hold, through the double kernels with the class-index legend
    out.append(_case("rank-ties-knn", 0.0125, [IDX4], [
        _cb([7], [[1 / 3, 1 / 3, 1 / 3, 0]], dtype="f64"), _cb([7], [[0, 3 / 7, 2 / 7, 2 / 7]], dtype="f64"),
        _cb([7, 5], [[2 / 5, 2 / 5, 1 / 5, 0], [1 / 3, 0, 1 / 3, 1 / 3]], dtype="f64"),
        _cb([3, 3], [[2 / 7, 3 / 7, 2 / 7, 0], [3 / 7, 2 / 7, 2 / 7, 0]], dtype="f64"), _cb([4], [[0, 0, 0.5, 0.5]], dtype="f64")], dtype="f64"))

    # ---- segment sums that tie exactly (equal durations, swapped confidences: a * w + b * w == b * w + a * w); the key order decides
    sw2 = [[0.3, 0.7], [0.7, 0.3]]
    out.append(_case("sum-ties-strings", 0.0125, [["b", "a"]], [_cb([7, 7], sw2), _cb([5, 5], sw2[::-1])]))          # a is inserted first: a
    # ... unless an earlier single-syllable callback's top entry inserted b
    out.append(_case("sum-ties-strings-earlier-single", 0.0125, [["b", "a"]], [_cb([3], [[0.9, 0.1]]), _cb([7, 7], sw2), _cb([5, 5], sw2[::-1])]))
    # two lone syllables insert a, then b (against the legend's order); the tie goes to a.  (Only the lanes that add take part in an
    # insertion, yet every lane's stamp must move on: a stamp advanced only by the adding lane would date b as early as a.)
    out.append(_case("sum-ties-strings-two-singles", 0.0125, [["b", "a"]], [_cb([3], [[0.1, 0.9]]), _cb([3], [[0.9, 0.1]]), _cb([7, 7], sw2[::-1]), _cb([5, 5], sw2)]))
    # keys in Object.keys order: "0", "2", "10", then x — whatever the legend or the insertion order
    sw4 = [[0.35, 0.15, 0.35, 0.15], [0.15, 0.35, 0.15, 0.35]]
    out.append(_case("sum-ties-index", 0.0125, [["10", "2", "x", "0"]], [
        _cb([7, 7], sw4), _cb([5, 5], [[0.4, 0.1, 0.4, 0.1], [0.1, 0.2, 0.1, 0.2]]), _cb([5, 5], [[0.1, 0.4, 0.3, 0.2], [0.1, 0.3, 0.4, 0.2]]),
        _cb([5, 5], [[0.4, 0.1, 0.3, 0.2], [0.3, 0.1, 0.4, 0.2]])]))
    out.append(_case("sum-ties-index-after-string", 0.0125, [["x", "7"]], [_cb([3], [[0.9, 0.1]]), _cb([7, 7], [[0.6, 0.4], [0.4, 0.6]])]))

    # ---- array indices end at 2^32 - 2: "2147483648" and "4294967294" are index keys, "4294967295", "01" and "-1" are not.  First callback:
    # "4294967294", "4294967295" and "01" tie for the maximum, the two strings inserted first: the index key takes it.  Second: "2147483648"
    # ties with "-1", inserted before it
    big = ["2147483647", "2147483648", "4294967294", "4294967295", "01", "-1"]
    out.append(_case("index-2-31", 0.0125, [big], [
        _cb([7, 7], [[0.02, 0.08, 0.2, 0.3, 0.3, 0.1], [0.1, 0.1, 0.3, 0.2, 0.2, 0.1]]),
        _cb([5, 5], [[0.05, 0.3, 0.1, 0.1, 0.05, 0.4], [0.05, 0.4, 0.1, 0.1, 0.05, 0.3]]),
        _cb([5], [[0.05, 0.1, 0.1, 0.6, 0.05, 0.1]])]))
    out.append(_case("index-2-31-ensemble", 0.0125, [big, NASH], [
        _cb([7, 7], [[0.02, 0.08, 0.2, 0.3, 0.3, 0.1], [0.1, 0.1, 0.3, 0.2, 0.2, 0.1]], R[30:32]),
        _cb([5, 5], [[0.05, 0.3, 0.1, 0.1, 0.05, 0.4], [0.05, 0.4, 0.1, 0.1, 0.05, 0.3]], R[32:34])]))

    # ---- the ensemble's ties: `f.seg > best` and `am > max_inv` keep the earlier member (and the earlier callback)
    durs = [[7], [3, 5, 4], [9, 2], [7], [5, 5, 5, 5, 5]]
    cbs, q = [], 0
    for t in durs:
        cbs.append(_cb(t, R[q:q + len(t)], R[q:q + len(t)])); q += len(t)
    out.append(_case("ensemble-identical", 0.0125, [NASH, NASH], cbs))
    # two members that differ, but whose segment maxima tie on the third callback only (a lone syllable with the same top confidence)
    out.append(_case("ensemble-seg-tie-cb3", 0.0125, [NASH, ["x", "y"]], [
        _cb([7], [[0.5, 0.25, 0.125, 0.125]], [[0.25, 0.75]]), _cb([3, 5], R[12:14], R2[12:14]),
        _cb([7], [[0.125, 0.625, 0.125, 0.125]], [[0.625, 0.375]]), _cb([4, 4], R[14:16], R2[14:16]),
        _cb([7], [[0.125, 0.125, 0.625, 0.125]], [[0.375, 0.625]])]))
    # the launch maxima tie: member 1 reaches member 0's DB_entropies_all one callback later, under another label; min_entropy_db stays 0
    out.append(_case("ensemble-allmax-tie", 0.0125, [NASH, ["x", "y"]], [
        _cb([7], [[0.75, 0.125, 0.0625, 0.0625]], [[0.5, 0.25]]), _cb([7], [[0.0625, 0.25, 0.0625, 0.0625]], [[0.25, 0.75]]),
        _cb([7], [[0.0625, 0.0625, 0.0625, 0.75]], [[0.125, 0.125]])]))
    # no member has a sum above 0: no winner, min_entropy_db still none and the entropy NaN; then they come
    out.append(_case("ensemble-none-then-some", 0.0125, [NASH, ["x", "y"]], [
        _cb([7], z4, z2), _cb([7, 7], np.vstack([z4, z4]), np.vstack([z2, z2])), _cb([7], [[0.1, 0.2, 0.3, 0.4]], [[0.3, 0.7]]),
        _cb([0], z4, z2)]))
    # members of 1, 4 and 64 classes together
    L64 = [f"c{i}" for i in range(64)]
    R64, R1 = _rand_rows(13, 8, 64), np.ones((8, 1))
    out.append(_case("ensemble-1-4-64", 0.0125, [["only"], NASH, L64], [
        _cb([7], R1[0:1], R[0:1], R64[0:1]), _cb([3, 5, 4], R1[1:4], R[1:4], R64[1:4]), _cb([9], R1[4:5] * 0.25, R[4:5], R64[4:5]),
        _cb([2, 2], R1[5:7] * 0.5, R[5:7], R64[5:7])]))
    # eight members of 1 .. 8 classes
    legs8 = [[f"m{d}k{c}" for c in range(d + 1)] for d in range(8)]
    rows8 = [_rand_rows(20 + d, 6, d + 1) for d in range(8)]
    out.append(_case("ensemble-8", 0.0125, legs8, [
        _cb([7], *[r[0:1] for r in rows8]), _cb([3, 5], *[r[1:3] for r in rows8]), _cb([9, 2, 4], *[r[3:6] for r in rows8])]))

    # ---- the entropy's sum runs in Object.keys order: legend "2", "1", "0" is read back "0", "1", "2", and a + b + c is not c + b + a
    # (after every callback of this case the two orders differ in the last bit)
    out.append(_case("entropy-order", 0.0125, [["2", "1", "0"]], [
        _cb([3, 3], [[0.05, 0.1, 0.15], [0.05, 0.1, 0.15]]), _cb([3, 3], [[0.2, 0.3, 0.5], [0.2, 0.3, 0.5]]), _cb([3], [[0.1, 0.2, 0.3]])]))
    return out


def _size_cases():
    """Sizes at which the kernels' loops and strides change: callbacks of 1, 2, 63, 64, 65 and 130 rows (`t_n[q] = 0` strides by 64 lanes, by
    the whole workgroup in the group kernel); 1, 2, 63 and 64 classes."""
    out = []
    R = _rand_rows(31, 330, 4)
    cbs, q = [], 0
    for n in (1, 2, 63, 64, 65, 130):
        cbs.append(_cb([3 + (i * 7) % 23 for i in range(n)], R[q:q + n])); q += n
    out.append(_case("long-callbacks", 0.0125, [NASH], cbs))
    for C in (1, 2, 63, 64):
        Rc = _rand_rows(40 + C, 7, C)
        Rc[5] = Rc[4][::-1]                                    # a sum tie between the first and the last class (lane 0 and lane C - 1)
        leg = [f"k{c}" for c in range(C)] if C % 2 else [str(C - 1 - c) for c in range(C)]
        out.append(_case(f"classes-{C}", 0.0125, [leg], [_cb([7], Rc[0:1]), _cb([3, 5, 4], Rc[1:4]), _cb([6, 6], Rc[4:6]), _cb([2], Rc[6:7])]))
    return out


CASES = _named_cases()
SIZE_CASES = _size_cases()
BY_NAME = {c["name"]: c for c in CASES + SIZE_CASES}
assert len(BY_NAME) == len(CASES) + len(SIZE_CASES)


def member_case(case, d):
    """member d of an ensemble case as a one-model case"""
    return dict(name=f"{case['name']}[{d}]", step_s=case["step_s"], legends=[case["legends"][d]], dtype=case["dtype"],
                callbacks=[dict(t_len=cb["t_len"], conf=[cb["conf"][d]]) for cb in case["callbacks"]])


def run_case(case):
    """The case through the restatement: one ensemble_ref.Launch, its callbacks in order.  Returns the Launch and the callbacks' results."""
    L = ensemble_ref.Launch(case["legends"])
    res = []
    for cb in case["callbacks"]:
        durs = [classify_ref.fixed3((t + 1) * case["step_s"]) for t in cb["t_len"]]
        res.append(L.callback(durs, cb["conf"]))
    return L, res


# ---- tables for the test entry: a batch of clips, or steps of streams
def filler_case(case, i):
    """one one-row callback with the case's legends (what most clips of a layout hold)"""
    confs = []
    for d, leg in enumerate(case["legends"]):
        c = _rand_rows(1000 + 17 * i + d, 1, len(leg))
        confs.append(c if case["dtype"] == "f32" else c / 3.0)
    return dict(name=f"filler{i}", step_s=case["step_s"], legends=case["legends"], dtype=case["dtype"],
                callbacks=[dict(t_len=[3 + i % 29], conf=confs)])


def batch_tables(launches, si0=0):
    """launches: one case-like dict per clip, or None for a clip without rows (all with the same legends and step).  Returns meta [n_rows, 8],
    row_off [n + 1], conf[d] [n_rows, C_d] (float64 values) and the list of callbacks (clip, callback index in the clip's launch)."""
    first = next(l for l in launches if l is not None)
    nd = len(first["legends"])
    meta, off, conf, cbs = [], [0], [[] for _ in range(nd)], []
    for clip, L in enumerate(launches):
        for k, cb in enumerate(L["callbacks"] if L else []):
            for j, t in enumerate(cb["t_len"]):
                meta.append([clip, si0 + 2 * k, 0, t, 0, 0, 0, 0])          # si: any distinct numbers per callback
                for d in range(nd):
                    conf[d].append(cb["conf"][d][j])
            cbs.append((clip, k))
        off.append(len(meta))
    C = [len(l) for l in first["legends"]]
    return (np.array(meta, np.int32).reshape(-1, 8), np.array(off, np.uint32),
            [np.array(conf[d], np.float64).reshape(-1, C[d]) for d in range(nd)], cbs)


class Restated:
    """What the device tables hold, from the restatement: feed callbacks in table order with callback(); read sums with sums()."""

    def __init__(self, legends, n):
        self.legends, self.n = legends, n
        self.launch = [ensemble_ref.Launch(legends) for _ in range(n)]
        self.rows = []                                            # per callback: dict of the device's figures

    def start(self, who):
        self.launch[who] = ensemble_ref.Launch(self.legends)

    def callback(self, who, si, first_row, t_len, conf, step_s):
        legends = self.legends
        durs = [classify_ref.fixed3((int(t) + 1) * step_s) for t in t_len]
        r = self.launch[who].callback(durs, conf)
        db = r["db"]
        self.rows.append(dict(
            cb=(who, si, first_row, len(t_len)),
            label=[-2 if lab == "skip" else (-1 if lab is None else legends[d].index(lab)) for d, (lab, _, _) in enumerate(r["per_db"])],
            conf=[c for _, c, _ in r["per_db"]], all_max=[m for _, _, m in r["per_db"]],
            db=-2 if db == "skip" else (-1 if db is None else db),
            top_label=legends[db].index(r["label"]) if isinstance(db, int) and r["label"] is not None else -1,
            top_conf=r["conf"], min_db=-1 if r["min_db"] is None else r["min_db"], entropy=r["entropy"]))

    def sums(self, d):
        """Label_conf_all of member d per clip / stream, by legend position (0 where the label is no key)"""
        return np.array([[L.acc_all[d].get(lab, 0.0) for lab in self.legends[d]] for L in self.launch], np.float64).reshape(self.n, len(self.legends[d]))

    def min_db(self):
        return np.array([-1 if L.min_entropy_db is None else L.min_entropy_db for L in self.launch], np.int32)


def restate_batch(meta, row_off, conf, legends, step_s):
    n = len(row_off) - 1
    R = Restated(legends, n)
    for clip in range(n):
        r, r1 = int(row_off[clip]), int(row_off[clip + 1])
        while r < r1:
            e = r + 1
            while e < r1 and meta[e][1] == meta[r][1]:
                e += 1
            R.callback(clip, int(meta[r][1]), r, meta[r:e, 3], [c[r:e] for c in conf], step_s)
            r = e
    return R


def deal_steps(launches, plan, front_rows=0, si0=0):
    """Streams: launches[s] (a case-like dict or None) dealt into steps.  plan[k][s] = (callbacks of stream s in step k, control byte).
    front_rows: one-row filler callbacks are NOT added here — put a filler stream with that many callbacks in front instead.  Returns
    meta [n_rows, 8], row_off [n_steps, n + 1], ctl [n_steps, n], conf[d]."""
    n = len(launches)
    first = next(l for l in launches if l is not None)
    nd = len(first["legends"])
    C = [len(l) for l in first["legends"]]
    meta, offs, conf, ctl = [], [], [[] for _ in range(nd)], []
    nxt = [0] * n
    for step in plan:
        off, row = [0], 0
        for s in range(n):
            take, byte = step[s]
            if byte & 2:                                           # START: the stream's launch begins again
                nxt[s] = 0
            for k in range(nxt[s], nxt[s] + take):
                cb = launches[s]["callbacks"][k]
                for j, t in enumerate(cb["t_len"]):
                    meta.append([s, si0 + 2 * k, 0, t, 0, 0, 0, 0])
                    for d in range(nd):
                        conf[d].append(cb["conf"][d][j])
                    row += 1
            nxt[s] += take
            off.append(row)
        offs.append(off)
        ctl.append([b for _, b in step])
    return (np.array(meta, np.int32).reshape(-1, 8), np.array(offs, np.uint32), np.array(ctl, np.uint8),
            [np.array(conf[d], np.float64).reshape(-1, C[d]) for d in range(nd)])


def restate_steps(meta, row_off, ctl, conf, legends, step_s):
    """Per step: the Restated rows of the step's callbacks (first rows counted from the step's first row), the sums and min_db as the step
    leaves them."""
    n_steps, n = ctl.shape
    R = Restated(legends, n)
    steps, row0 = [], 0
    for k in range(n_steps):
        before = len(R.rows)
        for s in range(n):
            if ctl[k][s] & 2:
                R.start(s)
            r, r1 = row0 + int(row_off[k][s]), row0 + int(row_off[k][s + 1])
            while r < r1:
                e = r + 1
                while e < r1 and meta[e][1] == meta[r][1]:
                    e += 1
                R.callback(s, int(meta[r][1]), r - row0, meta[r:e, 3], [c[r:e] for c in conf], step_s)
                r = e
        steps.append(dict(rows=R.rows[before:], sums=[R.sums(d) for d in range(len(legends))], min_db=R.min_db()))
        row0 += int(row_off[k][n])
    return steps
