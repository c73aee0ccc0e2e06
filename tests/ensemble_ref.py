"""Float64 restatement of the app's prediction path with several model DBs (test helper): the per-DB fold of src/prediction.js:86-123
(classify_ref.fold_clip's arithmetic, one accumulator per DB) and the decision of seg_confidence_sort (lines 127-169) with the readout
of plot_prediction_meters (lines 172-215).  Exact double arithmetic in the reference's order of operations, so K6b-e and the decision
must equal it bit for bit when fed the same f32 probabilities."""
from tests import classify_ref

NAN = float("nan")
ARMS = classify_ref.FOLD_ARMS                        # the arm counters of the fold's comparisons, shared with classify_ref


class Launch:
    """One launch of the app (reset_predictions(true) at its start): `legends` = the legend of every DB in the order of available_DBs.
    min_entropy_db starts at None: the reference keeps the previous launch's value, the device reports -1 (include/wsa.h)."""

    def __init__(self, legends):
        self.legends = [list(l) for l in legends]
        self.acc_all = [{} for _ in legends]
        self.db_all = [0.0] * len(legends)          # DB_entropies_all
        self.max_inv_entropy = 0.0
        self.min_entropy_db = None

    def callback(self, durs, probs):
        """durs [n_syl] = parseFloat(seg_time[ph][1]); probs[d] [n_syl][C_d].  Returns a dict: skipped, per_db [(label or None, conf,
        all_max)], db (index, None = null), label, conf, min_db, entropy, meters [(label, value)] of min_db in key order."""
        seg_weight = 0.0
        for d in durs:
            seg_weight += d
        skipped = not seg_weight > 0
        ARMS["skip.zero" if skipped else "skip.positive"] += 1
        per_db, seg_max = [], []
        if not skipped:
            for di, labels in enumerate(self.legends):
                acc_all = self.acc_all[di]
                acc_seg = classify_ref.fold_segment(acc_all, durs, probs[di], labels)
                lab_seg, max_seg = classify_ref.segment_label(acc_all, acc_seg)
                max_all = 0.0
                for k in acc_all:                   # (a maximum does not depend on the key order)
                    if acc_all[k] > max_all:
                        max_all = acc_all[k]
                self.db_all[di] = max_all
                seg_max.append(max_seg)
                per_db.append((lab_seg, max_seg / seg_weight, max_all))
            best, db, label = 0.0, None, None
            for di in range(len(self.legends)):
                if seg_max[di] > best:
                    best, db, label = seg_max[di], di, per_db[di][0]
                    ARMS["winner.replaced"] += 1
                elif best > 0 and seg_max[di] == best:
                    ARMS["winner.tie_kept"] += 1
                if self.db_all[di] > self.max_inv_entropy:
                    self.max_inv_entropy, self.min_entropy_db = self.db_all[di], di
                    ARMS["min_db.raised"] += 1
                elif self.max_inv_entropy > 0 and self.db_all[di] == self.max_inv_entropy and di != self.min_entropy_db:
                    ARMS["min_db.tie_kept"] += 1
            if db is None:
                ARMS["winner.none"] += 1
            if self.min_entropy_db is None:
                ARMS["min_db.none"] += 1
            conf = best / seg_weight
        else:
            ARMS["min_db.skipped"] += 1
            per_db = [("skip", 0.0, self.db_all[di]) for di in range(len(self.legends))]
            db, label, conf = "skip", None, 0.0
        entropy, meters = NAN, []
        m = self.min_entropy_db
        if m is not None:
            keys = classify_ref._keys(self.acc_all[m])
            in_legend_order = [k for k in self.legends[m] if k in self.acc_all[m]]
            ARMS["all_sum.legend_order" if keys == in_legend_order else "all_sum.key_order_differs"] += 1
            total = 0
            for k in keys:
                total += self.acc_all[m][k]
            meters = [(k, self.acc_all[m][k] / total) for k in keys]
            entropy = 1 - self.db_all[m] / total
        return dict(skipped=skipped, per_db=per_db, db=db, label=label, conf=conf, min_db=m, entropy=entropy, meters=meters)


def fold_rows(meta, probs, legends, step_s):
    """The ensemble over a batch's compacted level-13 rows as the device reports it (probs[d] [n_rows][C_d]): dict of lists per
    callback in row order — cb (clip, si, first row, rows), cb_label[d] / cb_conf[d] / cb_all_max[d], cb_db, cb_top_label, cb_top_conf,
    cb_min_db, cb_entropy — plus clip_conf {clip: [Label_conf_all per member]} and clip_min_db {clip: db or -1}."""
    nd = len(legends)
    out = dict(cb=[], cb_label=[[] for _ in range(nd)], cb_conf=[[] for _ in range(nd)], cb_all_max=[[] for _ in range(nd)], cb_db=[],
               cb_top_label=[], cb_top_conf=[], cb_min_db=[], cb_entropy=[], clip_conf={}, clip_min_db={}, meters=[])
    launches = {}
    r = 0
    while r < len(meta):
        e = r + 1
        while e < len(meta) and meta[e][0] == meta[r][0] and meta[e][1] == meta[r][1]:
            e += 1
        clip = int(meta[r][0])
        L = launches.setdefault(clip, Launch(legends))
        durs = [classify_ref.fixed3((int(meta[q][3]) + 1) * step_s) for q in range(r, e)]
        res = L.callback(durs, [[probs[d][q] for q in range(r, e)] for d in range(nd)])
        out["cb"].append((clip, int(meta[r][1]), r, e - r))
        for d in range(nd):
            lab, conf, all_max = res["per_db"][d]
            out["cb_label"][d].append(-2 if lab == "skip" else (-1 if lab is None else legends[d].index(lab)))
            out["cb_conf"][d].append(conf)
            out["cb_all_max"][d].append(all_max)
        db = res["db"]
        out["cb_db"].append(-2 if db == "skip" else (-1 if db is None else db))
        out["cb_top_label"].append(legends[db].index(res["label"]) if isinstance(db, int) else -1)
        out["cb_top_conf"].append(res["conf"])
        out["cb_min_db"].append(-1 if res["min_db"] is None else res["min_db"])
        out["cb_entropy"].append(res["entropy"])
        out["meters"].append(res["meters"])
        r = e
    for clip, L in launches.items():
        out["clip_conf"][clip] = L.acc_all
        out["clip_min_db"][clip] = -1 if L.min_entropy_db is None else L.min_entropy_db
    return out
