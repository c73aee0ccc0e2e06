"""The app's ml5 KNN classifier on the GPU: the host half of specification KN-1 (K9 is the device half, capi.KnnStore).
What the reference application does with `ml5.KNNClassifier()` in src/neuralmodel.js:729-837 (train_knn): addExample(features, label)
for the first 80 % of a labelled feature DB, classify(features, 10, ...) for the next 100 rows, and the share that came out right.

Everything that is a label is resolved here; the device sees class indices in ml5's class order:
  * a STRING label gets the index of its first appearance (ml5 keeps `mapStringToIndex` and hands the tfjs classifier that index);
  * a NUMBER label is its own class id;
  * the classes are scanned in the order of JavaScript's `for ... in` over those ids: ids that are array indices ascending, then any other
    (-1, 1.5) in order of first appearance.  With string labels alone that is the order of first appearance.
A string label and a number label that land on the same id share a class, as they do in ml5.
"""
import numpy as np

from .dbstats import _strict_in, js_number_str, js_str

MAX_K, MAX_CLASSES = 64, 64            # WSA_KNN_MAX_K, WSA_MODEL_MAX_CLASSES
TOO_SMALL = "Sample size {}/{} too small for training"          # neuralmodel.js:793


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def label_order(labels):
    """(names, index) of a sequence of labels in insertion order: names = the label ml5 reports for each class, classes in ml5's scan
    order; index [len(labels)] i32 = the class of each label in that order.  Labels are strings or numbers (anything else never reaches
    the tfjs classifier with a usable id and is refused here)."""
    strings, keys, per = [], [], []
    for lab in labels:
        if isinstance(lab, str):
            if lab not in strings:
                strings.append(lab)
            key = strings.index(lab)
        elif _is_number(lab):
            v = float(lab)
            key = int(v) if v == v and v >= 0 and v == int(v) and v < 4294967295 else js_number_str(v)     # an array index, or a plain key
        else:
            raise ValueError(f"a KNN label is a string or a number, got {lab!r}")
        if key not in keys:
            keys.append(key)
        per.append(key)
    order = sorted(k for k in keys if isinstance(k, int)) + [k for k in keys if not isinstance(k, int)]
    pos = {k: i for i, k in enumerate(order)}
    names = [strings[k] if isinstance(k, int) and k < len(strings) and strings[k] else js_str(k) for k in order]
    return names, np.array([pos[k] for k in per], np.int32)


def evaluation_plan(true_labels, classes):
    """train_knn's choice of rows (neuralmodel.js:761-828): (rows added, rows classified).  true_labels[i] is row i's value of the label,
    None where the row has none; a row counts when its label is in `classes` (strict indexOf) or `classes` holds '*'.  The first
    int(0.8 n) rows are added, the next 100 classified; rows past the end or without a label are skipped.  Fewer than 10 added rows:
    ValueError with the app's message."""
    n = len(true_labels)
    split_at = int(n * 0.8)
    star = _strict_in("*", classes)

    def counts(i):
        return true_labels[i] is not None and (star or _strict_in(true_labels[i], classes))

    add = [i for i in range(split_at) if counts(i)]
    if len(add) < 10:
        raise ValueError(TOO_SMALL.format(len(add), n))
    test = [i for i in range(split_at, min(split_at + 100, n)) if counts(i)]
    return add, test


def name_results(classes, r):
    """The class indices of a KNN result (Batch.knn_classes / knn_fold_classes, Streams.knn_classes: any of `label`, `cb_label`) as the
    labels ml5 reports, `classes` being label_order's names: adds `label` / `cb_label` as lists of names (None for -1 = null and -2 = not
    predicted) and keeps the indices as `index` / `cb_index`; confidence tables are cut to the classes in use.  A table the result does
    not have (None at level 5) stays None."""
    C = len(classes)
    out = dict(r, classes=list(classes))
    for key, raw in (("label", "index"), ("cb_label", "cb_index")):
        if r.get(key) is not None:
            out[raw] = r[key]
            out[key] = [classes[i] if i >= 0 else None for i in r[key]]
    for key in ("conf", "clip_conf", "stream_conf"):
        if r.get(key) is not None:
            out[key] = r[key][:, :C]
    return out


class Knn:
    """ml5.KNNClassifier on an Analyzer's device: add(rows, labels), classify(rows, k), classify_batch(batch, k), fold_batch(batch, k),
    attach(streams, k) / stream_classes(streams).  Keeps a host copy of what
    was added: a label that sorts in front of stored classes (a number label below a stored one) renumbers them, and the store is then
    refilled."""

    def __init__(self, analyzer, width, capacity=4096):
        self.an, self.width, self.capacity = analyzer, int(width), int(capacity)
        self.store = analyzer.knn_store(self.width, MAX_CLASSES, self.capacity)
        self._rows, self._labels = [], []
        self._index = np.zeros(0, np.int32)
        self.classes = []

    def _upload(self, rows, index):
        import torch
        dev = f"cuda:{self.an.device}"
        f = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).to(dev)
        c = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
        self.store.add(f.data_ptr(), c.data_ptr(), len(index), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.current_stream(dev).synchronize()

    def _upload_db(self, db, rows, index):
        """rows of a device DB: gathered on the device into a dense table, added from there"""
        import torch
        dev = f"cuda:{self.an.device}"
        s = torch.cuda.current_stream(dev)
        f = torch.empty((max(len(rows), 1), self.width), dtype=torch.float64, device=dev)
        c = torch.from_numpy(np.ascontiguousarray(index, np.int32)).to(dev)
        db.gather(rows, f.data_ptr(), s.cuda_stream)
        self.store.add(f.data_ptr(), c.data_ptr(), len(index), s.cuda_stream)
        s.synchronize()

    def _refill(self, index):
        """a fresh store filled with everything added so far, host rows and DB rows in the order they came"""
        self.store.close()
        self.store = self.an.knn_store(self.width, MAX_CLASSES, self.capacity)
        at = 0
        for part in self._rows:
            n = len(part[1]) if isinstance(part, tuple) else len(part)
            if n:
                if isinstance(part, tuple):
                    self._upload_db(part[0], part[1], index[at:at + n])
                else:
                    self._upload(part, index[at:at + n])
            at += n

    def add_db(self, db, rows, labels):
        """add() with the rows taken from a featdb.DeviceDB (capi.FeatDB) of the same Analyzer: `rows` are its row indices; the features
        never visit the host (wsa_featdb_gather, then wsa_knn_add).  This object keeps (db, rows), not a copy: a later add() or add_db() whose
        label renumbers the stored classes refills the store and gathers these rows AGAIN, so the DB must stay alive and uncleared for
        as long as anything may still be added here."""
        rows = np.ascontiguousarray(rows, np.uint32).reshape(-1)
        labels = list(labels)
        if db.width != self.width:
            raise ValueError(f"the DB's rows have {db.width} features, the store takes {self.width}")
        if len(labels) != len(rows):
            raise ValueError(f"{len(rows)} rows, {len(labels)} labels")
        names, index = label_order(self._labels + labels)
        if len(names) > MAX_CLASSES:
            raise ValueError(f"{len(names)} classes: a KNN store takes {MAX_CLASSES}")
        if len(index) > self.capacity:
            raise ValueError(f"{len(index)} rows: the store was created for {self.capacity}")
        old = len(self._labels)
        self._rows.append((db, rows))
        self._labels += labels
        if np.array_equal(index[:old], self._index):
            if len(labels):
                self._upload_db(db, rows, index[old:])
        else:
            self._refill(index)
        self._index, self.classes = index, names

    def add(self, rows, labels):
        rows = np.asarray(rows, np.float64).reshape(-1, self.width)
        labels = list(labels)
        if len(labels) != len(rows):
            raise ValueError(f"{len(rows)} rows, {len(labels)} labels")
        names, index = label_order(self._labels + labels)
        if len(names) > MAX_CLASSES:
            raise ValueError(f"{len(names)} classes: a KNN store takes {MAX_CLASSES}")
        if len(index) > self.capacity:
            raise ValueError(f"{len(index)} rows: the store was created for {self.capacity}")
        old = len(self._labels)
        self._rows.append(rows)
        self._labels += labels
        if np.array_equal(index[:old], self._index):
            if len(labels):
                self._upload(rows, index[old:])
        elif any(isinstance(part, tuple) for part in self._rows):
            self._refill(index)                      # rows of a device DB among them (add_db): part by part, the DB's gathered again
        else:                                        # stored classes were renumbered: a fresh store, filled in one go
            self.store.close()
            self.store = self.an.knn_store(self.width, MAX_CLASSES, self.capacity)
            self._upload(np.concatenate(self._rows), index)
        self._index, self.classes = index, names

    def count(self):
        """(rows stored, {label: rows}) — ml5 getCountByLabel."""
        n, per = self.store.count()
        return n, {name: int(per[i]) for i, name in enumerate(self.classes)}

    def _result(self, label, conf, nbr, sim, k_eff):
        C = len(self.classes)
        return dict(label=[self.classes[i] if i >= 0 else None for i in label], index=label, conf=conf[:, :C], nbr=nbr[:, :k_eff], sim=sim[:, :k_eff],
                    classes=list(self.classes))

    def classify(self, rows, k=10):
        """dict(label [n] (the class's label as ml5 reports it), index [n] i32, conf [n, C] f64 in the order of `classes`, nbr [n, k_eff]
        i32 insertion indices in selection order, sim [n, k_eff] f32, classes)."""
        import torch
        rows = np.asarray(rows, np.float64).reshape(-1, self.width)
        n, dev = len(rows), f"cuda:{self.an.device}"
        k_eff = min(int(k), len(self._labels))
        f = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
        label = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        conf = torch.empty((max(n, 1), MAX_CLASSES), dtype=torch.float64, device=dev)
        nbr = torch.empty((max(n, 1), int(k)), dtype=torch.int32, device=dev)
        sim = torch.empty((max(n, 1), int(k)), dtype=torch.float32, device=dev)
        s = torch.cuda.current_stream(dev)
        self.store.classify_rows(f.data_ptr(), n, k, label.data_ptr(), conf.data_ptr(), nbr.data_ptr(), sim.data_ptr(), s.cuda_stream)
        s.synchronize()
        return self._result(label[:n].cpu().numpy(), conf[:n].cpu().numpy(), nbr[:n].cpu().numpy(), sim[:n].cpu().numpy(), k_eff)

    def classify_batch(self, batch, k=10, stream=0):
        """The same over the rows of a batch's last run (wsa_batch_knn); a thrown level-12 row has label None and NaN confidences."""
        batch.knn(self.store, k, stream)
        r = batch.knn_classes(stream)
        return self._result(r["label"], r["conf"], r["nbr"], r["sim"], r["k_eff"])

    def fold_batch(self, batch, k=10, stream=0):
        """classify_batch, then the per-callback fold KN-2 over it (level 13; wsa_batch_knn_fold): dict(cb [n_cb, 4], cb_label (names;
        None: null or not predicted), cb_index, cb_conf, clip_conf [n_clips, C], classes)."""
        batch.knn(self.store, k, stream)
        batch.knn_fold(stream)
        return name_results(self.classes, batch.knn_fold_classes(stream))

    def attach(self, streams, k=10):
        """K9s (and at level 13 the fold KN-2) inside every step of `streams` (wsa_stream_set_knn) with the rows stored NOW: attach again
        after add() — a step keeps the row count of the attach, and an add() that renumbers the classes makes a new store."""
        streams.set_knn(self.store, k)

    def detach(self, streams):
        streams.set_knn(None)

    def stream_classes(self, streams):
        """After streams.collect(): the step's KNN tables (Streams.knn_classes) with `label` and `cb_label` as label names."""
        return name_results(self.classes, streams.knn_classes())

    def close(self):
        self.store.close()


def evaluate(rows, true_labels, classes, k=10, analyzer=None, make_knn=None):
    """train_knn (neuralmodel.js:761-828) on a labelled feature DB: rows [n][width], true_labels [n] (None: the row has no such label),
    classes = the label's class list.  Returns (correct, all): the classified rows whose predicted label == their true one (compared as
    the reference's loose == does between ml5's label and the stored one: as strings), and how many were classified.
    make_knn(width, capacity) builds the classifier (default: Knn on `analyzer`); tests hand in a restatement."""
    add, test = evaluation_plan(true_labels, classes)
    rows = np.asarray(rows, np.float64)
    if make_knn is None:
        def make_knn(width, capacity):
            return Knn(analyzer, width, capacity)
    knn = make_knn(rows.shape[1], len(add))
    knn.add(rows[add], [true_labels[i] for i in add])
    if not test:
        return 0, 0
    got = knn.classify(rows[test], k)["label"]
    correct = sum(1 for g, i in zip(got, test) if g == js_str(true_labels[i]))
    return correct, len(test)
