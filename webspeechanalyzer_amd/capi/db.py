"""Feature DBs on the device: the labelled DB of K8 (wsa_dbstats) and the DB that stays there (K10, wsa_featdb)."""
import ctypes

import numpy as np

from ._abi import CROSSVAL_MAX_FOLDS, WsaError, lib
from ._util import _Handle
from .training import Trainer

DBSTATS_MAX_CLASSES, DBSTATS_MAX_HEADS, DBSTATS_CHUNK_ROWS = 256, 8, 256      # WSA_DBSTATS_* of include/wsa.h
_DB_CAT = np.dtype([("correct", "<u8"), ("wrong", "<u8"), ("blank", "<u8")])
_DB_CLASS = np.dtype([("count", "<u8"), ("correct", "<u8"), ("wrong", "<u8"), ("duration", "<f8"), ("first_row", "<u4"), ("reserved", "<u4")])
_DB_ORD = np.dtype([("true_n", "<u8"), ("pred_n", "<u8"), ("min", "<f8"), ("max", "<f8"), ("sq_sum", "<f8")])
_DB_AGREE = np.dtype([("n", "<u8")] + [(k, "<f8") for k in ("mean_true", "mean_pred", "var_true", "var_pred", "cov", "ccc", "pearson")])   # wsa_dbstats_agree (wsa_eval.h)


class FeatureDBStats(_Handle):
    """wsa_dbstats: one labelled feature DB on the device (K8, spec DS-1).  features [n][53] f64, or 264 / 23 wide: the rows of level 11 / 12 (None: a DB that is only counted) and
    durations [n] f64 are host arrays; vocab_sizes has one vocabulary size per categorical head, n_ord is the number of ordinal heads.
    Indices and values are what the device sees; webspeechanalyzer_amd.dbstats builds them from the app's rows."""

    _destroy = "wsa_dbstats_destroy"
    n_files = 0               # until set_files
    n_folds = 0               # until set_folds

    def __init__(self, an, features, durations, vocab_sizes=(), n_ord=0, first_row=0):
        """first_row: with a FeatDB as `features`, the DB row of the first of the len(durations) rows taken"""
        self.an, self.L = an, an.L
        dur = np.ascontiguousarray(durations, np.float64)
        if isinstance(features, FeatDB):                 # the rows of a device DB, copied device to device (wsa_featdb_dbstats_create)
            if dur.ndim != 1:
                raise ValueError(f"durations {dur.shape}: expected [n]")
            self.n_feat, self.n_rows, self.vocab, self.n_ord = features.width, dur.shape[0], [int(v) for v in vocab_sizes], int(n_ord)
            voc = np.ascontiguousarray(self.vocab, np.uint32)
            self.h = ctypes.c_void_p()
            an._check(self.L.wsa_featdb_dbstats_create(an.h, features.h, int(first_row), self.n_rows, dur.ctypes.data if self.n_rows else None, len(self.vocab),
                                                   voc.ctypes.data if len(self.vocab) else None, self.n_ord, ctypes.byref(self.h)))
            return
        feat = None if features is None else np.ascontiguousarray(features, np.float64)
        if dur.ndim != 1 or (feat is not None and (feat.ndim != 2 or feat.shape[0] != dur.shape[0] or feat.shape[1] not in (53, 264, 23))):
            raise ValueError(f"features {None if feat is None else feat.shape} / durations {dur.shape}: expected [n][53] (or [n][264], [n][23]) and [n]")
        self.n_feat = 53 if feat is None else feat.shape[1]
        self.n_rows, self.vocab, self.n_ord = dur.shape[0], [int(v) for v in vocab_sizes], int(n_ord)
        voc = np.ascontiguousarray(self.vocab, np.uint32)
        self.h = ctypes.c_void_p()
        an._check(self.L.wsa_wide_dbstats_create(an.h, None if feat is None else feat.ctypes.data, self.n_feat, dur.ctypes.data if self.n_rows else None,
                                                 self.n_rows, len(self.vocab), voc.ctypes.data if len(self.vocab) else None, self.n_ord, ctypes.byref(self.h)))

    def _column(self, x, dtype, name):
        if x is None:
            return None
        a = np.ascontiguousarray(x, dtype)
        if a.shape != (self.n_rows,):
            raise ValueError(f"{name} has shape {a.shape}, the DB has {self.n_rows} rows")
        return a

    def set_classes(self, head, true_idx, pred_idx=None):
        """true_idx [n] (-1: the row does not count), pred_idx [n] (-1: blank) or None (all blank): vocabulary indices of categorical head `head`."""
        t, p = self._column(true_idx, np.int32, "true_idx"), self._column(pred_idx, np.int32, "pred_idx")
        self.an._check(self.L.wsa_dbstats_set_classes(self.h, int(head), t.ctypes.data, None if p is None else p.ctypes.data))

    def set_values(self, head, true_value, pred_value=None):
        """true_value [n], pred_value [n] or None (all missing) of ordinal head `head`; NaN = missing."""
        t, p = self._column(true_value, np.float64, "true_value"), self._column(pred_value, np.float64, "pred_value")
        self.an._check(self.L.wsa_dbstats_set_values(self.h, int(head), t.ctypes.data, None if p is None else p.ctypes.data))

    @staticmethod
    def _map(legend_to_vocab):
        return np.ascontiguousarray(legend_to_vocab, np.int32)

    def predict_classes(self, head, model, legend_to_vocab, stream=0):
        """K6 over every row, then K8's decision into the head's predicted column (enqueues)."""
        m = self._map(legend_to_vocab)
        if m.shape != (model.n_classes,):
            raise ValueError(f"legend_to_vocab has shape {m.shape}, the model has {model.n_classes} classes")
        self.an._check(self.L.wsa_dbstats_predict_classes(self.h, int(head), model.h, m.ctypes.data, stream))

    def decide_rows(self, head, d_prob, n_classes, legend_to_vocab, stream=0):
        """K8's decision alone on a device table d_prob [n_rows][n_classes] f32 (enqueues)."""
        m = self._map(legend_to_vocab)
        if m.shape != (int(n_classes),):
            raise ValueError(f"legend_to_vocab has shape {m.shape}, the table has {n_classes} classes")
        self.an._check(self.L.wsa_dbstats_decide_rows(self.h, int(head), d_prob, int(n_classes), m.ctypes.data, stream))

    def predict_values(self, head, model, out_min=None, out_max=None, stream=0):
        """K6 with the regression epilogue into the head's predicted column (enqueues); the range defaults to the spec's own."""
        lo, hi = model.out_range(out_min, out_max)
        self.an._check(self.L.wsa_dbstats_predict_values(self.h, int(head), model.h, lo, hi, stream))

    # ---- held-out prediction (K6f, spec CV-1; include/wsa_crossval.h)
    def set_folds(self, fold_of_row, n_folds):
        """fold_of_row [n] i32 (-1: the row is never held out and never predicted; else 0 .. n_folds - 1), n_folds 2 .. 32; set once."""
        f = self._column(fold_of_row, np.int32, "fold_of_row")
        self.an._check(self.L.wsa_dbstats_set_folds(self.h, f.ctypes.data, int(n_folds)))
        self.n_folds = int(n_folds)

    @staticmethod
    def _members(models):
        models = list(models)
        return models, (ctypes.c_void_p * max(len(models), 1))(*[m.h if m is not None else None for m in models])

    def predict_classes_folds(self, head, models, legend_to_vocab, stream=0):
        """predict_classes with models[k] over the rows of fold k, in one launch of K6f; rows without a fold get zero probabilities and
        are decided blank (enqueues).  The models share one legend."""
        models, arr = self._members(models)
        m = self._map(legend_to_vocab)
        if models and models[0] is not None and m.shape != (models[0].n_classes,):
            raise ValueError(f"legend_to_vocab has shape {m.shape}, the models have {models[0].n_classes} classes")
        self.an._check(self.L.wsa_dbstats_predict_classes_folds(self.h, int(head), ctypes.cast(arr, ctypes.c_void_p), len(models), m.ctypes.data, stream))

    def predict_values_folds(self, head, models, ranges=None, stream=0):
        """predict_values with models[k] and its own range over the rows of fold k, in one launch of K6f; rows without a fold get NaN
        (enqueues).  ranges: one (out_min, out_max) per model, None: the spec's own."""
        models, arr = self._members(models)
        ranges = list(ranges) if ranges is not None else [None] * len(models)
        if len(ranges) != len(models):
            raise ValueError("one (out_min, out_max) per model")
        lo_hi = [m.out_range(*(r if r is not None else (None, None))) if m is not None else (0.0, 1.0) for m, r in zip(models, ranges)]
        n = max(len(models), 1)
        lo, hi = (ctypes.c_double * n)(*[a for a, _ in lo_hi]), (ctypes.c_double * n)(*[b for _, b in lo_hi])
        self.an._check(self.L.wsa_dbstats_predict_values_folds(self.h, int(head), ctypes.cast(arr, ctypes.c_void_p), len(models),
                                                               ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(hi, ctypes.c_void_p), stream))

    def table(self, stream=0):
        """Synchronises; (cat [n_cat], cls [sum V], ord [n_ord]) as numpy records (wsa_dbstats_cat / _class / _ord)."""
        cat, cls, od = np.zeros(len(self.vocab), _DB_CAT), np.zeros(sum(self.vocab), _DB_CLASS), np.zeros(self.n_ord, _DB_ORD)
        self.an._check(self.L.wsa_dbstats_table(self.h, stream, cat.ctypes.data if len(cat) else None, cls.ctypes.data if len(cls) else None,
                                                od.ctypes.data if len(od) else None))
        return cat, cls, od

    def confusion(self, head, stream=0):
        """K8e (spec EV-1): categorical head `head`'s confusion matrix [V][V + 1] u64 over the counted rows, m[true][predicted]; column V
        collects the blank predictions.  Synchronises."""
        V = self.vocab[int(head)] if 0 <= int(head) < len(self.vocab) else 1      # (a head the DB lacks is refused by the library, before m is touched)
        m = np.zeros((V, V + 1), np.uint64)
        self.an._check(self.L.wsa_dbstats_confusion(self.h, int(head), stream, m.ctypes.data))
        return m

    def agreement(self, stream=0):
        """K8e (spec EV-1): [n_ord] records (wsa_dbstats_agree) over the rows whose true and predicted value both count.  Synchronises."""
        out = np.zeros(self.n_ord, _DB_AGREE)
        self.an._check(self.L.wsa_dbstats_agreement(self.h, stream, out.ctypes.data if len(out) else None))
        return out

    # ---- per file (K8e): a file where K6b / RG-1 have a clip, then the files evaluated as rows
    def set_files(self, file_of_row, callback_of_row, n_files):
        """file_of_row [n] i32 (-1: no file; non-decreasing otherwise), callback_of_row [n] i32 (the row's si); set once."""
        f, c = self._column(file_of_row, np.int32, "file_of_row"), self._column(callback_of_row, np.int32, "callback_of_row")
        self.an._check(self.L.wsa_dbstats_set_files(self.h, f.ctypes.data, c.ctypes.data, int(n_files)))
        self.n_files = int(n_files)

    def _file_column(self, x, dtype, name):
        a = np.ascontiguousarray(x, dtype)
        if a.shape != (self.n_files,):
            raise ValueError(f"{name} has shape {a.shape}, the DB has {self.n_files} files")
        return a

    def set_file_classes(self, head, true_idx):
        """true_idx [n_files] i32: a file's true class of categorical head `head`, -1: the file does not count (the predicted column stays)."""
        t = self._file_column(true_idx, np.int32, "true_idx")             # (held until the call returns: a converted copy is a temporary)
        self.an._check(self.L.wsa_dbstats_set_file_classes(self.h, int(head), t.ctypes.data))

    def set_file_values(self, head, true_value):
        """true_value [n_files] f64 of ordinal head `head`; NaN = missing."""
        t = self._file_column(true_value, np.float64, "true_value")
        self.an._check(self.L.wsa_dbstats_set_file_values(self.h, int(head), t.ctypes.data))

    def fold_files(self, head, stream=0):
        """K6b per file on the probabilities the last predict_classes(head, ..) kept (enqueues)."""
        self.an._check(self.L.wsa_dbstats_fold_files(self.h, int(head), stream))

    def fold_file_values(self, head, stream=0):
        """RG-1's running value per file over ordinal head `head`'s predicted column (enqueues)."""
        self.an._check(self.L.wsa_dbstats_fold_file_values(self.h, int(head), stream))

    def file_table(self, stream=0):
        nf = self.n_files
        cat, cls, od = np.zeros(len(self.vocab), _DB_CAT), np.zeros(sum(self.vocab), _DB_CLASS), np.zeros(self.n_ord, _DB_ORD)
        self.an._check(self.L.wsa_dbstats_file_table(self.h, stream, cat.ctypes.data if len(cat) and nf else None, cls.ctypes.data if len(cls) and nf else None,
                                                     od.ctypes.data if len(od) and nf else None))
        return cat, cls, od

    def file_confusion(self, head, stream=0):
        V = self.vocab[int(head)] if 0 <= int(head) < len(self.vocab) else 1
        m = np.zeros((V, V + 1), np.uint64)
        self.an._check(self.L.wsa_dbstats_file_confusion(self.h, int(head), stream, m.ctypes.data))
        return m

    def file_agreement(self, stream=0):
        out = np.zeros(self.n_ord, _DB_AGREE)
        self.an._check(self.L.wsa_dbstats_file_agreement(self.h, stream, out.ctypes.data if len(out) else None))
        return out

    def file_sums(self, head, n_classes, stream=0):
        """The meter sums (Label_conf_all at the file's end) [n_files][n_classes] f64 of a folded head."""
        out = np.zeros((max(self.n_files, 1), int(n_classes)), np.float64)
        self.an._check(self.L.wsa_dbstats_copy_file_sums(self.h, int(head), stream, out.ctypes.data, int(n_classes)))
        return out[:self.n_files]

    def file_classes(self, head, stream=0):
        out = np.zeros(max(self.n_files, 1), np.int32)
        self.an._check(self.L.wsa_dbstats_copy_file_classes(self.h, int(head), stream, out.ctypes.data))
        return out[:self.n_files]

    def file_values(self, head, stream=0):
        out = np.zeros(max(self.n_files, 1), np.float64)
        self.an._check(self.L.wsa_dbstats_copy_file_values(self.h, int(head), stream, out.ctypes.data))
        return out[:self.n_files]

    def pred_classes(self, head, stream=0):
        out = np.zeros(self.n_rows, np.int32)
        self.an._check(self.L.wsa_dbstats_copy_classes(self.h, int(head), stream, out.ctypes.data))
        return out

    def pred_values(self, head, stream=0):
        out = np.zeros(self.n_rows, np.float64)
        self.an._check(self.L.wsa_dbstats_copy_values(self.h, int(head), stream, out.ctypes.data))
        return out

    def probs(self, n_classes, stream=0):
        """The probabilities the last predict_classes decided on, [n_rows][n_classes] f32."""
        out = np.zeros((self.n_rows, int(n_classes)), np.float32)
        self.an._check(self.L.wsa_dbstats_copy_probs(self.h, stream, out.ctypes.data, int(n_classes)))
        return out


def crossval_tiles(rows_per_fold, rb):
    """wsa_crossval_tiles: the (member, tile) pairs of one K6f launch from the folds' row counts and the members' row-block factors
    (1, 2 or 4) alone; needs no device."""
    n, b = np.ascontiguousarray(rows_per_fold, np.uint32), np.ascontiguousarray(rb, np.int32)
    if n.ndim != 1 or n.shape != b.shape:
        raise ValueError(f"rows_per_fold {n.shape} / rb {b.shape}: expected one of each per fold")
    out = ctypes.c_uint64()
    st = lib().wsa_crossval_tiles(n.ctypes.data if len(n) else None, b.ctypes.data if len(b) else None, len(n), ctypes.byref(out))
    if st != 0:
        raise WsaError(f"wsa_crossval_tiles refused the shapes ({st}): 1 .. {CROSSVAL_MAX_FOLDS} folds, rb 1, 2 or 4")
    return int(out.value)


class FeatDB(_Handle):
    """wsa_featdb: the feature columns of the app's feature DB on the device of one context (K10, spec FD-1): one allocation of
    capacity x width doubles, rows appended behind the ones it holds and never moved.  Strings stay with the caller
    (webspeechanalyzer_amd.featdb.DeviceDB keeps them); pass the same stream to every call."""

    _destroy = "wsa_featdb_destroy"

    def __init__(self, an, width, capacity):
        self.an, self.L, self.h = an, an.L, ctypes.c_void_p()
        self.width, self.capacity = int(width), int(capacity)
        an._check(self.L.wsa_featdb_create(an.h, self.width, self.capacity, ctypes.byref(self.h)))

    @staticmethod
    def tile_info():
        """(source rows per wave tile, per step of the keep kernel's workgroup, appended rows per pass of the copy kernel) of K10."""
        a, b, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        lib().wsa_featdb_tile_info(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return a.value, b.value, c.value

    @property
    def count(self):
        n = ctypes.c_uint32()
        self.an._check(self.L.wsa_featdb_count(self.h, ctypes.byref(n)))
        return int(n.value)

    def clear(self):
        self.an._check(self.L.wsa_featdb_clear(self.h))

    def append_batch(self, batch, stream=0):
        """The rows of the batch's last run that the app's storing keeps (wsa_featdb_append_batch; synchronises).  Returns (first DB row,
        kept): kept [n_added] i32 = the source row (level 11: utterance row) of every appended row."""
        cap = max(int(batch.info["rows_cap"]), int(batch.info["n_clips"]))       # what a run can keep at most; more than the DB's capacity is refused before
        kept = np.zeros(max(min(cap, self.capacity), 1), np.int32)
        first, n = ctypes.c_uint32(), ctypes.c_uint32()
        self.an._check(self.L.wsa_featdb_append_batch(self.h, batch.h, stream, ctypes.byref(first), ctypes.byref(n), kept.ctypes.data, len(kept)))
        return int(first.value), kept[:n.value].copy()

    def append_host(self, features, stream=0):
        """Dense host rows [n][width] (an imported DB); returns the first DB row."""
        feat = np.ascontiguousarray(features, np.float64).reshape(-1, self.width)
        first = self.count
        self.an._check(self.L.wsa_featdb_append_host(self.h, feat.ctypes.data if len(feat) else None, len(feat), stream))
        return first

    def device_rows(self):
        """The device pointer of the dense table [count][width] f64 (valid until close)."""
        p = ctypes.c_void_p()
        self.an._check(self.L.wsa_featdb_device_rows(self.h, ctypes.byref(p)))
        return p.value

    def copy_rows(self, first=0, n=None, stream=0):
        n = self.count - int(first) if n is None else int(n)
        out = np.zeros((n, self.width), np.float64)
        self.an._check(self.L.wsa_featdb_copy_rows(self.h, stream, int(first), n, out.ctypes.data if n else None))
        return out

    def gather(self, rows, d_out, stream=0):
        """d_out [n][width] f64 (device pointer) = DB rows `rows`; only enqueues."""
        r = np.ascontiguousarray(rows, np.uint32)
        if r.ndim != 1:
            raise ValueError(f"rows has shape {r.shape}: expected a list of DB row indices")
        self.an._check(self.L.wsa_featdb_gather(self.h, r.ctypes.data if len(r) else None, len(r), d_out, stream))

    def ranges(self, rows=None, stream=0):
        """(in_min, in_max) [width] over the selected rows (None: all); NaN for a column that holds one; synchronises."""
        r = None if rows is None else np.ascontiguousarray(rows, np.uint32)
        n = self.count if r is None else len(r)
        mn, mx = np.zeros(self.width, np.float64), np.zeros(self.width, np.float64)
        self.an._check(self.L.wsa_featdb_ranges(self.h, None if r is None else r.ctypes.data, n, stream, mn.ctypes.data, mx.ctypes.data))
        return mn, mx

    def trainer(self, spec, rows, labels, n_val, batch_size, learning_rate):
        """A Trainer over DB rows `rows` in that order (wsa_trainer_create_db)."""
        return Trainer(self.an, spec, rows, labels, n_val, batch_size, learning_rate, db=self)

    def regress_trainer(self, spec, rows, values, n_val, batch_size, learning_rate, out_min=None, out_max=None):
        return Trainer(self.an, spec, rows, values, n_val, batch_size, learning_rate, db=self,
                       regression=(spec.out_min if out_min is None else out_min, spec.out_max if out_max is None else out_max))
