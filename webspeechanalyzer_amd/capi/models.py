"""Trained models on the device: the Dense classifier, the ensemble, the regression group and the KNN store."""
import ctypes

import numpy as np

from ._abi import _ModelDesc, lib
from ._util import _Handle


def _model_desc(spec):
    """(wsa_model_desc of an nnmodel.ModelSpec, the objects that own what it points to)."""
    from .. import nnmodel
    nl = len(spec.kernels)
    keep = [np.ascontiguousarray(k, np.float32) for k in spec.kernels] + [np.ascontiguousarray(b, np.float32) for b in spec.biases]
    units = (ctypes.c_int32 * (nl + 1))(*spec.units)
    acts = (ctypes.c_int32 * nl)(*[nnmodel.ACT[a] for a in spec.activations])
    kp = (ctypes.c_void_p * nl)(*[a.ctypes.data for a in keep[:nl]])
    bp = (ctypes.c_void_p * nl)(*[a.ctypes.data for a in keep[nl:]])
    mn, mx = np.ascontiguousarray(spec.in_min, np.float64), np.ascontiguousarray(spec.in_max, np.float64)
    labels = list(spec.labels)
    lab = (ctypes.c_char_p * len(labels))(*[str(x).encode() for x in labels]) if len(labels) == spec.n_classes else None
    d = _ModelDesc(nl, ctypes.cast(units, ctypes.c_void_p), ctypes.cast(acts, ctypes.c_void_p), ctypes.cast(kp, ctypes.c_void_p),
                   ctypes.cast(bp, ctypes.c_void_p), mn.ctypes.data, mx.ctypes.data, ctypes.cast(lab, ctypes.c_void_p) if lab is not None else None)
    return d, (keep, units, acts, kp, bp, mn, mx, lab)


class Model(_Handle):
    """wsa_model: a Dense classifier (the app's ml5 model) on the device of one context."""
    _destroy = "wsa_model_destroy"

    def __init__(self, an, spec):
        self.an, self.L, self.spec = an, an.L, spec
        self.labels = list(spec.labels)
        self.n_classes = spec.n_classes
        self.n_inputs = int(spec.units[0])
        d, self._keep = _model_desc(spec)
        self.h = ctypes.c_void_p()
        an._check(self.L.wsa_model_create(an.h, ctypes.byref(d), ctypes.byref(self.h)))
        self._keep = None

    def classify_rows(self, d_feat, n_rows, d_prob, stream=0):
        """K6 on device rows: d_feat [n_rows][n_inputs] f64 (dense) -> d_prob [n_rows][n_classes] f32 (device pointers, asynchronous on `stream`)."""
        self.an._check(self.L.wsa_classify_rows(self.h, d_feat, int(n_rows), d_prob, stream))

    def out_range(self, out_min=None, out_max=None):
        """(out_min, out_max) as floats: the arguments, else the spec's own; a model without a range and no arguments is refused"""
        lo = getattr(self.spec, "out_min", None) if out_min is None else out_min
        hi = getattr(self.spec, "out_max", None) if out_max is None else out_max
        if lo is None or hi is None:
            raise ValueError("the model has no output range (out_min / out_max): not a regression model's spec, and none was given")
        return float(lo), float(hi)

    def regress_rows(self, d_feat, n_rows, d_value, out_min=None, out_max=None, stream=0):
        """K6 with the un-normalising epilogue on device rows: d_feat [n_rows][n_inputs] f64 (dense) -> d_value [n_rows] f64 (device pointers,
        asynchronous on `stream`); the range defaults to the spec's own."""
        lo, hi = self.out_range(out_min, out_max)
        self.an._check(self.L.wsa_regress_rows(self.h, lo, hi, d_feat, int(n_rows), d_value, stream))


class KnnStore(_Handle):
    """wsa_knn: the unit rows of an ml5 KNN classifier on the device (K9, spec KN-1).  Class indices are what the device sees;
    webspeechanalyzer_amd.knn maps labels to them."""
    _destroy = "wsa_knn_destroy"

    def __init__(self, an, width, n_classes, capacity):
        self.an, self.L, self.h = an, an.L, ctypes.c_void_p()
        self.width, self.n_classes, self.capacity = int(width), int(n_classes), int(capacity)
        an._check(self.L.wsa_knn_create(an.h, self.width, self.n_classes, self.capacity, ctypes.byref(self.h)))

    @staticmethod
    def tile_info():
        """(train rows per tile, query rows per workgroup) of K9."""
        t, q = ctypes.c_int32(), ctypes.c_int32()
        lib().wsa_knn_tile_info(ctypes.byref(t), ctypes.byref(q))
        return t.value, q.value

    def add(self, d_feat, d_class, n, stream=0):
        """n dense device rows [n][width] f64 with their device class indices [n] i32 (wsa_knn_add); only enqueues."""
        self.an._check(self.L.wsa_knn_add(self.h, d_feat, d_class, int(n), stream))

    def count(self, stream=0):
        """Synchronises; (rows stored, rows per class [n_classes])."""
        n, per = ctypes.c_uint32(), np.zeros(self.n_classes, np.uint32)
        self.an._check(self.L.wsa_knn_count(self.h, stream, ctypes.byref(n), per.ctypes.data))
        return n.value, per

    def classify_rows(self, d_feat, n_rows, k, d_label=None, d_conf=None, d_nbr=None, d_sim=None, stream=0):
        """wsa_knn_classify_rows on device pointers (any output may be None); only enqueues."""
        self.an._check(self.L.wsa_knn_classify_rows(self.h, d_feat, int(n_rows), int(k), d_label, d_conf, d_nbr, d_sim, stream))


class Ensemble(_Handle):
    """wsa_ensemble: the models of the app's `available_DBs`, in that order, classified and folded in one pass."""
    _destroy = "wsa_ensemble_destroy"

    def __init__(self, an, models):
        self.an, self.L, self.models = an, an.L, list(models)
        arr = (ctypes.c_void_p * max(len(self.models), 1))(*[m.h if m is not None else None for m in self.models])
        self.h = ctypes.c_void_p()
        an._check(self.L.wsa_ensemble_create(an.h, ctypes.cast(arr, ctypes.c_void_p), len(self.models), ctypes.byref(self.h)))


class RegressGroup(_Handle):
    """wsa_regress_group: 1 .. 8 regression Models with their output ranges, predicted in one grouped launch and folded by RG-1."""
    _destroy = "wsa_regress_group_destroy"

    def __init__(self, an, models, ranges=None):
        self.an, self.L, self.models = an, an.L, list(models)
        ranges = list(ranges) if ranges is not None else [None] * len(self.models)
        if len(ranges) != len(self.models):
            raise ValueError("one (out_min, out_max) per model")
        lo_hi = [m.out_range(*(r if r is not None else (None, None))) if m is not None else (0.0, 1.0) for m, r in zip(self.models, ranges)]
        n = max(len(self.models), 1)
        arr = (ctypes.c_void_p * n)(*[m.h if m is not None else None for m in self.models])
        lo, hi = (ctypes.c_double * n)(*[a for a, _ in lo_hi]), (ctypes.c_double * n)(*[b for _, b in lo_hi])
        self.ranges = lo_hi
        self.h = ctypes.c_void_p()
        an._check(self.L.wsa_regress_group_create(an.h, ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(hi, ctypes.c_void_p),
                                                  len(self.models), ctypes.byref(self.h)))

    def regress_rows(self, d_feat, n_rows, d_values, stream=0):
        """One grouped launch over dense device rows: d_feat [n_rows][53] f64 -> d_values[h] [n_rows] f64 (one device pointer per head),
        asynchronous on `stream`; head h's values are Model.regress_rows' bit for bit."""
        ptrs = (ctypes.c_void_p * max(len(d_values), 1))(*d_values)
        if len(d_values) != len(self.models):
            raise ValueError("one value pointer per head")
        self.an._check(self.L.wsa_regress_group_rows(self.h, d_feat, int(n_rows), ctypes.cast(ptrs, ctypes.c_void_p), stream))
