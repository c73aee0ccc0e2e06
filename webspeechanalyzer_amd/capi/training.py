"""wsa_trainer and wsa_train_group: training the app's models (K7, K7g)."""
import ctypes

import numpy as np

from ._abi import TRAIN_GROUP_MAX, WsaError, _TrainStats, lib
from ._util import _Handle
from .models import Model, _model_desc


class Trainer(_Handle):
    """wsa_trainer: minibatch SGD on the app's Dense classifiers (K7, spec TR-1).  `spec` holds the INITIAL weights, the ranges to
    normalise with and the legend; features [n][spec.units[0]] f64 (53, 264 or 23 wide) and labels [n] class indices are host arrays, the last n_val rows validation."""

    _destroy = "wsa_trainer_destroy"

    def __init__(self, an, spec, features, labels, n_val, batch_size, learning_rate, regression=None, db=None):
        """regression: None, or (out_min, out_max): `labels` are then real-valued targets and the trainer is TR-2's (Adam, mean squared error).
        db: a FeatDB of `an`; `features` is then the list of its rows to train on, in that order (wsa_trainer_create_db: nothing is uploaded
        but the list), and the trainer is bit for bit the one made from the host copy of those rows."""
        self.an, self.L, self.spec = an, an.L, spec
        self.out_range = None if regression is None else (float(regression[0]), float(regression[1]))
        lab = np.ascontiguousarray(labels, np.int32 if regression is None else np.float64)
        if db is not None:
            rows = np.ascontiguousarray(features, np.uint32)
            if rows.ndim != 1 or lab.shape != rows.shape:
                raise ValueError(f"rows {rows.shape} / labels {lab.shape}: expected [n] DB row indices and [n]")
            self.n_rows, self.n_val, self.n_train = rows.shape[0], int(n_val), rows.shape[0] - int(n_val)
            d, keep = _model_desc(spec)
            self.h = ctypes.c_void_p()
            if regression is None:
                an._check(self.L.wsa_trainer_create_db(an.h, ctypes.byref(d), db.h, rows.ctypes.data, lab.ctypes.data, rows.shape[0], int(n_val),
                                                       int(batch_size), float(learning_rate), ctypes.byref(self.h)))
            else:
                an._check(self.L.wsa_regress_trainer_create_db(an.h, ctypes.byref(d), db.h, rows.ctypes.data, lab.ctypes.data, rows.shape[0], int(n_val),
                                                               int(batch_size), float(learning_rate), self.out_range[0], self.out_range[1], ctypes.byref(self.h)))
            del keep
            return
        feat = np.ascontiguousarray(features, np.float64)
        if feat.ndim != 2 or feat.shape[1] != int(spec.units[0]) or lab.shape != (feat.shape[0],):
            raise ValueError(f"features {feat.shape} / labels {lab.shape}: expected [n][{int(spec.units[0])}] (the model's inputs) and [n]")
        self.n_rows, self.n_val, self.n_train = feat.shape[0], int(n_val), feat.shape[0] - int(n_val)
        d, keep = _model_desc(spec)
        self.h = ctypes.c_void_p()
        if regression is None:
            an._check(self.L.wsa_trainer_create(an.h, ctypes.byref(d), feat.ctypes.data, lab.ctypes.data, feat.shape[0], int(n_val), int(batch_size),
                                                float(learning_rate), ctypes.byref(self.h)))
        else:
            an._check(self.L.wsa_regress_trainer_create(an.h, ctypes.byref(d), feat.ctypes.data, lab.ctypes.data, feat.shape[0], int(n_val),
                                                        int(batch_size), float(learning_rate), self.out_range[0], self.out_range[1], ctypes.byref(self.h)))
        del keep

    def epoch(self, order=None, stream=0):
        """Enqueues one epoch over the training rows in `order` (a sequence of n_train row indices; None = 0, 1, 2, ...)."""
        o = None if order is None else np.ascontiguousarray(order, np.uint32)
        if o is not None and o.shape != (self.n_train,):
            raise ValueError(f"order has shape {o.shape}, the trainer has {self.n_train} training rows")
        self.an._check(self.L.wsa_trainer_epoch(self.h, o.ctypes.data if o is not None else None, stream))

    def stats(self, stream=0):
        """Synchronises; {epochs_done, loss, acc, val_loss, val_acc} of the last finished epoch (ml5's whileTraining / tfjs history)."""
        st = _TrainStats()
        self.an._check(self.L.wsa_trainer_stats(self.h, stream, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in _TrainStats._fields_}

    def weights(self, stream=0):
        """Synchronises; (kernels, biases) as nnmodel.ModelSpec holds them."""
        u = self.spec.units
        ks = [np.zeros((u[i], u[i + 1]), np.float32) for i in range(len(u) - 1)]
        bs = [np.zeros(u[i + 1], np.float32) for i in range(len(u) - 1)]
        kp = (ctypes.c_void_p * len(ks))(*[a.ctypes.data for a in ks])
        bp = (ctypes.c_void_p * len(bs))(*[a.ctypes.data for a in bs])
        self.an._check(self.L.wsa_trainer_copy_weights(self.h, stream, ctypes.cast(kp, ctypes.c_void_p), ctypes.cast(bp, ctypes.c_void_p)))
        return ks, bs

    def spec_now(self, stream=0):
        """The current weights as an nnmodel.ModelSpec (what nnmodel.save_dir writes)."""
        from .. import nnmodel
        ks, bs = self.weights(stream)
        s = self.spec
        out = nnmodel.ModelSpec(list(s.units), list(s.activations), ks, bs, np.array(s.in_min, np.float64), np.array(s.in_max, np.float64), list(s.labels))
        if self.out_range is not None:
            out.out_min, out.out_max = self.out_range
        return out

    def model(self, stream=0):
        """A snapshot of the current weights as a Model on the same context (wsa_trainer_model)."""
        m = Model.__new__(Model)
        m.an, m.L, m.spec = self.an, self.L, self.spec
        if self.out_range is not None:
            m.spec = self.spec_now(stream)
        m.labels, m.n_classes, m._keep, m.n_inputs = list(self.spec.labels), self.spec.n_classes, None, int(self.spec.units[0])
        m.h = ctypes.c_void_p()
        self.an._check(self.L.wsa_trainer_model(self.h, stream, ctypes.byref(m.h)))
        return m


def train_group_launch_count(nl, n_train, batch, n_val):
    """wsa_train_group_launch_count: the kernel launches of one group epoch (spec TG-1) from the members' shapes alone; needs no device."""
    a = [np.ascontiguousarray(v, np.uint32) for v in (nl, n_train, batch, n_val)]
    if any(v.ndim != 1 or v.shape != a[0].shape for v in a):
        raise ValueError("nl, n_train, batch and n_val are sequences of one length")
    out = ctypes.c_uint64()
    st = lib().wsa_train_group_launch_count(*[v.ctypes.data for v in a], len(a[0]), ctypes.byref(out))
    if st != 0:
        raise WsaError(f"wsa_train_group_launch_count refused the shapes ({st}): 1 .. {TRAIN_GROUP_MAX} members, nl 1 .. 8, n_train and batch at least 1")
    return int(out.value)


class TrainGroup(_Handle):
    """wsa_train_group: Trainers of one Analyzer stepped in lock step (K7g, spec TG-1): a group epoch is Trainer.epoch on every member,
    bit for bit, in about the launches of the longest one.  The members stay usable (stats, weights, model, a solo epoch between group
    epochs, all on the same stream); close the group before its members."""

    _destroy = "wsa_train_group_destroy"

    def __init__(self, an, trainers):
        self.an, self.L, self.trainers = an, an.L, list(trainers)
        hs = (ctypes.c_void_p * max(len(self.trainers), 1))(*[t.h for t in self.trainers])
        self.h = ctypes.c_void_p()
        an._check(self.L.wsa_train_group_create(an.h, ctypes.cast(hs, ctypes.c_void_p), len(self.trainers), ctypes.byref(self.h)))

    def epoch(self, orders=None, stream=0):
        """Enqueues one epoch of every member; orders: None, or one entry per member, each None or that member's order (see Trainer.epoch)."""
        ptr = None
        if orders is not None:
            if len(orders) != len(self.trainers):
                raise ValueError(f"{len(orders)} orders for {len(self.trainers)} members")
            keep = [None if o is None else np.ascontiguousarray(o, np.uint32) for o in orders]
            for i, (o, t) in enumerate(zip(keep, self.trainers)):
                if o is not None and o.shape != (t.n_train,):
                    raise ValueError(f"member {i}: order has shape {o.shape}, the trainer has {t.n_train} training rows")
            arr = (ctypes.c_void_p * len(keep))(*[None if o is None else o.ctypes.data for o in keep])
            ptr = ctypes.cast(arr, ctypes.c_void_p)
        self.an._check(self.L.wsa_train_group_epoch(self.h, ptr, stream))

    def stats(self, stream=0):
        """Synchronises once; one Trainer.stats dict per member, in member order."""
        st = (_TrainStats * len(self.trainers))()
        self.an._check(self.L.wsa_train_group_stats(self.h, stream, ctypes.cast(st, ctypes.c_void_p)))
        return [{k: getattr(x, k) for k, _ in _TrainStats._fields_} for x in st]

    def launches(self):
        """The kernel launches of one epoch of this group (spec TG-1's formula; host arithmetic)."""
        n = ctypes.c_uint32()
        self.an._check(self.L.wsa_train_group_launches(self.h, ctypes.byref(n)))
        return int(n.value)
