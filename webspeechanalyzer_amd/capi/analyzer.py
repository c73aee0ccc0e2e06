"""The settings object and the context (wsa_ctx) every other object is made from."""
import ctypes

import numpy as np

from ._abi import WsaError, _Config, _Geometry, lib
from ._util import _Handle
from .batch import Batch
from .db import FeatDB, FeatureDBStats
from .models import Ensemble, KnnStore, Model, RegressGroup
from .streams import Streams
from .training import TrainGroup, Trainer


class Config(dict):
    """The reference's settings object (defaults dist/main.js:2 @B2965, output_level 4 = Segment Formants)."""

    def __init__(self, **kw):
        c = _Config()
        lib().wsa_config_default(ctypes.byref(c))
        super().__init__({k: getattr(c, k) for k, _ in _Config._fields_})
        for k, v in kw.items():
            if k not in self:
                raise KeyError(k)
            self[k] = v

    def c_struct(self):
        c = _Config()
        for k, t in _Config._fields_:
            setattr(c, k, int(self[k]) if t is ctypes.c_int32 else float(self[k]))
        return c


class Analyzer(_Handle):
    """One configured context on one GPU (wsa_ctx)."""
    _destroy = "wsa_destroy"

    def __init__(self, config=None, device=0):
        self.L = lib()
        self.config = config or Config()
        self.h = ctypes.c_void_p()
        cs = self.config.c_struct()
        st = self.L.wsa_create(ctypes.byref(cs), device, ctypes.byref(self.h))
        if st != 0:
            raise WsaError(f"wsa_create failed ({st}): {self.L.wsa_last_error(None).decode()}")
        self.device = device

    def _check(self, st):
        if st != 0:
            raise WsaError(f"libwsa error {st}: {self.L.wsa_last_error(self.h).decode()}")

    def geometry(self, fs):
        g = _Geometry()
        self._check(self.L.wsa_geometry_for(self.h, float(fs), ctypes.byref(g)))
        return {k: getattr(g, k) for k, _ in _Geometry._fields_}

    def bins_hz(self, fs):
        n = self.geometry(fs)["bands"]
        out = np.zeros(n)
        self._check(self.L.wsa_bins_hz(self.h, float(fs), out.ctypes.data, n))
        return out

    def batch(self, n_samples, fs, resample_to=None):
        """resample_to: analysis rate when the clips handed to run* are at `fs` and are to be converted first (spec RS-1); `fs` may then be a
        sequence with one rate per clip (a folder of files of different rates in one launch)."""
        return Batch(self, n_samples, fs, resample_to)

    def streams(self, n_streams, fs, frames_per_step=1, max_span_frames=1024, resample_to=None):
        """resample_to: analysis rate of a set whose streams arrive at `fs` — one rate, or a sequence with one rate per stream — and are
        converted inside the step (spec RS-1, wsa_stream_create_mixed); streams already at resample_to pass unfiltered."""
        return Streams(self, n_streams, fs, frames_per_step, max_span_frames, resample_to)

    def load_model(self, src):
        """The app's trained classifier on this context's device: `src` = a directory as dist/nnmodel/<db>/cats_<label>/ ships it, a
        (model_json, meta_json, weights_bytes) tuple, or a parsed nnmodel.ModelSpec."""
        from .. import nnmodel
        if isinstance(src, nnmodel.ModelSpec):
            spec = src
        elif isinstance(src, (tuple, list)):
            spec = nnmodel.parse(*src)
        else:
            spec = nnmodel.load_dir(src)
        return Model(self, spec)

    def trainer(self, spec, features, labels, n_val, batch_size, learning_rate):
        """K7 on this context: SGD from the weights of `spec` over host rows (see Trainer; webspeechanalyzer_amd.train drives it)."""
        return Trainer(self, spec, features, labels, n_val, batch_size, learning_rate)

    def regress_trainer(self, spec, features, values, n_val, batch_size, learning_rate, out_min=None, out_max=None):
        """K7 on this context for a regression model (spec TR-2): Adam on the mean squared error from the weights of `spec` over host rows
        and their real-valued targets; the range defaults to spec.out_min / spec.out_max (webspeechanalyzer_amd.train drives it)."""
        return Trainer(self, spec, features, values, n_val, batch_size, learning_rate,
                       regression=(spec.out_min if out_min is None else out_min, spec.out_max if out_max is None else out_max))

    def train_group(self, trainers):
        """K7g on this context: 1 .. 32 of its Trainers (classifiers and regression models alike) stepped in lock step, one launch per
        stage for all of them (see TrainGroup; webspeechanalyzer_amd.train.train_many drives it)."""
        return TrainGroup(self, trainers)

    def feature_db(self, features, durations, vocab_sizes=(), n_ord=0, first_row=0):
        """K8 on this context: a labelled feature DB on the device (see FeatureDBStats; webspeechanalyzer_amd.dbstats drives it)."""
        return FeatureDBStats(self, features, durations, vocab_sizes, n_ord, first_row)

    def device_db(self, width, capacity):
        """K10 on this context: an empty feature DB of `capacity` rows of `width` features that stays on the device (see FeatDB;
        webspeechanalyzer_amd.featdb.DeviceDB drives it)."""
        return FeatDB(self, width, capacity)

    def knn_store(self, width, n_classes, capacity):
        """K9 on this context: an empty ml5 KNN store of `capacity` rows of `width` features (see KnnStore; webspeechanalyzer_amd.knn drives it)."""
        return KnnStore(self, width, n_classes, capacity)

    def ensemble(self, models):
        """The app's `available_DBs` on this context: a list of 1 .. 8 Models in that order (every tie between DBs goes to the earlier one)."""
        return Ensemble(self, models)

    def regress_group(self, models, ranges=None):
        """1 .. 8 regression Models (the app's ords_<label>: V, A, D) as the heads of one grouped launch and of the fold RG-1; ranges = one
        (out_min, out_max) per head, None (or a None entry) for the model's own."""
        return RegressGroup(self, models, ranges)
