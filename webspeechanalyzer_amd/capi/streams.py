"""wsa_stream: live streams advancing in lock step."""
import ctypes
import functools

import numpy as np

from ._abi import (NFEAT, PCM_F32, WsaError, _PCM_DTYPE, _StreamClassResult, _StreamDbResult, _StreamEnsembleResult, _StreamKnnResult, _StreamRows,
                   _StreamValueResult, lib)
from ._util import _Handle, host_copy
from .batch import _track_records
from .pcm import channel_select, pcm_format

ACTIVE, START, STOP = 1, 2, 4        # WSA_STREAM_* control bits
_table = functools.partial(host_copy, null_is_none=True)      # a table the step does not produce at this level comes as a null pointer: None


class Streams(_Handle):
    """n concurrent launches advancing in lock step (wsa_stream): the reference's online path — one
    spectrum_push per frame with carried state, callbacks as segments close (dist/main.js:2 @B8752, @B28869)."""

    _destroy = "wsa_stream_destroy"

    def __init__(self, an, n_streams, fs, frames_per_step=1, max_span_frames=1024, resample_to=None):
        self.an, self.L = an, an.L
        self.n = int(n_streams)
        self.h = ctypes.c_void_p()
        self.mixed = bool(resample_to)
        if np.ndim(fs) > 0 and not resample_to:
            raise WsaError("one rate per stream needs resample_to: a stream set has one geometry")
        if resample_to:
            self.fs_in = np.ascontiguousarray(np.broadcast_to(np.asarray(fs, np.float64), (self.n,)) if np.ndim(fs) == 0 else fs, dtype=np.float64)
            if self.fs_in.shape != (self.n,):
                raise WsaError("fs as a sequence holds one rate per stream")
            self.fs = float(resample_to)
            an._check(self.L.wsa_stream_create_mixed(an.h, self.n, self.fs_in.ctypes.data, self.fs, int(frames_per_step), int(max_span_frames), ctypes.byref(self.h)))
        else:
            self.fs = float(fs)
            self.fs_in = np.full(self.n, self.fs)
            an._check(self.L.wsa_stream_create(an.h, self.n, self.fs, int(frames_per_step), int(max_span_frames), ctypes.byref(self.h)))
        self.samples_per_step = int(self.L.wsa_stream_samples_per_step(self.h))
        self.input_stride = int(self.L.wsa_stream_input_stride(self.h))
        self.input_capacity = np.array([self.L.wsa_stream_input_capacity(self.h, i) for i in range(self.n)], np.uint32)
        self.frame_capacity = int(self.L.wsa_stream_step_frame_capacity(self.h))
        self.input_format, self.channels = PCM_F32, np.ones(self.n, np.uint32)
        self.input_stride_bytes = int(self.L.wsa_stream_input_stride_bytes(self.h))

    def paced_input(self):
        """What n_in=None takes from every stream in the next step (a step without START): [n] uint32."""
        return np.array([self.L.wsa_stream_paced_input(self.h, i) for i in range(self.n)], np.uint32)

    @staticmethod
    def resample_ready(n_in, fs_in, fs_out):
        """Outputs of the first n_in samples whose taps have all arrived (wsa_resample_ready; pure)."""
        return int(lib().wsa_resample_ready(int(n_in), float(fs_in), float(fs_out)))

    def converted(self):
        """After collect(): the converted samples the last step produced, a list of n float32 arrays (a mixed set)."""
        counts = np.zeros(self.n, np.uint32)
        self.an._check(self.L.wsa_stream_copy_converted(self.h, None, 0, counts.ctypes.data))
        cap = max(int(counts.max()), 1)
        out = np.zeros((self.n, cap), np.float32)
        self.an._check(self.L.wsa_stream_copy_converted(self.h, out.ctypes.data, cap, counts.ctypes.data))
        return [out[i, :int(c)].copy() for i, c in enumerate(counts)]

    def enable_graph(self, on=True):
        self.an._check(self.L.wsa_stream_enable_graph(self.h, int(on)))

    def host_input(self):
        """The pinned [n, input_stride] float32 input buffer of step_host (a numpy view; input_stride = samples_per_step on a plain set)."""
        p = self.L.wsa_stream_host_input(self.h)
        return np.ctypeslib.as_array(p, shape=(self.n, self.input_stride))

    @staticmethod
    def _ctl(ctl):
        if ctl is None:
            return None, None
        a = np.ascontiguousarray(ctl, dtype=np.uint8)
        return a, a.ctypes.data

    def step(self, d_pcm, stream_stride, ctl=None, stream=0, n_in=None):
        """n_in: samples per stream in this step ([n] uint32, at most input_capacity); None: paced (a plain set: samples_per_step)."""
        keep, ptr = self._ctl(ctl)
        if n_in is None:
            self.an._check(self.L.wsa_stream_step(self.h, d_pcm, int(stream_stride), ptr, stream))
        else:
            cnt = np.ascontiguousarray(n_in, dtype=np.uint32)
            self.an._check(self.L.wsa_stream_step_n(self.h, d_pcm, int(stream_stride), cnt.ctypes.data, ptr, stream))

    def step_host(self, ctl=None, stream=0, n_in=None):
        keep, ptr = self._ctl(ctl)
        if n_in is None:
            self.an._check(self.L.wsa_stream_step_host(self.h, ptr, stream))
        else:
            cnt = np.ascontiguousarray(n_in, dtype=np.uint32)
            self.an._check(self.L.wsa_stream_step_host_n(self.h, cnt.ctypes.data, ptr, stream))

    def _channels(self, channels):
        """One channel count per stream as uint32 [n] from one number or a sequence (None stays None); the library checks 1 .. 64."""
        if channels is None:
            return None
        ch = np.ascontiguousarray(np.broadcast_to(np.asarray(channels, np.int64), (self.n,)) if np.ndim(channels) == 0 else channels, dtype=np.int64)
        if ch.shape != (self.n,):
            raise WsaError("channels as a sequence holds one count per stream")
        if ch.min() < 0 or ch.max() > 0xFFFFFFFF:
            raise WsaError(f"channel count {int(ch.min() if ch.min() < 0 else ch.max())} outside 1 .. 64")
        return ch.astype(np.uint32)

    def set_input_format(self, fmt, channels=None):
        """The format of the samples the set is fed from now on (spec PK-1, wsa_stream_set_input_format): 'f32' (the default), 'i16', 'mulaw'
        or 'alaw' (or a PCM_* number); channels = interleaved channels per stream, one number or one per stream (1 .. 64, channel 0 is
        analysed).  Legal before the first step and between a collect() and the next step; the next step recaptures the graph."""
        f = pcm_format(fmt)
        ch = self._channels(channels)
        self.an._check(self.L.wsa_stream_set_input_format(self.h, f, ch.ctypes.data if ch is not None else None))
        self.input_format = f
        self.channels = ch if ch is not None else np.ones(self.n, np.uint32)
        self.input_stride_bytes = int(self.L.wsa_stream_input_stride_bytes(self.h))

    def set_input_channels(self, fmt, channels=None, select=None, source=None):
        """set_input_format() with a select and a source per stream (spec PK-3, wsa_stream_set_input_channels): stream i takes channel select[i]
        ('mix': the mono mix; None: channel 0; one value for all is fine) of the packed row of stream source[i] (None: its own).  The host fills
        one row per source; counts and control bytes stay per stream."""
        f = pcm_format(fmt)
        ch = self._channels(channels)
        sel = None
        if select is not None:
            sv = [select] * self.n if isinstance(select, (str, int)) else list(select)
            if len(sv) != self.n:
                raise WsaError("one select (a channel index or 'mix') per stream")
            sel = np.asarray([channel_select(v) for v in sv], np.uint32)
        src = None
        if source is not None:
            src = np.ascontiguousarray(source, dtype=np.int64)
            if src.shape != (self.n,) or src.min() < 0 or src.max() > 0xFFFFFFFF:
                raise WsaError("one source (a stream index) per stream")
            src = src.astype(np.uint32)
        self.an._check(self.L.wsa_stream_set_input_channels(self.h, f, ch.ctypes.data if ch is not None else None, sel.ctypes.data if sel is not None else None,
                                                            src.ctypes.data if src is not None else None))
        self.input_format = f
        self.channels = ch if ch is not None else np.ones(self.n, np.uint32)
        self.input_stride_bytes = int(self.L.wsa_stream_input_stride_bytes(self.h))

    def host_input_packed(self):
        """The pinned packed input buffer of step_host while a packed format is set: a numpy view, int16 ('i16') or uint8 (G.711), shape
        [n, input_stride_bytes / itemsize]; stream i's interleaved frames of the step at the start of row i."""
        p = self.L.wsa_stream_host_input_packed(self.h)
        if not p:
            raise WsaError("no packed input buffer: the input format is 'f32' (set_input_format)")
        dt = np.dtype(_PCM_DTYPE[self.input_format])
        stride = int(self.L.wsa_stream_input_stride_bytes(self.h))
        ctype = ctypes.c_int16 if dt == np.int16 else ctypes.c_uint8
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(self.n, stride // dt.itemsize))

    def step_packed(self, d_ptr, stride_bytes, ctl=None, stream=0, n_in=None):
        """One step on device-resident packed input (wsa_stream_step_packed): stream i's interleaved frames at d_ptr + i * stride_bytes
        (16-byte aligned, stride_bytes a multiple of 16); n_in as for step()."""
        keep, ptr = self._ctl(ctl)
        cnt = None if n_in is None else np.ascontiguousarray(n_in, dtype=np.uint32)
        self.an._check(self.L.wsa_stream_step_packed(self.h, d_ptr, int(stride_bytes), cnt.ctypes.data if cnt is not None else None, ptr, stream))

    def time_steps_packed(self, n_steps, feed=None, stream=0):
        """time_steps() on a packed set: feed = [k, n, input_stride_bytes / itemsize] blocks of the format's dtype, or None."""
        out = np.zeros(n_steps)
        rows = ctypes.c_uint64(0)
        fptr, fk = None, 0
        if feed is not None:
            feed = np.ascontiguousarray(feed)
            stride = int(self.L.wsa_stream_input_stride_bytes(self.h))
            assert feed.ndim == 3 and feed.shape[1] == self.n and feed.shape[2] * feed.dtype.itemsize == stride, "feed blocks are [k, n, input_stride_bytes / itemsize]"
            fptr, fk = feed.ctypes.data, feed.shape[0]
        self.an._check(self.L.wsa_stream_time_steps_packed(self.h, int(n_steps), fptr, int(fk), stream, out.ctypes.data, ctypes.byref(rows)))
        return out, rows.value

    def time_steps(self, n_steps, feed=None, stream=0):
        """n_steps steps timed inside the library (step_host + collect, microseconds each); feed = [k, n, input_stride] float32
        blocks copied into the pinned input before each step (cycled), or None.  Returns (us array, rows produced)."""
        out = np.zeros(n_steps)
        rows = ctypes.c_uint64(0)
        fptr, fk = None, 0
        if feed is not None:
            feed = np.ascontiguousarray(feed, dtype=np.float32)
            assert feed.ndim == 3 and feed.shape[1:] == (self.n, self.input_stride)
            fptr, fk = feed.ctypes.data, feed.shape[0]
        self.an._check(self.L.wsa_stream_time_steps(self.h, int(n_steps), fptr, int(fk), stream, out.ctypes.data, ctypes.byref(rows)))
        return out, rows.value

    def set_model(self, model):
        """Attach a Model (K6 on every step's rows; at level 13 the fold, one accumulator per stream reset by START) or detach (None).
        The next step recaptures the graph."""
        self.an._check(self.L.wsa_stream_set_model(self.h, model.h if model is not None else None))
        self._model = model

    def classes(self):
        """After collect(): host copies of the step's classification, dict(prob [n_rows, C] f32, cb [n_cb, 4] i32 = {stream, si, first row,
        rows}, cb_label [n_cb] i32 (-1: null, -2: not predicted), cb_conf [n_cb] f64, stream_conf [n, C] f64 = Label_conf_all since each
        stream's START, labels).  Level 5: cb / cb_label / cb_conf / stream_conf are None."""
        r = _StreamClassResult()
        self.an._check(self.L.wsa_stream_classes(self.h, ctypes.byref(r)))
        n, C, k = int(r.n_rows), int(r.n_classes), int(r.n_callbacks)
        return dict(prob=_table(r.prob, np.float32, (n, C)), cb=_table(r.cb, np.int32, (k, 4)), cb_label=_table(r.cb_label, np.int32, (k,)),
                    cb_conf=_table(r.cb_conf, np.float64, (k,)), stream_conf=_table(r.stream_conf, np.float64, (int(r.n_streams), C)),
                    labels=list(self._model.labels))

    def set_knn(self, store, k=10):
        """Attach a KnnStore (K9s on every step's rows; at level 13 the fold KN-2, one accumulator per stream reset by START) or detach
        (None).  Stands beside a Model or an Ensemble; the next step recaptures the graph.  The store's rows are those at this call."""
        self.an._check(self.L.wsa_stream_set_knn(self.h, store.h if store is not None else None, int(k)))
        self._knn = store

    def knn_classes(self):
        """After collect(): host copies of the step's KNN tables, dict(label [n_rows] i32, conf [n_rows, C] f64, nbr [n_rows, k] i32,
        sim [n_rows, k] f32, k_eff, slices, cb [n_cb, 4] i32 = {stream, si, first row, rows}, cb_label [n_cb] i32 (a class index; -1: null,
        -2: not predicted), cb_conf [n_cb] f64, stream_conf [n, C] f64).  Level 5: cb / cb_label / cb_conf / stream_conf are None."""
        r = _StreamKnnResult()
        self.an._check(self.L.wsa_stream_knn_classes(self.h, ctypes.byref(r)))
        n, C, k, ncb = int(r.n_rows), int(r.n_classes), int(r.k), int(r.n_callbacks)
        arr, i32, f64 = _table, np.int32, np.float64
        return dict(label=arr(r.label, i32, (n,)), conf=arr(r.conf, f64, (n, C)), nbr=arr(r.nbr, i32, (n, k)), sim=arr(r.sim, np.float32, (n, k)),
                    k_eff=int(r.k_eff), slices=int(r.slices), cb=arr(r.cb, i32, (ncb, 4)), cb_label=arr(r.cb_label, i32, (ncb,)),
                    cb_conf=arr(r.cb_conf, f64, (ncb,)), stream_conf=arr(r.stream_conf, f64, (int(r.n_streams), C)))

    def set_regress(self, group):
        """Attach a RegressGroup (the grouped K6 on every step's rows; at level 13 the fold RG-1, the running sums of every (stream, head)
        reset by START) or detach (None).  Stands beside a Model or an Ensemble and a KnnStore; the next step recaptures the graph."""
        self.an._check(self.L.wsa_stream_set_regress(self.h, group.h if group is not None else None))
        self._group = group

    def values(self):
        """After collect(): host copies of the step's regression tables, dict(value [H, n_rows] f64, cb [n_cb, 4] i32 = {stream, si, first
        row, rows}, cb_value / cb_weight [H, n_cb] f64, stream_sum / stream_weight / stream_value [H, n] f64 since each stream's START).
        Level 5: value only, the others None."""
        r = _StreamValueResult()
        self.an._check(self.L.wsa_stream_values(self.h, ctypes.byref(r)))
        H, n, k, ns = int(r.n_heads), int(r.n_rows), int(r.n_callbacks), int(r.n_streams)

        def per_head(ptrs, m):
            cols = [_table(ptrs[h], np.float64, (m,)) for h in range(H)]
            return None if any(c is None for c in cols) else np.stack(cols) if cols else np.zeros((0, m))
        return dict(value=per_head(r.value, n), cb=_table(r.cb, np.int32, (k, 4)), cb_value=per_head(r.cb_value, k),
                    cb_weight=per_head(r.cb_weight, k), stream_sum=per_head(r.stream_sum, ns), stream_weight=per_head(r.stream_weight, ns),
                    stream_value=per_head(r.stream_value, ns))

    def set_featdb(self, db):
        """Attach a FeatDB (every step appends its rows to it on the device, spec FD-2: two kernels of the step) or detach (None).  Stands
        beside every other attachment; the next step recaptures the graph.  The DB's count advances at collect()."""
        self.an._check(self.L.wsa_stream_set_featdb(self.h, db.h if db is not None else None))
        self._featdb = db

    @staticmethod
    def featdb_tile_info():
        """(rows per wave tile, rows per step of the plan kernel's walk, stored rows per copy tile, the copy kernel's largest grid)."""
        v = [ctypes.c_int32() for _ in range(4)]
        lib().wsa_stream_featdb_tile_info(*[ctypes.byref(x) for x in v])
        return tuple(x.value for x in v)

    def db_rows(self):
        """After collect(): what the step stored in the attached DB, dict(first_row, n_added, n_replaced, not_fitted, kept [n_added] i32 =
        the collected row (level 11: utterance row) behind DB row first_row + i, replaced [n_replaced, 2] i32 = {utterance row, DB row}
        (level 11; else None))."""
        r = _StreamDbResult()
        self.an._check(self.L.wsa_stream_db_rows(self.h, ctypes.byref(r)))
        na, nr = int(r.n_added), int(r.n_replaced)
        return dict(first_row=int(r.first_row), n_added=na, n_replaced=nr, not_fitted=int(r.not_fitted), kept=host_copy(r.kept, np.int32, (na,)),
                    replaced=_table(r.replaced, np.int32, (nr, 2)))

    def set_ensemble(self, ensemble):
        """Attach an Ensemble (K6e on every step's rows; at level 13 one accumulator per stream and member and one running min_entropy_db
        per stream, reset by START) or detach (None).  Detaches a Model; the next step recaptures the graph."""
        self.an._check(self.L.wsa_stream_set_ensemble(self.h, ensemble.h if ensemble is not None else None))
        self._ensemble = ensemble

    def ensemble_classes(self):
        """After collect(): host copies of the step's ensemble classification, the tables of Batch.ensemble_classes with `stream` for `clip`
        (stream_conf, stream_min_db).  Level 5: prob only."""
        r = _StreamEnsembleResult()
        self.an._check(self.L.wsa_stream_ensemble_classes(self.h, ctypes.byref(r)))
        nm, n, k, ns = int(r.n_members), int(r.n_rows), int(r.n_callbacks), int(r.n_streams)
        C = [int(r.n_classes[d]) for d in range(nm)]
        arr, i32, f64 = host_copy, np.int32, np.float64
        out = dict(prob=[arr(r.prob[d], np.float32, (n, C[d])) for d in range(nm)], labels=[list(m.labels) for m in self._ensemble.models])
        if not r.cb:
            return out
        out.update(cb_label=[arr(r.cb_label[d], i32, (k,)) for d in range(nm)], cb_conf=[arr(r.cb_conf[d], f64, (k,)) for d in range(nm)],
                   cb_all_max=[arr(r.cb_all_max[d], f64, (k,)) for d in range(nm)],
                   stream_conf=[arr(r.stream_conf[d], f64, (ns, C[d])) for d in range(nm)],
                   cb=arr(r.cb, i32, (k, 4)), cb_db=arr(r.cb_db, i32, (k,)), cb_top_label=arr(r.cb_top_label, i32, (k,)),
                   cb_top_conf=arr(r.cb_top_conf, f64, (k,)), cb_min_db=arr(r.cb_min_db, i32, (k,)), cb_entropy=arr(r.cb_entropy, f64, (k,)),
                   stream_min_db=arr(r.stream_min_db, i32, (ns,)))
        return out

    def collect(self, stream=0):
        """Rows of the last step: dict(meta [n,8] i32, feat [n,53] f64, segments [m,4] i32) (copies)."""
        r = _StreamRows()
        self.an._check(self.L.wsa_stream_collect(self.h, stream, ctypes.byref(r)))
        n, m = r.n_rows, r.n_segments
        out = dict(meta=host_copy(r.row_meta, np.int32, (n, 8)), feat=host_copy(r.row_feat, np.float64, (n, NFEAT)), segments=host_copy(r.segments, np.int32, (m, 4)),
                   cuts=host_copy(r.stream_cuts, np.uint32, (self.n,)), flags=int(r.status_flags))
        if r.utt_feat:                                  # level 11: one 264-vector per result of the step
            nu = int(r.n_utterance_rows)
            out["utt_meta"] = host_copy(r.utt_meta, np.int32, (nu, 4))
            out["utt_feat"] = host_copy(r.utt_feat, np.float64, (nu, 264))
        if r.track_off:                                 # level 3: ranked raw tracks of the step's segments (the layout of Batch.tracks())
            npt, nrk = int(r.n_track_points), int(r.n_track_ranked)
            out["track_off"] = host_copy(r.track_off, np.uint64, (m + 1, 2))
            out["track_points"] = host_copy(r.track_points, np.int32, (npt, 8))
            out["track_ranked"] = host_copy(r.track_ranked, np.int32, (nrk,))
            out["tracks"] = _track_records(out["track_off"], out["track_points"], out["track_ranked"], m)
        if r.formants and r.row_formant_off:           # levels 4 / 10: frames of row k = formants[formant_off[k]:formant_off[k + 1]]
            off = host_copy(r.row_formant_off, np.uint32, (r.n_rows + 1,))
            out["formant_off"] = off
            out["formants"] = host_copy(r.formants, np.float32, (int(off[-1]), 9))
        return out
