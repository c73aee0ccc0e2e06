"""wsa_batch: a planned batch of clips, its runs and the host copies of their results."""
import ctypes

import numpy as np

from ._abi import (NFEAT, WsaError, _BatchInfo, _ClassResult, _DeviceResult, _EnsembleHost, _EnsembleResult, _KnnFoldResult, _KnnResult, _PCM_DTYPE,
                   _PCM_ELEMS, _ValueHost, _ValueResult)
from ._util import _Handle
from .pcm import _pcm_array, channel_select, pcm_format


def _track_records(seg_off, pts, rk, n_segments):
    """the reference's 18-field track records per segment from the per-point entries (layout: include/wsa.h wsa_batch_copy_tracks)."""
    num = lambda x: int(x) if float(x).is_integer() else float(x)
    out = []
    for k in range(n_segments):
        p0, p1 = int(seg_off[k][0]), int(seg_off[k + 1][0])
        r0, r1 = int(seg_off[k][1]), int(seg_off[k + 1][1])
        per = {}
        for q in pts[p0:p1]:
            per.setdefault(int(q[0]), []).append(q)
        seg = []
        for t in rk[r0:r1]:
            P = per[int(t)]
            frames = [int(q[6]) for q in P]; starts = [int(q[4]) for q in P]; ends = [int(q[7]) for q in P]
            bins = [int(q[1]) & 0xff for q in P]; amps = [int(np.uint32(q[5])) for q in P]
            en = [float(np.array([q[2], q[3]], np.int32).view(np.float64)[0]) for q in P]
            h = len(P) - 1                                   # the velocity of the last update (ref @B36624), from the bins before it
            pb = bins[-1]
            vel = 0.0 if h == 0 else (pb - bins[0] if h == 1 else (((pb - bins[1]) + (bins[0] - bins[1])) / 2 if h == 2
                                      else ((pb - bins[h - 1]) + (bins[h - 2] - bins[h - 1]) + (bins[h - 3] - bins[h - 2])) / 3))
            sE = 0.0; sEb = 0.0; sW = 0
            for b_, e_, st_, en_ in zip(bins, en, starts, ends):
                sE += e_; sEb += e_ * b_; sW += en_ - st_ + 1
            seg.append([starts[-1], ends[-1], frames[-1], frames[-1], num(vel), pb, amps[-1], frames, starts, ends, bins, amps,
                        [num(e_) for e_ in en], num(sE), len(P), num(sEb), 0, sW])
        out.append(seg)
    return out


def rows_to_callbacks(level, step, meta, feat, payload):
    """One clip's compacted rows (meta [n, 8] i32 = {clip, si, t_start, t_len, ..}, feat [n, 53]) as the callbacks the reference's dispatcher delivers
    for them: levels 4 / 5 one per row with the time pair as numbers, levels 10 / 12 / 13 one per result with the syllables' time pairs as the
    reference's toFixed(3) strings.  step = window_step in seconds; payload(m, f) = what the row hands over.  Other levels have no row callbacks."""
    cbs = []
    if level in (4, 5):
        for m, f in zip(meta, feat):
            cbs.append([int(m[1]), [], [m[2] * step, (m[3] + 1) * step], payload(m, f)])
    elif level in (10, 12, 13):
        i = 0
        while i < len(meta):
            j = i
            while j < len(meta) and meta[j][1] == meta[i][1]:
                j += 1
            tm = [["%.3f" % (m[2] * step), "%.3f" % ((m[3] + 1) * step)] for m in meta[i:j]]
            rows_ = list(zip(meta[i:j], feat[i:j]))
            if level == 12:                  # numeric threw on a syllable: the reference keeps the rows before it
                cut = next((q for q, (_, f) in enumerate(rows_) if f[23] != 0), len(rows_))
                rows_ = rows_[:cut]
            if level != 12 or rows_:
                cbs.append([int(meta[i][1]), [], tm, [payload(m, f) for m, f in rows_]])
            i = j
    return cbs


class Batch(_Handle):
    """A planned batch shape (wsa_batch).  `run*` take raw device pointers (e.g. torch data_ptr())."""
    _destroy = "wsa_batch_destroy"

    def __init__(self, an, n_samples, fs, resample_to=None):
        self.an, self.L = an, an.L
        self.n_samples = np.ascontiguousarray(n_samples, dtype=np.uint32)
        self.fs = float(fs) if np.ndim(fs) == 0 else None
        self.h = ctypes.c_void_p()
        if self.fs is None and not resample_to:
            raise WsaError("one rate per clip needs resample_to: a launch has one geometry")
        if resample_to and np.ndim(fs) > 0:              # one rate per clip (wsa_batch_create_mixed); clips already at resample_to pass unfiltered
            self.n_samples_in, self.fs_in, self.fs = self.n_samples, np.ascontiguousarray(fs, dtype=np.float64), float(resample_to)
            if self.fs_in.shape != self.n_samples_in.shape:
                raise WsaError("fs as a sequence holds one rate per clip")
            an._check(self.L.wsa_batch_create_mixed(an.h, len(self.n_samples_in), self.n_samples_in.ctypes.data, self.fs_in.ctypes.data, self.fs, ctypes.byref(self.h)))
            self.n_samples = np.array([self.L.wsa_resample_length(int(n), float(f), self.fs) for n, f in zip(self.n_samples_in, self.fs_in)], np.uint32)
        elif resample_to:
            self.n_samples_in, self.fs_in, self.fs = self.n_samples, self.fs, float(resample_to)
            an._check(self.L.wsa_batch_create_resampled(an.h, len(self.n_samples_in), self.n_samples_in.ctypes.data, self.fs_in, self.fs, ctypes.byref(self.h)))
            self.n_samples = np.array([self.L.wsa_resample_length(int(n), self.fs_in, self.fs) for n in self.n_samples_in], np.uint32)
        else:
            an._check(self.L.wsa_batch_create(an.h, len(self.n_samples), self.n_samples.ctypes.data, self.fs, ctypes.byref(self.h)))
        info = _BatchInfo()
        an._check(self.L.wsa_batch_get_info(self.h, ctypes.byref(info)))
        self.info = {k: getattr(info, k) for k, _ in _BatchInfo._fields_}

    def run(self, d_pcm, clip_stride, stream=0):
        self.an._check(self.L.wsa_batch_run(self.h, d_pcm, int(clip_stride), stream))

    def run_frontend(self, d_pcm, clip_stride, stream=0):
        self.an._check(self.L.wsa_batch_run_frontend(self.h, d_pcm, int(clip_stride), stream))

    def run_backend(self, d_spectra, stream=0):
        self.an._check(self.L.wsa_batch_run_backend(self.h, d_spectra, stream))

    def converted_pcm(self, stream=0):
        """Resampling batch, after a run: the clips at the analysis rate, [n_clips, longest] float32 (zero padded)."""
        stride = max(int(self.n_samples.max()) if len(self.n_samples) else 0, 1)
        out = np.zeros((len(self.n_samples), stride), np.float32)
        self.an._check(self.L.wsa_batch_copy_pcm(self.h, stream, out.ctypes.data, stride))
        return out

    def run_host(self, clips, stream=0):
        clips = [np.ascontiguousarray(c, dtype=np.float32) for c in clips]
        ptrs = (ctypes.c_void_p * len(clips))(*[c.ctypes.data for c in clips])
        self.an._check(self.L.wsa_batch_run_host(self.h, ptrs, stream))

    def run_host_i16(self, clips, channels=None, stream=0):
        """16-bit PCM in host memory (clip i interleaved over channels[i] channels, channel 0 analysed); converted on the device."""
        clips = [np.ascontiguousarray(c, dtype=np.int16) for c in clips]
        ptrs = (ctypes.c_void_p * len(clips))(*[c.ctypes.data for c in clips])
        ch = None if channels is None else (ctypes.c_uint32 * len(clips))(*[int(c) for c in channels])
        self.an._check(self.L.wsa_batch_run_host_i16(self.h, ptrs, ch, stream))

    def _formats(self, formats, channels):
        n = len(self.n_samples)
        fm = [formats] * n if isinstance(formats, (str, int)) else list(formats)
        if len(fm) != n or (channels is not None and len(channels) != n):
            raise WsaError("one format (and one channel count) per clip")
        # (numbers go to the library as they are: it names the clip when it refuses one)
        fm = (ctypes.c_int32 * max(n, 1))(*[pcm_format(f) if isinstance(f, str) else int(f) for f in fm])
        ch = None if channels is None else (ctypes.c_uint32 * max(n, 1))(*[int(c) for c in channels])
        return fm, ch

    def _clip_arrays(self, clips, fm, ch, src=None):
        """Per clip its flat array of the format's sample type, holding at least the plan's frames; None for a clip that names another as its source."""
        held = []
        ns_in = getattr(self, "n_samples_in", self.n_samples)
        for i, c in enumerate(clips):
            if src is not None and int(src[i]) != i:
                held.append(None)
                continue
            f = int(fm[i])
            a = _pcm_array(f, f, c) if f in _PCM_DTYPE else np.ascontiguousarray(c).reshape(-1)
            need = int(ns_in[i]) * (int(ch[i]) if ch is not None else 1) * _PCM_ELEMS.get(f, 1)
            if f in _PCM_DTYPE and a.size < need:
                raise WsaError(f"clip {i}: {a.size} elements, the plan's {int(ns_in[i])} frames need {need}")
            held.append(a)
        return held

    def run_host_packed(self, clips, formats, channels=None, stream=0):
        """Clips in host memory as the bytes a file holds (spec PK-2): clip i in formats[i] ('f32', 'i16', 'mulaw', 'alaw', 'u8', 'i24', 'i32',
        'f64' or the numbers; one name for all clips is fine), interleaved over channels[i] channels, channel 0 analysed; unpacked on the device.
        The arrays have the format's sample type (as pcm_decode takes them) and hold at least the plan's frames."""
        fm, ch = self._formats(formats, channels)
        held = self._clip_arrays(clips, fm, ch)
        ptrs = (ctypes.c_void_p * max(len(held), 1))(*[a.ctypes.data for a in held])
        self.an._check(self.L.wsa_batch_run_host_packed(self.h, ptrs, fm, ch, stream))

    def set_input_format(self, formats, channels=None):
        """Plans the device-resident packed layout (wsa_batch_set_input_format): packed_offsets() says where each clip's bytes go."""
        fm, ch = self._formats(formats, channels)
        self.an._check(self.L.wsa_batch_set_input_format(self.h, fm, ch))

    def packed_offsets(self):
        """uint64 [n_clips + 1]: clip i's bytes start at offset i (a multiple of 16) of the packed buffer, the last entry is the buffer's size."""
        return np.array([self.L.wsa_batch_packed_offset(self.h, i) for i in range(len(self.n_samples) + 1)], np.uint64)

    def run_packed(self, d_packed, stream=0):
        """Device-resident packed clips at d_packed + packed_offsets()[i] (a raw device pointer, 16-byte aligned): kernel launches only."""
        self.an._check(self.L.wsa_batch_run_packed(self.h, d_packed, stream))

    def _select_source(self, select, source):
        n = len(self.n_samples)
        sel = None
        if select is not None:
            sv = [select] * n if isinstance(select, (str, int)) else list(select)
            if len(sv) != n:
                raise WsaError("one select (a channel index or 'mix') per clip")
            sel = (ctypes.c_uint32 * max(n, 1))(*[channel_select(v) for v in sv])
        src = None
        if source is not None:
            if len(source) != n:
                raise WsaError("one source (a clip index) per clip")
            if any(int(v) < 0 or int(v) > 0xFFFFFFFF for v in source):
                raise WsaError("a source is a clip index")
            src = (ctypes.c_uint32 * max(n, 1))(*[int(v) for v in source])
        return sel, src

    def set_input_channels(self, formats, channels=None, select=None, source=None):
        """Plans the device-resident layout of spec PK-3 (wsa_batch_set_input_channels): clip i takes channel select[i] ('mix': the mono mix; None:
        channel 0) of the bytes of clip source[i] (None: its own).  Only sources have bytes: packed_offsets()[i] of a consumer is its source's
        offset, the last entry the buffer's size.  run_packed() then runs it."""
        fm, ch = self._formats(formats, channels)
        sel, src = self._select_source(select, source)
        self.an._check(self.L.wsa_batch_set_input_channels(self.h, fm, ch, sel, src))

    def run_host_channels(self, clips, formats, channels=None, select=None, source=None, stream=0):
        """run_host_packed() with a select and a source per clip (spec PK-3, wsa_batch_run_host_channels): a source's bytes are uploaded once and
        feed every clip that names it; clips[i] of a consumer is not read (None is fine)."""
        fm, ch = self._formats(formats, channels)
        sel, src = self._select_source(select, source)
        held = self._clip_arrays(clips, fm, ch, src)
        if len(held) != len(self.n_samples):
            raise WsaError("one entry per clip (a consumer's may be None)")
        arr = (ctypes.c_void_p * max(len(held), 1))(*[None if a is None else a.ctypes.data for a in held])
        self.an._check(self.L.wsa_batch_run_host_channels(self.h, arr, fm, ch, sel, src, stream))

    def enable_timing(self, on):
        self.an._check(self.L.wsa_batch_enable_timing(self.h, int(on)))

    def keep_spectra(self, on=True):
        """Kept for older hosts: the u32 frames are always stored (spectra())."""
        self.an._check(self.L.wsa_batch_keep_spectra(self.h, int(on)))
        return self

    def backend_reruns(self):
        n = ctypes.c_uint32(0)
        self.an._check(self.L.wsa_batch_backend_reruns(self.h, ctypes.byref(n)))
        return n.value

    def keep_counters(self, on=True):
        """Test entry (csrc/debug.hip, not part of wsa.h): the batch's runs leave their device counters standing for tiers()."""
        self.an._check(self.L.wsa_debug_batch_keep_counters(self.h, int(on)))
        return self

    def tiers(self, stream=0):
        """Test entry: dict(flags, spans, redo) of the last run — the flag word (bit 1: the 140-entry track table overflowed), the number of spans and
        how many of them the paired tracker kernel handed to the one-span kernel.  Needs keep_counters() before the run, and is to be read before
        the first fetch of results (rows(), callbacks(), ...): a fetch that finds flag bit 1 reruns the back end, and these are the rerun's then."""
        out = (ctypes.c_uint32 * 3)()
        self.an._check(self.L.wsa_debug_batch_tiers(self.h, stream, out))
        return dict(flags=int(out[0]), spans=int(out[1]), redo=int(out[2]))

    def enable_trace(self, on=True):
        self.an._check(self.L.wsa_batch_enable_trace(self.h, int(on)))

    def trace(self, stream=0):
        n = self.info["n_frames_total"]
        out = np.zeros((n, 12))
        self.an._check(self.L.wsa_batch_copy_trace(self.h, stream, out.ctypes.data, max(n, 1)))
        return out

    def device_result(self, stream=0):
        r = _DeviceResult()
        self.an._check(self.L.wsa_batch_result(self.h, stream, ctypes.byref(r)))
        return r

    def stage_ms(self):
        out = np.zeros(4, np.float32)
        self.an._check(self.L.wsa_batch_stage_ms(self.h, out.ctypes.data))
        return out

    def rows(self, stream=0):
        """Host copies: dict(meta [n,8] i32, feat [n,53] f64, segments [m,4] i32, row_off, seg_off)."""
        r = self.device_result(stream)
        n, m, nc = r.n_rows, r.n_segments, r.n_clips
        meta = np.zeros((n, 8), np.int32)
        feat = np.zeros((n, NFEAT), np.float64)
        segs = np.zeros((m, 4), np.int32)
        roff = np.zeros(nc + 1, np.uint32)
        soff = np.zeros(nc + 1, np.uint32)
        self.an._check(self.L.wsa_batch_copy_rows(self.h, stream, meta.ctypes.data, feat.ctypes.data, max(n, 1),
                                                   segs.ctypes.data, max(m, 1), roff.ctypes.data, soff.ctypes.data))
        return dict(meta=meta, feat=feat, segments=segs, row_off=roff, seg_off=soff)

    def row_meta(self, stream=0):
        """The row metadata alone, [n, 8] i32: the features stay on the device (featdb.DeviceDB)."""
        n = self.device_result(stream).n_rows
        meta = np.zeros((n, 8), np.int32)
        self.an._check(self.L.wsa_batch_copy_rows(self.h, stream, meta.ctypes.data, None, max(n, 1), None, 0, None, None))
        return meta

    def utterance_meta(self, stream=0):
        """level 11: the utterance metadata alone, [n, 4] i32."""
        n = self.device_result(stream).n_utterance_rows
        meta = np.zeros((n, 4), np.int32)
        self.an._check(self.L.wsa_batch_copy_utterance(self.h, stream, meta.ctypes.data, None, max(n, 1), None))
        return meta

    def spectra(self, stream=0):
        words = self.info["n_frames_total"] * self.info["bands"]
        out = np.zeros((self.info["n_frames_total"], self.info["bands"]), np.uint32)
        foff = np.zeros(self.info["n_clips"] + 1, np.uint32)
        self.an._check(self.L.wsa_batch_copy_spectra(self.h, stream, out.ctypes.data, max(words, 1), foff.ctypes.data))
        return out, foff

    def formants(self, stream=0):
        """levels 4 / 10: the [n_frames_total, 9] float32 table of straightened frames."""
        n = self.info["n_frames_total"]
        out = np.zeros((n, 9), np.float32)
        self.an._check(self.L.wsa_batch_copy_formants(self.h, stream, out.ctypes.data, max(n, 1)))
        return out

    def utterance(self, stream=0):
        """level 11: dict(meta [n,4] i32 = {clip, result index, t_start, t_sum}, feat [n,264] f64, off [n_clips+1])."""
        r = self.device_result(stream)
        n = r.n_utterance_rows
        meta = np.zeros((n, 4), np.int32)
        feat = np.zeros((n, 264), np.float64)
        off = np.zeros(len(self.n_samples) + 1, np.uint32)
        self.an._check(self.L.wsa_batch_copy_utterance(self.h, stream, meta.ctypes.data, feat.ctypes.data, max(n, 1), off.ctypes.data))
        return dict(meta=meta, feat=feat, off=off)

    def tracks(self, stream=0):
        """Level 3: per segment (in d_segments order) the ranked raw tracks as the reference's 18-field records
        (ref accumulate_fm @B35952; field map SURVEY.md App. A), rebuilt from the per-point entries the device hands out:
        [0] start [1] end [2],[3] last frame [4] velocity [5] last bin [6] last amp [7] frames [8] starts [9] ends [10] bins
        [11] amps [12] energies [13] sum E [14] count [15] sum E*bin [16] 0 [17] sum width."""
        class _TI(ctypes.Structure):
            _fields_ = [("n_segments", ctypes.c_uint32), ("n_points", ctypes.c_uint64), ("n_ranked", ctypes.c_uint64)]
        ti = _TI()
        self.an._check(self.L.wsa_batch_tracks_info(self.h, stream, ctypes.byref(ti)))
        seg_off = np.zeros((ti.n_segments + 1, 2), np.uint64)
        pts = np.zeros((max(int(ti.n_points), 1), 8), np.int32)
        rk = np.zeros(max(int(ti.n_ranked), 1), np.int32)
        self.an._check(self.L.wsa_batch_copy_tracks(self.h, stream, seg_off.ctypes.data, pts.ctypes.data, int(ti.n_points), rk.ctypes.data, int(ti.n_ranked)))
        return _track_records(seg_off, pts, rk, ti.n_segments)

    def callbacks(self, stream=0):
        """Per clip, the callback sequence of the reference's dispatcher (dist/main.js:2 @B28869) in the
        same shape tests/golden/gen/ref_driver.js records: [si, label, seg_time, features]."""
        r = self.rows(stream)
        level = int(self.an.config["output_level"])
        step = float(self.an.config["window_step"]) / 1e3
        utt = self.utterance(stream) if level == 11 else None
        trk = self.tracks(stream) if level == 3 else None
        fm = self.formants(stream) if level in (4, 10) else None
        foff = None
        if fm is not None:
            foff = np.zeros(len(self.n_samples) + 1, np.uint32)
            self.an._check(self.L.wsa_batch_copy_spectra(self.h, stream, None, 0, foff.ctypes.data))
        out = []
        for c in range(len(self.n_samples)):
            a, b = int(r["row_off"][c]), int(r["row_off"][c + 1])
            meta, feat = r["meta"][a:b], r["feat"][a:b]
            cbs = []
            payload = (lambda m, f: f[:23].copy() if level == 12 else f.copy()) if fm is None else (lambda m, f: fm[int(foff[c]) + m[6]: int(foff[c]) + m[6] + m[7]].copy())
            if level == 11:
                for k in range(int(utt["off"][c]), int(utt["off"][c + 1])):
                    m = utt["meta"][k]
                    cbs.append([0, [], [m[2] * step, (m[3] + 1) * step], utt["feat"][k].copy()])
            else:
                cbs = rows_to_callbacks(level, step, meta, feat, payload)
            sa, sb = int(r["seg_off"][c]), int(r["seg_off"][c + 1])
            if level == 3:                           # ref @B30132: `s[e].length > 0 && b(e, label, s[e])` (three arguments)
                cbs = [[k, [], trk[sa + k]] for k in range(sb - sa) if len(trk[sa + k]) > 0]
            out.append(dict(callbacks=cbs, segments_ci=[[int(s[1]), int(s[2])] for s in r["segments"][sa:sb]],
                            flags=[int(s[3]) for s in r["segments"][sa:sb]], meta=meta))
        return out

    def classify(self, model, stream=0):
        """K6 (+ K6b at level 13) on the rows of the last run, enqueued on `stream` (wsa_batch_classify).  Level 11 takes a 264-input
        model and classifies the utterance rows (utterance()'s order), level 12 a 23-input model over slots 0 .. 22 of the rows (NaN
        for a row whose fit threw); both give prob only."""
        self.an._check(self.L.wsa_batch_classify(self.h, model.h, stream))
        self._model = model

    def class_result(self, stream=0):
        r = _ClassResult()
        self.an._check(self.L.wsa_batch_class_result(self.h, stream, ctypes.byref(r)))
        return r

    def classes(self, stream=0):
        """Host copies of the last classification: dict(prob [n_rows, C] f32, cb [n_cb, 4] i32 = {clip, si, first row, rows},
        cb_label [n_cb] i32 (-1: null, -2: not predicted), cb_conf [n_cb] f64, clip_conf [n_clips, C] f64, labels)."""
        r = self.class_result(stream)
        C, n, k = int(r.n_classes), int(r.n_rows), int(r.n_callbacks)
        prob, cb = np.zeros((n, C), np.float32), np.zeros((k, 4), np.int32)
        lab, conf = np.zeros(k, np.int32), np.zeros(k, np.float64)
        clip = np.zeros((int(r.n_clips), C), np.float64) if r.d_clip_conf else np.zeros((0, C))
        self.an._check(self.L.wsa_batch_copy_classes(self.h, stream, prob.ctypes.data, max(n, 1), cb.ctypes.data, lab.ctypes.data, conf.ctypes.data,
                                                      max(k, 1), clip.ctypes.data if r.d_clip_conf else None))
        return dict(prob=prob, cb=cb, cb_label=lab, cb_conf=conf, clip_conf=clip, labels=list(self._model.labels))

    def regress(self, model, out_min=None, out_max=None, stream=0):
        """K6 with the un-normalising epilogue on the rows of the last run, enqueued on `stream` (wsa_batch_regress); the range defaults
        to the model's own (spec.out_min / spec.out_max)."""
        lo, hi = model.out_range(out_min, out_max)
        self.an._check(self.L.wsa_batch_regress(self.h, model.h, lo, hi, stream))
        self._model = model

    def values(self, stream=0):
        """Host copy of the last regress: [n_rows] f64, one value per row in the order of rows()."""
        n = ctypes.c_uint32()
        self.an._check(self.L.wsa_batch_copy_values(self.h, stream, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, np.float64)
        self.an._check(self.L.wsa_batch_copy_values(self.h, stream, out.ctypes.data, max(n.value, 1), ctypes.byref(n)))
        return out

    def knn(self, store, k=10, stream=0):
        """K9 on the rows of the last run, enqueued on `stream` (wsa_batch_knn): levels 5 / 13 with a 53-wide store, level 11 with a
        264-wide one (the utterance rows), level 12 with a 23-wide one (label -1 and NaN for a row whose fit threw)."""
        self.an._check(self.L.wsa_batch_knn(self.h, store.h, int(k), stream))
        self._knn = store

    def knn_result(self, stream=0):
        r = _KnnResult()
        self.an._check(self.L.wsa_batch_knn_result(self.h, stream, ctypes.byref(r)))
        return r

    def knn_classes(self, stream=0):
        """Host copies of the last knn(): dict(label [n] i32, conf [n, C] f64, nbr [n, k] i32, sim [n, k] f32, k_eff), rows in the order of
        rows() (level 11: utterance())."""
        r = self.knn_result(stream)
        n, C, k = int(r.n_rows), int(r.n_classes), int(r.k)
        out = dict(label=np.zeros(n, np.int32), conf=np.zeros((n, C), np.float64), nbr=np.zeros((n, k), np.int32), sim=np.zeros((n, k), np.float32), k_eff=int(r.k_eff))
        self.an._check(self.L.wsa_batch_copy_knn(self.h, stream, out["label"].ctypes.data, out["conf"].ctypes.data, out["nbr"].ctypes.data, out["sim"].ctypes.data, max(n, 1)))
        return out

    def knn_fold(self, stream=0):
        """KN-2 on the tables of the last knn() at level 13, enqueued on `stream` (wsa_batch_knn_fold): K6b's fold fed the rows' KNN
        confidences with the class indices as the legend, one accumulator per clip."""
        self.an._check(self.L.wsa_batch_knn_fold(self.h, stream))

    def knn_fold_classes(self, stream=0):
        """Host copies of the last knn_fold(): dict(cb [n_cb, 4] i32 = {clip, si, first row, rows}, cb_label [n_cb] i32 (a class index;
        -1: null, -2: not predicted), cb_conf [n_cb] f64, clip_conf [n_clips, C] f64)."""
        r = _KnnFoldResult()
        self.an._check(self.L.wsa_batch_knn_fold_result(self.h, stream, ctypes.byref(r)))
        k, C = int(r.n_callbacks), int(r.n_classes)
        out = dict(cb=np.zeros((k, 4), np.int32), cb_label=np.zeros(k, np.int32), cb_conf=np.zeros(k, np.float64), clip_conf=np.zeros((int(r.n_clips), C), np.float64))
        self.an._check(self.L.wsa_batch_copy_knn_fold(self.h, stream, out["cb"].ctypes.data, out["cb_label"].ctypes.data, out["cb_conf"].ctypes.data, max(k, 1),
                                                       out["clip_conf"].ctypes.data))
        return out

    def regress_group(self, group, stream=0):
        """The grouped K6 over a RegressGroup's heads on the rows of the last run and, at level 13, the fold RG-1, enqueued on `stream`
        (wsa_batch_regress_group); levels 5 and 13."""
        self.an._check(self.L.wsa_batch_regress_group(self.h, group.h, stream))
        self._group = group

    def value_result(self, stream=0):
        r = _ValueResult()
        self.an._check(self.L.wsa_batch_value_result(self.h, stream, ctypes.byref(r)))
        return r

    def value_fold(self, stream=0):
        """Host copies of the last regress_group(): dict(value [H, n_rows] f64; at level 13 also cb [n_cb, 4] i32 = {clip, si, first row,
        rows}, cb_value / cb_weight [H, n_cb] f64 (NaN / 0: a skipped callback), clip_sum / clip_weight / clip_value [H, n_clips] f64)."""
        r = self.value_result(stream)
        H, n, k, nc = int(r.n_heads), int(r.n_rows), int(r.n_callbacks), int(r.n_clips)
        out = dict(value=np.zeros((H, n), np.float64))
        if r.d_cb:
            out.update(cb=np.zeros((k, 4), np.int32), cb_value=np.zeros((H, k)), cb_weight=np.zeros((H, k)),
                       clip_sum=np.zeros((H, nc)), clip_weight=np.zeros((H, nc)), clip_value=np.zeros((H, nc)))
        h = _ValueHost()
        h.rows_cap, h.cb_cap = max(n, 1), max(k, 1)
        for name, v in out.items():
            if name == "cb":
                h.cb = v.ctypes.data
            else:
                for d in range(H):
                    getattr(h, name)[d] = v[d].ctypes.data
        self.an._check(self.L.wsa_batch_copy_value_fold(self.h, stream, ctypes.byref(h)))
        return out

    def classify_ensemble(self, ensemble, stream=0):
        """K6e (+ K6b-e and the cross-DB decision at level 13) on the rows of the last run, enqueued on `stream` (wsa_batch_classify_ensemble)."""
        self.an._check(self.L.wsa_batch_classify_ensemble(self.h, ensemble.h, stream))
        self._ensemble = ensemble

    def ensemble_result(self, stream=0):
        r = _EnsembleResult()
        self.an._check(self.L.wsa_batch_ensemble_result(self.h, stream, ctypes.byref(r)))
        return r

    def ensemble_classes(self, stream=0):
        """Host copies of the last ensemble classification.  Per member (lists of n_members arrays): prob [n_rows, C_d] f32, cb_label /
        cb_conf / cb_all_max [n_cb], clip_conf [n_clips, C_d].  Across members: cb [n_cb, 4], cb_db (-1: null, -2: not predicted),
        cb_top_label, cb_top_conf, cb_min_db, cb_entropy [n_cb], clip_min_db [n_clips]; labels = the members' legends.  Level 5: prob only."""
        r = self.ensemble_result(stream)
        nm, n, k, nc = int(r.n_members), int(r.n_rows), int(r.n_callbacks), int(r.n_clips)
        fold = bool(r.d_cb)
        C = [int(r.n_classes[d]) for d in range(nm)]
        out = dict(prob=[np.zeros((n, c), np.float32) for c in C], labels=[list(m.labels) for m in self._ensemble.models])
        h = _EnsembleHost()
        h.rows_cap, h.cb_cap = max(n, 1), max(k, 1)
        if fold:
            for name, dt in (("cb_label", np.int32), ("cb_conf", np.float64), ("cb_all_max", np.float64)):
                out[name] = [np.zeros(k, dt) for _ in C]
            out["clip_conf"] = [np.zeros((nc, c), np.float64) for c in C]
            out.update(cb=np.zeros((k, 4), np.int32), cb_db=np.zeros(k, np.int32), cb_top_label=np.zeros(k, np.int32), cb_top_conf=np.zeros(k),
                       cb_min_db=np.zeros(k, np.int32), cb_entropy=np.zeros(k), clip_min_db=np.zeros(nc, np.int32))
        for name, v in out.items():
            if name == "labels":
                continue
            if isinstance(v, list):
                for d in range(nm):
                    getattr(h, name)[d] = v[d].ctypes.data
            else:
                setattr(h, name, v.ctypes.data)
        self.an._check(self.L.wsa_batch_copy_ensemble(self.h, stream, ctypes.byref(h)))
        return out
