"""Test access: the wsa_debug_* entries of the library (not part of include/wsa.h) on hand-built tables."""
import ctypes

import numpy as np

from ._abi import NFEAT, P, WsaError, dbl, i32, lib, st, u32, u64, vp

# name: (restype, argtypes) of the test entries, the ones tests and probes call without a wrapper included; lib() declares them at load
DEBUG_TABLE = {
    "wsa_debug_batch_keep_counters": (st, [vp, i32]),                 # Batch.keep_counters
    "wsa_debug_batch_tiers": (st, [vp, vp, vp]),                      # Batch.tiers
    "wsa_debug_regress_fold": (st, [i32, vp, vp, u32, u32, dbl, u32, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]),
    "wsa_debug_featdb_append": (st, [vp, i32, vp, vp, u32, vp, u32, u32, vp, P(u32), P(u32), vp, u32]),
    "wsa_debug_featdb_copy_capacity": (st, [vp, vp]),
    "wsa_debug_stream_featdb_step": (st, [vp, i32, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, u32]),
    "wsa_debug_class_fold": (st, [i32, vp]),
    "wsa_debug_classify": (st, [vp]),
    "wsa_debug_knn_split": (st, [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp]),
    "wsa_debug_gate": (st, [i32, i32, vp, vp, u32, i32, vp, u32, u32, u32, u32, vp, vp, vp] + [vp] * 9),
    "wsa_debug_peaks": (st, [i32, vp, u32, i32, i32, vp, vp, vp, vp]),
    "wsa_debug_resample": (st, [i32, vp, u32, u64, u32, u32, vp, vp, dbl, i32, i32, i32, i32, vp, u64, vp, vp, u32, vp]),
    "wsa_debug_fe_choice": (st, [vp, dbl, ctypes.c_char_p, u32]),
    "wsa_debug_stream_spectra": (st, [vp, vp, u64]),
    "wsa_debug_stream_ctl": (st, [vp, vp, u64]),
    "wsa_debug_stream_step_backend": (st, [vp, vp, vp, vp, u32, vp]),
    "wsa_debug_compact": (st, [i32, vp]),
    "wsa_debug_span_order": (st, [i32, i32, vp, vp, u32, i32, vp, u32, vp] + [vp] * 6),
    # called by tests and probes directly
    "wsa_debug_jsmath": (st, [i32, i32, vp, vp, vp, u32]),
    "wsa_debug_floor_law": (st, [i32, u64, u64, vp]),
    "wsa_debug_score": (st, [i32, vp, vp, u32]),
    "wsa_debug_features": (st, [i32, vp, u32, dbl, i32, vp]),
    "wsa_debug_coeffs": (st, [i32, vp, vp, vp, u32, vp, u32, u32, u32, u32, dbl, vp]),
    "wsa_debug_utterance": (st, [i32, vp, u32, vp, vp, u32, vp, vp, vp, u32, u32, u32, vp, vp, vp, i32, vp, vp, vp, vp]),
    "wsa_debug_batch_unpack": (st, [i32] + [vp] * 5 + [u32, vp, u64]),
    "wsa_debug_batch_deinterleave": (st, [i32, vp, u64] + [vp] * 5 + [u32, vp, vp, u64, ctypes.c_char_p, u32]),
    "wsa_debug_peaks_time": (st, [i32, vp, u32, i32, i32, i32, i32, vp]),
}

GATE_INT_RUNS, GATE_INT_GENERAL, GATE_F64, GATE_STREAM = 0, 1, 2, 3
GATE_STATE_WORDS = 16
GATE_SENTINEL = -2


def debug_regress_fold(meta, values, step_s, row_off, ctl=None, device=0, sentinel=-7.0):
    """Test access to the fold RG-1 on its own (csrc/debug_fold.hip wsa_debug_regress_fold; not part of include/wsa.h): hand-built row meta
    [n_rows, 8] i32 and value columns [H, n_rows] f64.  ctl None: a batch, row_off [n + 1]; else streams, row_off [n_steps, n + 1] counting
    from each step's first row and ctl [n_steps, n] control bytes.  Returns dict(n_cb (int, or [n_steps]), cb [K, 4], cb_value / cb_weight
    [H, K] over all K callbacks (the steps' one after the other), run_sum / run_weight / run_value [H, n] (streams: [n_steps, H, n]))."""
    L = lib()
    meta = np.ascontiguousarray(meta, np.int32).reshape(-1, 8)
    values = np.ascontiguousarray(values, np.float64)
    H, n_rows = values.shape
    assert n_rows == len(meta)
    row_off = np.ascontiguousarray(row_off, np.uint32)
    streams = ctl is not None
    n_steps = row_off.shape[0] if streams else 0
    n = row_off.shape[-1] - 1
    ctl_a = np.ascontiguousarray(ctl, np.uint8) if streams else None
    K = max(n_rows, 1)
    tables = max(n_steps, 1)
    n_cb = np.zeros(tables, np.uint32)
    cb = np.full((K, 4), int(sentinel), np.int32)
    cbv, cbw = np.full((H, K), sentinel), np.full((H, K), sentinel)
    run = [np.full((tables, H, n), sentinel) for _ in range(3)]
    rc = L.wsa_debug_regress_fold(device, meta.ctypes.data, values.ctypes.data, n_rows, H, float(step_s), n, n_steps, row_off.ctypes.data,
                                  ctl_a.ctypes.data if streams else None, K, n_cb.ctypes.data, cb.ctypes.data, cbv.ctypes.data, cbw.ctypes.data,
                                  run[0].ctypes.data, run[1].ctypes.data, run[2].ctypes.data)
    if rc != 0:
        raise WsaError(f"wsa_debug_regress_fold: status {rc}")
    k = int(n_cb.sum())
    sel = (lambda a: a) if streams else (lambda a: a[0])
    return dict(n_cb=n_cb if streams else int(n_cb[0]), cb=cb[:k], cb_value=cbv[:, :k], cb_weight=cbw[:, :k],
                run_sum=sel(run[0]), run_weight=sel(run[1]), run_value=sel(run[2]))


def debug_featdb_append(db, level, meta, feat, clip_off=None, stream=0):
    """Test access to K10 on hand-built tables (csrc/featdb.hip wsa_debug_featdb_append; not part of include/wsa.h): meta [n][8] i32
    (None at levels 5 / 13 / 11), feat [n][stride] f64, clip_off [n_clips + 1] u32 (level 11).  The tables are uploaded with torch, the
    product's keep, scan and copy kernels run over them.  Returns (first DB row, kept)."""
    import torch
    L = lib()
    dev = f"cuda:{db.an.device}"
    feat = np.ascontiguousarray(feat, np.float64)
    n, stride = feat.shape
    t_feat = torch.from_numpy(feat.view(np.int64)).to(dev)
    t_meta = None if meta is None else torch.from_numpy(np.ascontiguousarray(meta, np.int32).reshape(n, 8)).to(dev)
    off = None if clip_off is None else np.ascontiguousarray(clip_off, np.uint32)
    t_off = None if off is None else torch.from_numpy(off.view(np.int32)).to(dev)
    n_clips = 0 if off is None else len(off) - 1
    items = n_clips if level == 11 else n
    kept = np.zeros(max(items, 1), np.int32)
    first, added = u32(), u32()
    torch.cuda.synchronize(dev)
    db.an._check(L.wsa_debug_featdb_append(db.h, int(level), None if t_meta is None else t_meta.data_ptr(), t_feat.data_ptr() if n else None, stride,
                                           None if t_off is None else t_off.data_ptr(), n, n_clips, stream, ctypes.byref(first), ctypes.byref(added),
                                           kept.ctypes.data, len(kept)))
    torch.cuda.synchronize(dev)
    return int(first.value), kept[:added.value].copy()


def debug_featdb_copy_capacity(db):
    """Test access (csrc/stream_featdb.hip wsa_debug_featdb_copy_capacity; not part of include/wsa.h): the DB's whole table
    [capacity][width], the rows beyond its count included."""
    L = lib()
    out = np.zeros((db.capacity, db.width), np.float64)
    db.an._check(L.wsa_debug_featdb_copy_capacity(db.h, out.ctypes.data))
    return out


def debug_stream_featdb_step(db, level, meta, feat, n_rows=None, flags=0, utt_off=None, bits=None, slot=None, rows_cap=None, stream=0):
    """Test access to the stream step's DB kernels on hand-built tables (csrc/debug.hip wsa_debug_stream_featdb_step; not part of
    include/wsa.h): meta [n][8] i32 (level 12; else None), feat [n][stride] f64, n_rows = the step's row-count word (None: n), flags = its
    flags word, and at level 11 utt_off [n_streams + 1] u32, bits [n_streams] u32 (bit 0: START) and slot [n_streams] i32.  The tables are
    uploaded with torch; the plan and the copy kernel run once.  Returns dict(first_row, n_added, n_replaced, not_fitted, kept, replaced,
    slot = the slot table afterwards)."""
    import torch
    L = lib()
    dev = f"cuda:{db.an.device}"
    feat = np.ascontiguousarray(feat, np.float64)
    n, stride = feat.shape
    up = lambda a: torch.from_numpy(a).to(dev)
    t_feat = up(feat.view(np.int64)) if n else None
    t_meta = None if meta is None or not n else up(np.ascontiguousarray(meta, np.int32).reshape(n, 8))
    t_words = up(np.array([n if n_rows is None else n_rows, flags], np.uint32).view(np.int32))
    n_streams, t_off, t_bits, t_slot = 0, None, None, None
    if utt_off is not None:
        off = np.ascontiguousarray(utt_off, np.uint32)
        n_streams = len(off) - 1
        t_off = up(off.view(np.int32))
        t_bits = up(np.ascontiguousarray(bits, np.uint32).view(np.int32))
        t_slot = up(np.ascontiguousarray(slot, np.int32).copy())
    kept = np.zeros(max(n, n_streams, 1), np.int32)
    rep = np.zeros((max(n_streams, 1), 2), np.int32)
    out4 = np.zeros(4, np.uint32)
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize(dev)
    db.an._check(L.wsa_debug_stream_featdb_step(db.h, int(level), ptr(t_meta), ptr(t_feat), stride, n if rows_cap is None else int(rows_cap), ptr(t_off), n_streams,
                                                t_words.data_ptr(), t_words.data_ptr() + 4, ptr(t_bits), ptr(t_slot), stream, out4.ctypes.data,
                                                kept.ctypes.data, len(kept), rep.ctypes.data, len(rep)))
    torch.cuda.synchronize(dev)
    return dict(first_row=int(out4[0]), n_added=int(out4[1]), n_replaced=int(out4[2]), not_fitted=int(out4[3]), kept=kept[:out4[1]].copy(),
                replaced=rep[:out4[2]].copy() if utt_off is not None else None, slot=None if t_slot is None else t_slot.cpu().numpy())


class _DebugFoldIO(ctypes.Structure):
    """struct wsa_debug_fold_io of csrc/debug_fold.hip"""
    _M = 8                                            # WSA_ENSEMBLE_MAX
    _vp, _u32, _i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    _fields_ = [("meta", _vp), ("row_off", _vp), ("ctl", _vp), ("step_s", ctypes.c_double),
                ("n_rows", _u32), ("n", _u32), ("n_steps", _u32), ("cap", _u32), ("n_members", _u32), ("cb_cap", _u32), ("single", _i32), ("f64", _i32),
                ("C", _u32 * _M), ("legend", _vp * _M), ("conf", _vp * _M),
                ("n_cb", _vp), ("cb", _vp),
                ("cb_label", _vp * _M), ("cb_conf", _vp * _M), ("cb_all_max", _vp * _M), ("run_conf", _vp * _M),
                ("cb_db", _vp), ("cb_top_label", _vp), ("cb_top_conf", _vp), ("cb_min_db", _vp), ("cb_entropy", _vp), ("run_min_db", _vp),
                ("h_cb", _vp), ("h_cb_label", _vp * _M), ("h_cb_conf", _vp * _M), ("h_cb_all_max", _vp * _M),
                ("h_cb_db", _vp), ("h_cb_top_label", _vp), ("h_cb_top_conf", _vp), ("h_cb_min_db", _vp), ("h_cb_entropy", _vp)]


def debug_class_fold(meta, row_off, step_s, legends, conf, single=False, f64=False, ctl=None, cap=0, cb_cap=None, device=0, sentinel=-7):
    """Test access to the class fold K6b / K6b-e on its own (csrc/debug_fold.hip wsa_debug_class_fold; not part of include/wsa.h): hand-built row
    meta [n_rows, 8] i32, per member a legend (strings) and confidences conf[d] [n_rows, C_d] (sent as float32, or float64 with f64).
    single: the one-model kernels (one member), else the group's.  ctl None: a batch, row_off [n + 1]; else streams, row_off
    [n_steps, n + 1] counting from each step's first row, ctl [n_steps, n] control bytes and the D2H window `cap`.
    Every output table starts as `sentinel` and comes back whole.  Returns a dict: n_cb (int, or [n_steps]); cb [K, 4]; cb_label / cb_conf /
    cb_all_max [M][K]; run_conf [M] of [n, C_d] (streams: [n_steps, n, C_d]); cb_db, cb_top_label, cb_top_conf, cb_min_db, cb_entropy [K];
    run_min_db [n] (streams: [n_steps, n]); streams also h_* [n_steps, max(cap, 1)] like the cb_* tables."""
    L = lib()
    meta = np.ascontiguousarray(meta, np.int32).reshape(-1, 8)
    n_rows, M = len(meta), len(legends)
    row_off = np.ascontiguousarray(row_off, np.uint32)
    streams = ctl is not None
    n_steps = row_off.shape[0] if streams else 0
    n = row_off.shape[-1] - 1
    ctl_a = np.ascontiguousarray(ctl, np.uint8) if streams else None
    K = int(cb_cap) if cb_cap is not None else 2 * max(n_rows, 1) + 3          # room beyond the callbacks: the sentinel must survive there
    tables, W = max(n_steps, 1), max(int(cap), 1)
    confs = [np.ascontiguousarray(c, np.float64 if f64 else np.float32).reshape(n_rows, len(leg)) for c, leg in zip(conf, legends)]
    io = _DebugFoldIO()
    keep = [meta, row_off, ctl_a, confs]
    io.meta, io.row_off, io.ctl, io.step_s = meta.ctypes.data, row_off.ctypes.data, ctl_a.ctypes.data if streams else None, float(step_s)
    io.n_rows, io.n, io.n_steps, io.cap, io.n_members, io.cb_cap, io.single, io.f64 = n_rows, n, n_steps, int(cap), M, K, int(bool(single)), int(bool(f64))
    sent_i = lambda *shape: np.full(shape, int(sentinel), np.int32)
    sent_d = lambda *shape: np.full(shape, float(sentinel), np.float64)
    out = dict(n_cb=np.zeros(tables, np.uint32), cb=sent_i(K, 4), cb_label=[sent_i(K) for _ in range(M)], cb_conf=[sent_d(K) for _ in range(M)],
               cb_all_max=[sent_d(K) for _ in range(M)], run_conf=[sent_d(tables, n, len(leg)) for leg in legends],
               cb_db=sent_i(K), cb_top_label=sent_i(K), cb_top_conf=sent_d(K), cb_min_db=sent_i(K), cb_entropy=sent_d(K), run_min_db=sent_i(tables, n),
               h_cb=sent_i(n_steps, W, 4), h_cb_label=[sent_i(n_steps, W) for _ in range(M)], h_cb_conf=[sent_d(n_steps, W) for _ in range(M)],
               h_cb_all_max=[sent_d(n_steps, W) for _ in range(M)], h_cb_db=sent_i(n_steps, W), h_cb_top_label=sent_i(n_steps, W),
               h_cb_top_conf=sent_d(n_steps, W), h_cb_min_db=sent_i(n_steps, W), h_cb_entropy=sent_d(n_steps, W))
    for d in range(min(M, _DebugFoldIO._M)):          # (more members than the struct holds: n_members says so, the entry refuses)
        strs = [str(s).encode() for s in legends[d]]
        arr = (ctypes.c_char_p * len(strs))(*strs)
        keep += [strs, arr]
        io.C[d], io.legend[d], io.conf[d] = len(strs), ctypes.cast(arr, ctypes.c_void_p).value, confs[d].ctypes.data
    for name, v in out.items():
        if isinstance(v, list):
            for d in range(min(M, _DebugFoldIO._M)):
                getattr(io, name)[d] = v[d].ctypes.data
        else:
            setattr(io, name, v.ctypes.data)
    rc = L.wsa_debug_class_fold(device, ctypes.addressof(io))
    if rc != 0:
        raise WsaError(f"wsa_debug_class_fold: status {rc}")
    del keep
    if not streams:
        out["n_cb"] = int(out["n_cb"][0])
        out["run_conf"] = [r[0] for r in out["run_conf"]]
        out["run_min_db"] = out["run_min_db"][0]
    return out


class _DebugClassifyIO(ctypes.Structure):
    """struct wsa_debug_classify_io of csrc/debug_classify.hip"""
    _vp, _u32, _i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    _fields_ = [("models", _vp), ("n_models", _u32), ("feat", _vp), ("feat_rows", _u32), ("stride", _u32), ("nan_slot", _i32),
                ("n_rows", _u32), ("rows_cap", _u32), ("n_dev", _i32), ("rb", _i32), ("one_block", _i32), ("regress", _i32),
                ("out_min", ctypes.c_double), ("out_max", ctypes.c_double), ("out", _vp * 8), ("out_rows", _u32)]


DEBUG_CLASSIFY_SEED_F32, DEBUG_CLASSIFY_SEED_F64 = 0xffc0beef, 0xfff8beef0000beef      # NaNs no kernel writes: K6's own NaN is the positive quiet one


def debug_classify(models, feat, n_rows=None, n_dev=None, rows_cap=None, rb=0, one_block=False, nan_slot=-1, out_range=None, out_rows=None):
    """Test access to K6 / K6e through the product's own launches (csrc/debug_classify.hip wsa_debug_classify; not part of include/wsa.h): one Model, or a
    list of 2 .. 8 as a group, over host rows feat [rows, stride] f64 (stride >= the models' inputs; nan_slot as level 12's `threw` mark).
    n_dev: the row count on the device (n_rows: the launch's own, one model only; default every row of feat); rows_cap sizes the grid (default the
    count, at least 1); rb 0 / 1 / 2 / 4 overrides the row-block factor; one_block runs a group's members with one row block each;
    out_range (out_min, out_max): the regression epilogue.  Every output table has out_rows rows (default the count + 3), starts as the seed
    pattern and comes back whole: a uint32 view [out_rows, C] per model, or uint64 [out_rows] for a regression; a list for a group."""
    L = lib()
    group = isinstance(models, (list, tuple))
    ms = list(models) if group else [models]
    feat = np.ascontiguousarray(feat, np.float64)
    assert feat.ndim == 2
    count = int(n_dev) if n_dev is not None else (int(n_rows) if n_rows is not None else len(feat))
    cap = int(rows_cap) if rows_cap is not None else max(count, 1)
    R = int(out_rows) if out_rows is not None else count + 3
    if len(feat) == 0:
        feat = np.zeros((1, feat.shape[1]), np.float64)
    io = _DebugClassifyIO()
    handles = (ctypes.c_void_p * len(ms))(*[m.h for m in ms])
    io.models, io.n_models = ctypes.cast(handles, ctypes.c_void_p), len(ms)
    io.feat, io.feat_rows, io.stride, io.nan_slot = feat.ctypes.data, feat.shape[0], feat.shape[1], int(nan_slot)
    io.n_rows, io.rows_cap, io.n_dev, io.rb, io.one_block = count, cap, -1 if n_dev is None else int(n_dev), int(rb), int(bool(one_block))
    io.regress = int(out_range is not None)
    io.out_min, io.out_max = (float(out_range[0]), float(out_range[1])) if out_range is not None else (0.0, 0.0)
    if out_range is not None:
        outs = [np.full(R, DEBUG_CLASSIFY_SEED_F64, np.uint64) for _ in ms]
    else:
        outs = [np.full((R, m.n_classes), DEBUG_CLASSIFY_SEED_F32, np.uint32) for m in ms]
    for d, o in enumerate(outs[:8]):
        io.out[d] = o.ctypes.data
    io.out_rows = R
    rc = L.wsa_debug_classify(ctypes.addressof(io))
    if rc != 0:
        raise WsaError(f"wsa_debug_classify: status {rc}")
    return outs if group else outs[0]


def debug_knn_split(store, d_feat, n_rows, k, slices, d_label, d_conf, d_nbr, d_sim, stream=0):
    """Test access to K9s on its own (csrc/knn.hip wsa_debug_knn_split; not part of include/wsa.h): the split-store kernels over n_rows dense
    device rows with a forced slice count (0: the rule's), outputs as KnnStore.classify_rows.  Only enqueues (its scratch table stays with
    the store); with n_rows = 0 the kernels still run, over no row."""
    L = lib()
    store.an._check(L.wsa_debug_knn_split(store.h, d_feat, int(n_rows), int(k), int(slices), d_label, d_conf, d_nbr, d_sim, stream))


def debug_gate(variant, clips, settings, blocks=0, F=0, max_span=0, step_nfr=None, step_ctl=None, device=0):
    """Test access to the gate on its own (csrc/debug_gate.hip wsa_debug_gate; not part of include/wsa.h): clips = [frames_c, bands] u32 arrays, settings =
    the six gate settings by name, variant = GATE_*.  Streams (GATE_STREAM): step_nfr / step_ctl [n_steps, n_clips].  Returns the gate's outputs as the
    kernel left them: fr_info / fr_v / fr_fl (fr_span) per clip, seg_i [.., seg_cap, 8], seg_d [.., seg_cap, 2], seg_count, flags, counter0, seg_cap (ring,
    state per step); frames no step fed keep GATE_SENTINEL.  Raises WsaError on a refusal."""
    L = lib()
    n = len(clips)
    bands = int(clips[0].shape[1])
    nfr = np.array([len(c) for c in clips], np.uint32)
    total = int(nfr.sum())
    spec = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint32).reshape(-1, bands) for c in clips], axis=0)) if total else np.zeros((1, bands), np.uint32)
    s6 = np.array([settings["window_step"], settings["pause_length"], settings["min_seg_length"], float(bool(settings["auto_noise_gate"])),
                   settings["voiced_max_dB"], settings["voiced_min_dB"]], np.float64)
    streams = variant == GATE_STREAM
    n_steps = 0
    if streams:
        step_nfr = np.ascontiguousarray(step_nfr, np.uint32)
        step_ctl = np.ascontiguousarray(step_ctl, np.uint32)
        n_steps = step_nfr.shape[0]
        assert step_nfr.shape == (n_steps, n) and step_ctl.shape == (n_steps, n)
    ptr = lambda a: a.ctypes.data if a is not None else None
    caps = np.zeros(2, np.int32)

    def call(*outs):
        rc = L.wsa_debug_gate(device, variant, ptr(spec), ptr(nfr), n, bands, ptr(s6), blocks, F, max_span, n_steps, ptr(step_nfr) if streams else None,
                              ptr(step_ctl) if streams else None, ptr(caps), *outs)
        if rc != 0:
            raise WsaError(f"wsa_debug_gate: error {rc}")
    call(*([None] * 9))
    seg_cap, ring = int(caps[0]), int(caps[1])
    lead = (n_steps, n) if streams else (n,)
    fr_info = np.full(max(total, 1), GATE_SENTINEL, np.int32)
    fr_span = np.full(max(total, 1), GATE_SENTINEL, np.int32)
    fr_v = np.full(max(total, 1), float(GATE_SENTINEL))
    fr_fl = np.full(max(total, 1), float(GATE_SENTINEL))
    seg_i = np.full(lead + (seg_cap, 8), GATE_SENTINEL, np.int32)
    seg_d = np.full(lead + (seg_cap, 2), float(GATE_SENTINEL))
    seg_count = np.full(lead, 0xffffffff, np.uint32)
    flags2 = np.zeros(2, np.uint32)
    state = np.zeros((max(n_steps, 1), n, GATE_STATE_WORDS))
    call(ptr(fr_info), ptr(fr_v), ptr(fr_fl), ptr(fr_span), ptr(seg_i), ptr(seg_d), ptr(seg_count), ptr(flags2), ptr(state))
    off = np.concatenate([[0], np.cumsum(nfr)]).astype(np.int64)
    cut = lambda a: [a[off[i]:off[i + 1]] for i in range(n)]
    out = dict(fr_info=cut(fr_info), fr_v=cut(fr_v), fr_fl=cut(fr_fl), seg_i=seg_i, seg_d=seg_d, seg_count=seg_count, flags=int(flags2[0]), counter0=int(flags2[1]),
               seg_cap=seg_cap)
    if streams:
        out.update(fr_span=cut(fr_span), state=state, ring=ring)
    return out


PEAKS_LANES_16, PEAKS_LANES_32, PEAKS_WAVE = 3, 4, 2          # modes of wsa_debug_peaks: peaks_kernel<16>, peaks_kernel<32>, peaks_wave_kernel (at most 128 bands)
CAND_CAP = 64


def debug_peaks(spec, mode, device=0):
    """Test access to the peak scan on its own (csrc/debug_gate.hip wsa_debug_peaks; not part of include/wsa.h): spec = [n_frames, bands] u32, one launch of
    the kernel behind `mode` (PEAKS_*).  Returns the frame records as the kernel left them in zero-filled tables, decoded: g [n] (40 bits), n [n], largest
    amplitude and bin [n], table base [n]; per candidate slot [n, 64] i, s, l, last, amp and the 40-bit prefix sums p_i = P[i - 1] and p_s = P[s]; the flag word;
    and the raw words hdr [n, 4], amp, ent [n, 64, 4] for bitwise comparisons.  Raises WsaError on a refusal."""
    L = lib()
    spec = np.ascontiguousarray(spec, np.uint32)
    n, bands = spec.shape
    hdr = np.zeros((n, 4), np.uint32)
    amp = np.zeros((n, CAND_CAP), np.uint32)
    ent = np.zeros((n, CAND_CAP, 4), np.uint32)
    flags = np.zeros(1, np.uint32)
    rc = L.wsa_debug_peaks(device, spec.ctypes.data, n, bands, mode, hdr.ctypes.data, amp.ctypes.data, ent.ctypes.data, flags.ctypes.data)
    if rc != 0:
        raise WsaError(f"wsa_debug_peaks: error {rc}")
    h1, w, hi = hdr[:, 1].astype(np.uint64), ent[:, :, 0], ent[:, :, 3].astype(np.uint64)
    return dict(g=hdr[:, 0].astype(np.uint64) | ((h1 & np.uint64(0xff)) << np.uint64(32)), n=(hdr[:, 1] >> 8) & 0xff, largest_bin=(hdr[:, 1] >> 16) & 0xff,
                largest_amp=hdr[:, 2].copy(), base=hdr[:, 3].copy(), hdr_top=hdr[:, 1] >> 24,
                i=w & 0xff, s=(w >> 8) & 0xff, l=(w >> 16) & 0xff, last=w >> 24, amp=amp,
                p_i=ent[:, :, 1].astype(np.uint64) | ((hi & np.uint64(0xff)) << np.uint64(32)),
                p_s=ent[:, :, 2].astype(np.uint64) | (((hi >> np.uint64(8)) & np.uint64(0xff)) << np.uint64(32)), ent_top=ent[:, :, 3] >> 16,
                flags=int(flags[0]), hdr=hdr, ent=ent)


def debug_resample(clips, fs_in, fs_out, form=0, S=0, J=0, chunks=0, offset_bytes=0, stride_in=None, stride_out=None, pad_bits=0, sentinel=0x7fa5c3d1, device=0):
    """Test access to the batch rate converter K0 on its own (csrc/debug_input.hip wsa_debug_resample; not part of include/wsa.h), no front end behind it.
    clips = float32 arrays, fs_in one rate or one per clip.  form 0: resample_kernel (one rate; S, J, chunks override the launch shape as WSA_RS_S / _J / _C do),
    1: resample_mixed_kernel with one launch per rate class, 2: with one launch over the whole work list.  The device copy starts offset_bytes (0, 4, 8, 12)
    behind a 16-byte boundary; pad_bits is the bit pattern of everything around the clips' samples: behind each clip inside its row of stride_in samples, the
    whole row of an empty clip, the words in front of and behind the copy.  Returns out [n, stride_out] as the kernel left rows that started as the
    `sentinel` bit pattern, n_out [n], plan [classes, 6] = {S, J, span, block, lds bytes, copy} per rate class and the launch's block and lds.  Raises WsaError
    on a refusal (status 1: overrides that cannot launch)."""
    L = lib()
    n = len(clips)
    rates = np.ascontiguousarray(np.broadcast_to(np.asarray(fs_in, np.float64), (n,)))
    n_in = np.array([len(c) for c in clips], np.uint32)
    stride_in = int(stride_in or max(int(n_in.max()), 1))
    buf = np.full((n, stride_in), pad_bits, np.uint32)
    for i, c in enumerate(clips):
        buf[i, :len(c)] = np.ascontiguousarray(c, np.float32).view(np.uint32)
    longest = max(int(L.wsa_resample_length(int(k), float(r), float(fs_out))) for k, r in zip(n_in, rates))
    stride_out = int(stride_out or longest + 8)
    out = np.full((n, stride_out), sentinel, np.uint32)
    n_out = np.zeros(n, np.uint32)
    plan = np.zeros((max(n, 1), 6), np.int32)
    shape3 = np.zeros(3, np.uint32)
    rc = L.wsa_debug_resample(device, buf.ctypes.data, n, stride_in, offset_bytes, pad_bits, n_in.ctypes.data, rates.ctypes.data, float(fs_out), form, S, J, chunks,
                              out.ctypes.data, stride_out, n_out.ctypes.data, plan.ctypes.data, len(plan), shape3.ctypes.data)
    if rc != 0:
        raise WsaError(f"wsa_debug_resample: error {rc}")
    return dict(out=out.view(np.float32), n_out=n_out, plan=plan[:int(shape3[0])].copy(), block=int(shape3[1]), lds=int(shape3[2]))


def debug_fe_choice(analyzer, fs):
    """Test access (csrc/debug_units.hip wsa_debug_fe_choice; not part of include/wsa.h): the name of the K1 instantiation the analyzer's settings select at the
    sample rate fs, as profiles/frontend_split.md writes it, e.g. 'fe_kernel_r8<4,5,8,true,4,3>'.  Plans on the host; launches nothing."""
    L = lib()
    buf = ctypes.create_string_buffer(64)
    rc = L.wsa_debug_fe_choice(analyzer.h, float(fs), buf, 64)
    if rc != 0:
        raise WsaError(f"wsa_debug_fe_choice: error {rc}")
    return buf.value.decode()


def debug_stream_spectra(streams, bands):
    """Test access (csrc/debug.hip wsa_debug_stream_spectra): the u32 frames the front end wrote in the stream set's last step,
    [n_streams, frames_per_step, bands]; call behind collect()."""
    L = lib()
    out = np.zeros((streams.n, streams.frame_capacity, int(bands)), np.uint32)
    rc = L.wsa_debug_stream_spectra(streams.h, out.ctypes.data, out.size)
    if rc != 0:
        raise WsaError(f"wsa_debug_stream_spectra: error {rc}")
    return out


def debug_stream_ctl(streams):
    """Test access (csrc/debug.hip wsa_debug_stream_ctl; not part of include/wsa.h): the device control words of a plain stream set's last step,
    [3, n_streams] uint32 = nfr, off (samples), bits (1 START, 2 STOP, 4 active); call behind collect().  A mixed-rate set is refused."""
    L = lib()
    out = np.zeros((3, streams.n), np.uint32)
    rc = L.wsa_debug_stream_ctl(streams.h, out.ctypes.data, out.size)
    if rc != 0:
        raise WsaError(f"wsa_debug_stream_ctl: error {rc}" + (" (a mixed-rate set has no plain control words)" if streams.mixed else ""))
    return out


def debug_stream_step_backend(streams, n_frames, ctl, frames, stream=0, bands=None):
    """Test access (csrc/debug.hip wsa_debug_stream_step_backend; not part of include/wsa.h): one step of a plain stream set past the front end.  frames
    [n_streams, frames_per_step, bands] u32 (stream i's first n_frames[i] frames count), n_frames [n] u32 (0 .. frames_per_step), ctl [n] u8
    (ACTIVE / START / STOP); the product's own launches from the peak scan down follow, uncaptured; collect() afterwards as behind any step.  A set is
    stepped through this entry only, or never through it.  bands: the band count handed down (default: frames' last axis); None arguments go down as
    null pointers (the refusals)."""
    L = lib()
    nfr = None if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.uint32)
    cb = None if ctl is None else np.ascontiguousarray(ctl, dtype=np.uint8)
    fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.uint32)
    if fr is not None and bands is None:
        if fr.shape[:2] != (streams.n, streams.frame_capacity):
            raise WsaError(f"frames of shape {fr.shape}: [n_streams, frames_per_step, bands] = [{streams.n}, {streams.frame_capacity}, bands] wanted")
        bands = fr.shape[2]
    if (nfr is not None and nfr.shape != (streams.n,)) or (cb is not None and cb.shape != (streams.n,)):
        raise WsaError("n_frames and ctl hold one entry per stream")
    ptr = lambda a: None if a is None else a.ctypes.data
    streams.an._check(L.wsa_debug_stream_step_backend(streams.h, ptr(nfr), ptr(cb), ptr(fr), int(bands or 0), stream))


COMPACT_FUSED, COMPACT_SCAN, COMPACT_COUNT_SCAN = 0, 1, 2     # compact_path of csrc/tracker.hip: what launch_compact ran
CARRY_HIST = 32
CARRY_WORDS = 2 + 2 * CARRY_HIST
SPAN_BUCKETS = 2048
COMPACT_SENTINEL = -7


class _DebugCompactIO(ctypes.Structure):
    """struct wsa_debug_compact_io of csrc/debug_rows.hip"""
    _vp, _u32, _i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    _fields_ = [("seg_i", _vp), ("seg_count", _vp), ("ctl", _vp), ("row_meta_in", _vp), ("row_feat_in", _vp), ("clip_rows", _vp), ("carry_in", _vp),
                ("n", _u32), ("seg_cap", _u32), ("pool", _u32), ("n_steps", _u32), ("rows_cap", _u32), ("segs_cap", _u32),
                ("level", _i32), ("fused", _i32), ("give_clr", _i32), ("give_host", _i32),
                ("seg_out", _vp), ("row_meta_out", _vp), ("row_feat_out", _vp), ("clip_row_off", _vp), ("clip_seg_off", _vp), ("totals", _vp),
                ("host4", _vp), ("counters", _vp), ("hist", _vp), ("path", _vp), ("carry", _vp)]


def debug_compact(seg_i, seg_count, row_meta_in, row_feat_in, level, fused=True, clip_rows=None, ctl=None, carry_in=None, counters=None, totals=None, hist=None,
                  give_clr=False, give_host=False, rows_cap=None, segs_cap=None, pool=None, device=0, sentinel=COMPACT_SENTINEL):
    """Test access to K3 on its own (csrc/debug_rows.hip wsa_debug_compact; not part of include/wsa.h).  Batch (ctl None): seg_i [n, seg_cap, 8] i32, seg_count [n],
    clip_rows [n] or None; streams: seg_i [n_steps, n, seg_cap, 8], seg_count / ctl [n_steps, n], carry_in [n, CARRY_WORDS] or None.  row_meta_in [pool, 8] i32,
    row_feat_in [pool, 53] (float64, or uint64 bit patterns).  counters [16] / totals [4] / hist [SPAN_BUCKETS]: the seeds (default: `sentinel` as u32, totals[2] = 0).
    Every output slot starts as `sentinel` (feature words: the u64 pattern of the sentinel repeated).  Returns dict(seg_out [.., segs_cap, 4], row_meta_out
    [.., rows_cap, 8], row_feat_out [.., rows_cap, 53] u64, clip_row_off / clip_seg_off [.., n + 1], totals [.., 4], host4, counters, hist, path (int, or
    [n_steps]), carry [n_steps, n, CARRY_WORDS]); `..` = n_steps for streams.  Raises WsaError on a refusal."""
    L = lib()
    streams = ctl is not None
    seg_i = np.ascontiguousarray(seg_i, np.int32)
    seg_count = np.ascontiguousarray(seg_count, np.uint32)
    n_steps = seg_i.shape[0] if streams else 0
    n, seg_cap = seg_i.shape[-3], seg_i.shape[-2]
    lead = (n_steps,) if streams else (1,)
    assert seg_i.shape == (lead if streams else ()) + (n, seg_cap, 8) and seg_count.shape == (lead if streams else ()) + (n,)
    meta_in = np.ascontiguousarray(row_meta_in, np.int32).reshape(-1, 8)
    feat_in = np.ascontiguousarray(row_feat_in)
    assert feat_in.dtype in (np.float64, np.uint64)
    feat_in = feat_in.reshape(-1, NFEAT)
    npool = len(meta_in) if pool is None else int(pool)
    su = np.uint32(sentinel & 0xffffffff)
    R = int(rows_cap) if rows_cap is not None else max(1, int(max(seg_i.reshape(lead[0], -1, 8)[k, :, 6].clip(0).sum() for k in range(lead[0])))) + 5
    S = int(segs_cap) if segs_cap is not None else int(seg_count.reshape(lead[0], -1).sum(axis=1).max()) + 3
    u64s = np.uint64((int(su) << 32) | int(su))
    out = dict(seg_out=np.full(lead + (S, 4), sentinel, np.int32), row_meta_out=np.full(lead + (R, 8), sentinel, np.int32), row_feat_out=np.full(lead + (R, NFEAT), u64s, np.uint64),
               clip_row_off=np.full(lead + (n + 1,), su, np.uint32), clip_seg_off=np.full(lead + (n + 1,), su, np.uint32),
               totals=np.tile(np.array([su, su, 0, su], np.uint32) if totals is None else np.ascontiguousarray(totals, np.uint32), lead + (1,)),
               host4=np.full(4, su, np.uint32), counters=np.full(16, su, np.uint32) if counters is None else np.array(counters, np.uint32),
               hist=np.full(SPAN_BUCKETS, su, np.uint32) if hist is None else np.array(hist, np.uint32), path=np.full(lead, -9, np.int32),
               carry=np.full((n_steps, n, CARRY_WORDS), sentinel, np.int32))
    assert out["counters"].shape == (16,) and out["hist"].shape == (SPAN_BUCKETS,) and out["totals"].shape == lead + (4,)
    ctl_a = np.ascontiguousarray(ctl, np.uint32) if streams else None
    rows_a = np.ascontiguousarray(clip_rows, np.uint32) if clip_rows is not None else None
    carry_a = np.ascontiguousarray(carry_in, np.int32) if carry_in is not None else None
    io = _DebugCompactIO()
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    io.seg_i, io.seg_count, io.ctl, io.row_meta_in, io.row_feat_in, io.clip_rows, io.carry_in = seg_i.ctypes.data, seg_count.ctypes.data, ptr(ctl_a), ptr(meta_in), ptr(feat_in), ptr(rows_a), ptr(carry_a)
    io.n, io.seg_cap, io.pool, io.n_steps, io.rows_cap, io.segs_cap = n, seg_cap, npool, n_steps, R, S
    io.level, io.fused, io.give_clr, io.give_host = int(level), int(bool(fused)), int(bool(give_clr)), int(bool(give_host))
    for name, v in out.items():
        setattr(io, name, v.ctypes.data if (name != "carry" or streams) else None)
    rc = L.wsa_debug_compact(device, ctypes.addressof(io))
    if rc != 0:
        e = WsaError(f"wsa_debug_compact: status {rc}")
        e.out = out                                      # a refusal writes nothing: the tests look at the sentinels
        raise e
    if not streams:
        for k in ("seg_out", "row_meta_out", "row_feat_out", "clip_row_off", "clip_seg_off", "totals"):
            out[k] = out[k][0]
        out["path"] = int(out["path"][0])
        del out["carry"]
    return out


def debug_span_order(variant, clips, settings, blocks=0, device=0, sentinel=0xfffffff9, seg_cap=None):
    """Test access to the span order on its own (csrc/debug_gate.hip wsa_debug_span_order; not part of include/wsa.h): clips / settings / variant / blocks as
    debug_gate's batch form; the gate counts the spans into hist / key as the batch driver has it, launch_span_order sorts.  Returns dict(seg_i [n, seg_cap, 8],
    seg_count [n], hist [SPAN_BUCKETS], key [n, seg_cap, 2] = {bucket, rank}, order [n * seg_cap, 2] = {clip, segment}, counters [4], seg_cap); key and order
    slots nobody wrote keep `sentinel`.  seg_cap: skip the sizing call and hand this number over.  A WsaError raised by the run carries the untouched tables as .out."""
    L = lib()
    n = len(clips)
    bands = int(clips[0].shape[1])
    nfr = np.array([len(c) for c in clips], np.uint32)
    total = int(nfr.sum())
    spec = np.ascontiguousarray(np.concatenate([np.asarray(c, np.uint32).reshape(-1, bands) for c in clips], axis=0)) if total else np.zeros((1, bands), np.uint32)
    s6 = np.array([settings["window_step"], settings["pause_length"], settings["min_seg_length"], float(bool(settings["auto_noise_gate"])),
                   settings["voiced_max_dB"], settings["voiced_min_dB"]], np.float64)
    caps = np.zeros(2, np.int32)

    def call(*outs):
        rc = L.wsa_debug_span_order(device, variant, spec.ctypes.data, nfr.ctypes.data, n, bands, s6.ctypes.data, blocks, caps.ctypes.data, *outs)
        if rc != 0:
            raise WsaError(f"wsa_debug_span_order: error {rc}")
    if seg_cap is None:
        call(*([None] * 6))
        seg_cap = int(caps[0])
    else:
        caps[0] = int(seg_cap)                          # (tests: a table size the entry did not hand out is refused)
    seg_i = np.full((n, seg_cap, 8), GATE_SENTINEL, np.int32)
    seg_count = np.full(n, 0xffffffff, np.uint32)
    hist = np.full(SPAN_BUCKETS, sentinel, np.uint32)
    key = np.full((n, seg_cap, 2), sentinel, np.uint32)
    order = np.full((n * seg_cap, 2), sentinel, np.uint32)
    counters = np.full(4, sentinel, np.uint32)
    out = dict(seg_i=seg_i, seg_count=seg_count, hist=hist, key=key, order=order, counters=counters, seg_cap=seg_cap)
    try:
        call(seg_i.ctypes.data, seg_count.ctypes.data, hist.ctypes.data, key.ctypes.data, order.ctypes.data, counters.ctypes.data)
    except WsaError as e:
        e.out = out
        raise
    return dict(seg_i=seg_i, seg_count=seg_count, hist=hist, key=key, order=order, counters=counters, seg_cap=seg_cap)
