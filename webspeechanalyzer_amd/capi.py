"""ctypes binding of include/wsa.h (libwsa.so).  No CPU fallback: if the HIP library is missing or no
gfx950 device is present, construction raises."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
NFEAT = 53


class WsaError(RuntimeError):
    pass


class _Config(ctypes.Structure):
    _fields_ = [("spec_type", ctypes.c_int32), ("output_level", ctypes.c_int32),
                ("f_min", ctypes.c_double), ("f_max", ctypes.c_double),
                ("N_fft_bins", ctypes.c_int32), ("N_mel_bins", ctypes.c_int32),
                ("window_width", ctypes.c_double), ("window_step", ctypes.c_double),
                ("pause_length", ctypes.c_double), ("min_seg_length", ctypes.c_double),
                ("auto_noise_gate", ctypes.c_int32),
                ("voiced_max_dB", ctypes.c_double), ("voiced_min_dB", ctypes.c_double),
                ("pre_norm_gain", ctypes.c_double), ("high_f_emph", ctypes.c_double)]


class _Geometry(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("nfft", "win", "hop", "bands", "kmax")]


class _DeviceResult(ctypes.Structure):
    _fields_ = [("n_clips", ctypes.c_uint32), ("n_rows", ctypes.c_uint32), ("n_segments", ctypes.c_uint32),
                ("n_frames_total", ctypes.c_uint32), ("status_flags", ctypes.c_uint32),
                ("d_row_meta", ctypes.c_void_p), ("d_row_feat", ctypes.c_void_p), ("d_segments", ctypes.c_void_p),
                ("d_clip_row_off", ctypes.c_void_p), ("d_clip_seg_off", ctypes.c_void_p),
                ("d_spectra", ctypes.c_void_p), ("d_clip_frame_off", ctypes.c_void_p), ("d_formants", ctypes.c_void_p),
                ("n_utterance_rows", ctypes.c_uint32), ("d_utt_meta", ctypes.c_void_p), ("d_utt_feat", ctypes.c_void_p),
                ("d_clip_utt_off", ctypes.c_void_p)]


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


class _StreamRows(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_segments", ctypes.c_uint32), ("status_flags", ctypes.c_uint32),
                ("row_meta", ctypes.c_void_p), ("row_feat", ctypes.c_void_p), ("segments", ctypes.c_void_p), ("stream_cuts", ctypes.c_void_p),
                ("formants", ctypes.c_void_p), ("row_formant_off", ctypes.c_void_p),
                ("n_utterance_rows", ctypes.c_uint32), ("utt_meta", ctypes.c_void_p), ("utt_feat", ctypes.c_void_p),
                ("n_track_points", ctypes.c_uint64), ("n_track_ranked", ctypes.c_uint64),
                ("track_off", ctypes.c_void_p), ("track_points", ctypes.c_void_p), ("track_ranked", ctypes.c_void_p)]


class _BatchInfo(ctypes.Structure):
    _fields_ = [("n_clips", ctypes.c_uint32), ("n_frames_total", ctypes.c_uint32),
                ("max_frames_per_clip", ctypes.c_uint32), ("bands", ctypes.c_uint32),
                ("rows_cap", ctypes.c_uint32), ("segments_cap", ctypes.c_uint32),
                ("workspace_bytes", ctypes.c_uint64)]


class _ModelDesc(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_int32), ("units", ctypes.c_void_p), ("activation", ctypes.c_void_p),
                ("kernel", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("in_min", ctypes.c_void_p), ("in_max", ctypes.c_void_p),
                ("labels", ctypes.c_void_p)]


class _ClassResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_classes", ctypes.c_uint32), ("n_callbacks", ctypes.c_uint32), ("n_clips", ctypes.c_uint32),
                ("d_prob", ctypes.c_void_p), ("d_cb", ctypes.c_void_p), ("d_cb_label", ctypes.c_void_p),
                ("d_cb_conf", ctypes.c_void_p), ("d_clip_conf", ctypes.c_void_p)]


class _StreamClassResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_classes", ctypes.c_uint32), ("n_callbacks", ctypes.c_uint32), ("n_streams", ctypes.c_uint32),
                ("prob", ctypes.c_void_p), ("cb", ctypes.c_void_p), ("cb_label", ctypes.c_void_p), ("cb_conf", ctypes.c_void_p),
                ("stream_conf", ctypes.c_void_p)]


class _TrainStats(ctypes.Structure):
    _fields_ = [("epochs_done", ctypes.c_uint32), ("loss", ctypes.c_double), ("acc", ctypes.c_double),
                ("val_loss", ctypes.c_double), ("val_acc", ctypes.c_double)]


ENSEMBLE_MAX = 8           # WSA_ENSEMBLE_MAX
_VP8, _U32x8 = ctypes.c_void_p * ENSEMBLE_MAX, ctypes.c_uint32 * ENSEMBLE_MAX


class _EnsembleResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_members", ctypes.c_uint32), ("n_callbacks", ctypes.c_uint32), ("n_clips", ctypes.c_uint32),
                ("n_classes", _U32x8), ("d_prob", _VP8), ("d_cb_label", _VP8), ("d_cb_conf", _VP8), ("d_cb_all_max", _VP8), ("d_clip_conf", _VP8),
                ("d_cb", ctypes.c_void_p), ("d_cb_db", ctypes.c_void_p), ("d_cb_top_label", ctypes.c_void_p), ("d_cb_top_conf", ctypes.c_void_p),
                ("d_cb_min_db", ctypes.c_void_p), ("d_cb_entropy", ctypes.c_void_p), ("d_clip_min_db", ctypes.c_void_p)]


class _EnsembleHost(ctypes.Structure):
    _fields_ = [("rows_cap", ctypes.c_uint32), ("cb_cap", ctypes.c_uint32),
                ("prob", _VP8), ("cb_label", _VP8), ("cb_conf", _VP8), ("cb_all_max", _VP8), ("clip_conf", _VP8),
                ("cb", ctypes.c_void_p), ("cb_db", ctypes.c_void_p), ("cb_top_label", ctypes.c_void_p), ("cb_top_conf", ctypes.c_void_p),
                ("cb_min_db", ctypes.c_void_p), ("cb_entropy", ctypes.c_void_p), ("clip_min_db", ctypes.c_void_p)]


class _StreamEnsembleResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_members", ctypes.c_uint32), ("n_callbacks", ctypes.c_uint32), ("n_streams", ctypes.c_uint32),
                ("n_classes", _U32x8), ("prob", _VP8), ("cb_label", _VP8), ("cb_conf", _VP8), ("cb_all_max", _VP8), ("stream_conf", _VP8),
                ("cb", ctypes.c_void_p), ("cb_db", ctypes.c_void_p), ("cb_top_label", ctypes.c_void_p), ("cb_top_conf", ctypes.c_void_p),
                ("cb_min_db", ctypes.c_void_p), ("cb_entropy", ctypes.c_void_p), ("stream_min_db", ctypes.c_void_p)]


class _KnnResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_classes", ctypes.c_uint32), ("k", ctypes.c_uint32), ("k_eff", ctypes.c_uint32),
                ("d_label", ctypes.c_void_p), ("d_conf", ctypes.c_void_p), ("d_nbr", ctypes.c_void_p), ("d_sim", ctypes.c_void_p)]


class _KnnFoldResult(ctypes.Structure):
    _fields_ = [("n_callbacks", ctypes.c_uint32), ("n_classes", ctypes.c_uint32), ("n_clips", ctypes.c_uint32),
                ("d_cb", ctypes.c_void_p), ("d_cb_label", ctypes.c_void_p), ("d_cb_conf", ctypes.c_void_p), ("d_clip_conf", ctypes.c_void_p)]


class _StreamKnnResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_classes", ctypes.c_uint32), ("k", ctypes.c_uint32), ("k_eff", ctypes.c_uint32),
                ("n_callbacks", ctypes.c_uint32), ("n_streams", ctypes.c_uint32), ("slices", ctypes.c_uint32),
                ("label", ctypes.c_void_p), ("conf", ctypes.c_void_p), ("nbr", ctypes.c_void_p), ("sim", ctypes.c_void_p),
                ("cb", ctypes.c_void_p), ("cb_label", ctypes.c_void_p), ("cb_conf", ctypes.c_void_p), ("stream_conf", ctypes.c_void_p)]


REGRESS_GROUP_MAX = 8      # WSA_REGRESS_GROUP_MAX
_VPH = ctypes.c_void_p * REGRESS_GROUP_MAX


class _ValueResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_heads", ctypes.c_uint32), ("n_callbacks", ctypes.c_uint32), ("n_clips", ctypes.c_uint32),
                ("d_value", _VPH), ("d_cb_value", _VPH), ("d_cb_weight", _VPH), ("d_clip_sum", _VPH), ("d_clip_weight", _VPH), ("d_clip_value", _VPH),
                ("d_cb", ctypes.c_void_p)]


class _ValueHost(ctypes.Structure):
    _fields_ = [("rows_cap", ctypes.c_uint32), ("cb_cap", ctypes.c_uint32),
                ("value", _VPH), ("cb_value", _VPH), ("cb_weight", _VPH), ("clip_sum", _VPH), ("clip_weight", _VPH), ("clip_value", _VPH),
                ("cb", ctypes.c_void_p)]


class _StreamDbResult(ctypes.Structure):
    _fields_ = [("first_row", ctypes.c_uint32), ("n_added", ctypes.c_uint32), ("n_replaced", ctypes.c_uint32), ("not_fitted", ctypes.c_uint32),
                ("kept", ctypes.c_void_p), ("replaced", ctypes.c_void_p)]


class _StreamValueResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_uint32), ("n_heads", ctypes.c_uint32), ("n_callbacks", ctypes.c_uint32), ("n_streams", ctypes.c_uint32),
                ("value", _VPH), ("cb", ctypes.c_void_p), ("cb_value", _VPH), ("cb_weight", _VPH),
                ("stream_sum", _VPH), ("stream_weight", _VPH), ("stream_value", _VPH)]


# every symbol include/wsa.h declares (checked by tests/test_abi.py)
ABI_VERSION = 5            # WSA_ABI_VERSION of include/wsa.h this binding's structures follow
ABI_SYMBOLS = ["wsa_config_default", "wsa_abi_version", "wsa_create", "wsa_destroy", "wsa_last_error",
               "wsa_geometry_for", "wsa_bins_hz", "wsa_batch_create", "wsa_batch_destroy", "wsa_batch_run",
               "wsa_batch_run_host", "wsa_batch_result", "wsa_batch_copy_rows", "wsa_batch_copy_spectra",
               "wsa_batch_get_info", "wsa_batch_stage_ms", "wsa_batch_enable_timing", "wsa_batch_run_frontend",
               "wsa_batch_run_backend", "wsa_batch_enable_trace", "wsa_batch_copy_trace", "wsa_batch_copy_formants", "wsa_batch_copy_utterance",
               "wsa_batch_tracks_info", "wsa_batch_copy_tracks", "wsa_batch_create_resampled", "wsa_resample_length", "wsa_batch_copy_pcm", "wsa_batch_create_mixed",
               "wsa_stream_create", "wsa_stream_destroy", "wsa_stream_samples_per_step", "wsa_stream_step",
               "wsa_stream_host_input", "wsa_stream_step_host", "wsa_stream_collect", "wsa_stream_enable_graph",
               "wsa_batch_keep_spectra", "wsa_batch_backend_reruns", "wsa_stream_time_steps", "wsa_batch_run_host_i16",
               "wsa_gather_create", "wsa_gather_destroy", "wsa_gather_rows", "wsa_gather_copy_rows", "wsa_host_alloc", "wsa_host_free", "wsa_queue_create", "wsa_queue_destroy",
               # additions within version 5 (probe for wsa_model_create): the app's syllable classifier
               "wsa_model_create", "wsa_model_destroy", "wsa_classify_rows", "wsa_batch_classify", "wsa_batch_class_result", "wsa_batch_copy_classes",
               # additions within version 5 (probe for wsa_stream_set_model): the classifier inside the stream step
               "wsa_stream_set_model", "wsa_stream_classes",
               # additions within version 5 (probe for wsa_ensemble_create): every model DB of the app in one pass
               "wsa_ensemble_create", "wsa_ensemble_destroy", "wsa_batch_classify_ensemble", "wsa_batch_ensemble_result", "wsa_batch_copy_ensemble",
               "wsa_stream_set_ensemble", "wsa_stream_ensemble_classes",
               # additions within version 5 (probe for wsa_stream_create_mixed): streams of different rates, converted inside the step
               "wsa_stream_create_mixed", "wsa_stream_input_capacity", "wsa_stream_input_stride", "wsa_stream_paced_input", "wsa_stream_step_frame_capacity",
               "wsa_stream_step_n", "wsa_stream_step_host_n", "wsa_resample_ready", "wsa_stream_frames_bound", "wsa_stream_copy_converted",
               # additions within version 5 (probe for wsa_trainer_create): training the app's classifiers (K7, spec TR-1)
               "wsa_trainer_create", "wsa_trainer_destroy", "wsa_trainer_epoch", "wsa_trainer_stats", "wsa_trainer_copy_weights", "wsa_trainer_model",
               # additions within version 5 (probe for wsa_regress_trainer_create): the app's regression models (ords_*, spec TR-2)
               "wsa_regress_rows", "wsa_batch_regress", "wsa_batch_copy_values", "wsa_regress_trainer_create", "wsa_queue_synchronize",
               # additions within version 5 (probe for wsa_dbstats_create): predicting a labelled feature DB and the app's results table (K8, spec DS-1)
               "wsa_dbstats_create", "wsa_dbstats_destroy", "wsa_dbstats_set_classes", "wsa_dbstats_set_values", "wsa_dbstats_predict_classes",
               "wsa_dbstats_decide_rows", "wsa_dbstats_predict_values", "wsa_dbstats_table", "wsa_dbstats_copy_classes", "wsa_dbstats_copy_values",
               "wsa_dbstats_copy_probs",
               # additions within version 5 (probe for wsa_level_feature_count): models, training and DBs at the row widths of levels 11 and 12
               "wsa_level_feature_count", "wsa_wide_dbstats_create",
               # additions within version 5 (probe for wsa_knn_create): the app's ml5 KNN classifier (K9, spec KN-1)
               "wsa_knn_create", "wsa_knn_destroy", "wsa_knn_add", "wsa_knn_count", "wsa_knn_classify_rows", "wsa_knn_tile_info",
               "wsa_batch_knn", "wsa_batch_knn_result", "wsa_batch_copy_knn",
               # additions within version 5 (probe for wsa_stream_set_knn): KNN on live streams (K9s) and the fold of KNN results (spec KN-2)
               "wsa_batch_knn_fold", "wsa_batch_knn_fold_result", "wsa_batch_copy_knn_fold", "wsa_stream_set_knn", "wsa_stream_knn_classes",
               # additions within version 5 (probe for wsa_regress_group_create): V, A, D per callback in batches and streams (spec RG-1)
               "wsa_regress_group_create", "wsa_regress_group_destroy", "wsa_regress_group_rows", "wsa_batch_regress_group", "wsa_batch_value_result",
               "wsa_batch_copy_value_fold", "wsa_stream_set_regress", "wsa_stream_values",
               # additions within version 5 (probe for wsa_train_group_create): a group of trainers in one pass of grouped launches (K7g, spec TG-1)
               "wsa_train_group_create", "wsa_train_group_destroy", "wsa_train_group_epoch", "wsa_train_group_stats", "wsa_train_group_launches",
               "wsa_train_group_launch_count",
               # additions within version 5 (probe for wsa_stream_set_input_format): 16-bit and G.711 PCM into streams, unpacked in the step (spec PK-1)
               "wsa_stream_set_input_format", "wsa_stream_host_input_packed", "wsa_stream_input_stride_bytes", "wsa_stream_step_packed",
               "wsa_stream_time_steps_packed", "wsa_pcm_decode",
               # additions within version 5 (probe for wsa_batch_run_host_packed): every PCM encoding a WAV holds into batches, unpacked on the GPU (spec PK-2)
               "wsa_batch_run_host_packed", "wsa_batch_set_input_format", "wsa_batch_packed_offset", "wsa_batch_run_packed",
               # additions within version 5 (probe for wsa_batch_set_input_channels): any channel, every channel or the mono mix of interleaved PCM (spec PK-3)
               "wsa_pcm_decode_select", "wsa_batch_set_input_channels", "wsa_batch_run_host_channels", "wsa_stream_set_input_channels",
               "wsa_pcm_channels_tile_frames",
               # additions within version 5 (probe for wsa_featdb_create): the feature DB that stays on the device (K10, spec FD-1)
               "wsa_featdb_create", "wsa_featdb_destroy", "wsa_featdb_clear", "wsa_featdb_count", "wsa_featdb_append_batch", "wsa_featdb_append_host",
               "wsa_featdb_device_rows", "wsa_featdb_copy_rows", "wsa_featdb_gather", "wsa_featdb_ranges", "wsa_featdb_tile_info",
               "wsa_trainer_create_db", "wsa_regress_trainer_create_db", "wsa_featdb_dbstats_create",
               # additions within version 5 (probe for wsa_stream_set_featdb): live streams collect into the device DB, inside the step (spec FD-2)
               "wsa_stream_set_featdb", "wsa_stream_db_rows", "wsa_stream_featdb_tile_info"]
CHANNEL_MIX = 0xFFFFFFFF                                # WSA_CHANNEL_MIX: the `select` word that takes the mono mix (spec PK-3); 'mix' in the Python entries
PCM_F32, PCM_I16, PCM_MULAW, PCM_ALAW = 0, 1, 2, 3      # WSA_PCM_* of include/wsa.h
PCM_U8, PCM_I24, PCM_I32, PCM_F64 = 8, 9, 10, 11        # ... the file encodings of spec PK-2 (batches and pcm_decode; 4 .. 7 are unassigned)
_PCM_NAMES = {"f32": PCM_F32, "i16": PCM_I16, "mulaw": PCM_MULAW, "alaw": PCM_ALAW, "u8": PCM_U8, "i24": PCM_I24, "i32": PCM_I32, "f64": PCM_F64}
_PCM_DTYPE = {PCM_F32: np.float32, PCM_I16: np.int16, PCM_MULAW: np.uint8, PCM_ALAW: np.uint8,
              PCM_U8: np.uint8, PCM_I24: np.uint8, PCM_I32: np.int32, PCM_F64: np.float64}
_PCM_ELEMS = {PCM_I24: 3}                               # array elements per sample ('i24': three uint8)
TRAIN_GROUP_MAX = 32       # WSA_TRAIN_GROUP_MAX of include/wsa.h

_LIB = None
_U32_RESULT = ("wsa_stream_input_capacity", "wsa_stream_paced_input", "wsa_stream_input_stride", "wsa_stream_step_frame_capacity", "wsa_stream_frames_bound",
               "wsa_stream_input_stride_bytes")


def library_path():
    # WSA_LIB_DIR: another build of the same sources (A/B timing of two builds in one GPU session, tools/README.md); never a fallback
    return os.path.join(os.environ.get("WSA_LIB_DIR") or os.path.join(_HERE, "lib"), "libwsa.so")


def build_library():
    """hipcc cross-compiles for gfx950 without a GPU (used by __graft_entry__.build())."""
    subprocess.run(["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc")], check=True)
    return library_path()


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise WsaError(f"{path} is missing: build it with `make -C webspeechanalyzer_amd/csrc` "
                       "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    # PyTorch-ROCm bundles its own HIP runtime (soname libamdhip64.so.7).  Device pointers and streams
    # handed to libwsa come from torch, so both must share ONE runtime: load torch's first, then the
    # loader satisfies libwsa's DT_NEEDED libamdhip64.so.7 from the copy already in the process.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    vp, i32, u32, u64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    L.wsa_abi_version.restype = ctypes.c_int
    if L.wsa_abi_version() != ABI_VERSION:
        raise WsaError(f"{path} has ABI version {L.wsa_abi_version()}, this binding is written against {ABI_VERSION} (include/wsa.h): rebuild the library")
    L.wsa_config_default.argtypes = [ctypes.POINTER(_Config)]
    L.wsa_create.argtypes = [ctypes.POINTER(_Config), i32, ctypes.POINTER(vp)]
    L.wsa_destroy.argtypes = [vp]
    L.wsa_last_error.restype = ctypes.c_char_p
    L.wsa_last_error.argtypes = [vp]
    L.wsa_geometry_for.argtypes = [vp, dbl, ctypes.POINTER(_Geometry)]
    L.wsa_bins_hz.argtypes = [vp, dbl, vp, i32]
    L.wsa_batch_create.argtypes = [vp, u32, vp, dbl, ctypes.POINTER(vp)]
    L.wsa_batch_create_resampled.argtypes = [vp, u32, vp, dbl, dbl, ctypes.POINTER(vp)]
    L.wsa_batch_create_mixed.argtypes = [vp, u32, vp, vp, dbl, ctypes.POINTER(vp)]
    L.wsa_resample_length.argtypes = [u64, dbl, dbl]
    L.wsa_resample_length.restype = ctypes.c_uint64
    L.wsa_batch_copy_pcm.argtypes = [vp, vp, vp, u64]
    L.wsa_batch_destroy.argtypes = [vp]
    L.wsa_batch_run.argtypes = [vp, vp, u64, vp]
    L.wsa_batch_run_host.argtypes = [vp, vp, vp]
    L.wsa_batch_run_host_i16.argtypes = [vp, vp, vp, vp]
    L.wsa_batch_run_frontend.argtypes = [vp, vp, u64, vp]
    L.wsa_batch_run_backend.argtypes = [vp, vp, vp]
    L.wsa_batch_result.argtypes = [vp, vp, ctypes.POINTER(_DeviceResult)]
    L.wsa_batch_copy_rows.argtypes = [vp, vp, vp, vp, u32, vp, u32, vp, vp]
    L.wsa_batch_copy_spectra.argtypes = [vp, vp, vp, u64, vp]
    L.wsa_batch_get_info.argtypes = [vp, ctypes.POINTER(_BatchInfo)]
    L.wsa_batch_stage_ms.argtypes = [vp, vp]
    L.wsa_batch_enable_timing.argtypes = [vp, i32]
    L.wsa_batch_enable_trace.argtypes = [vp, i32]
    L.wsa_batch_keep_spectra.argtypes = [vp, i32]
    L.wsa_batch_backend_reruns.argtypes = [vp, vp]
    L.wsa_batch_copy_trace.argtypes = [vp, vp, vp, u64]
    L.wsa_batch_copy_formants.argtypes = [vp, vp, vp, u64]
    L.wsa_batch_tracks_info.argtypes = [vp, vp, vp]
    L.wsa_batch_copy_tracks.argtypes = [vp, vp, vp, vp, u64, vp, u64]
    L.wsa_batch_copy_utterance.argtypes = [vp, vp, vp, vp, u32, vp]
    L.wsa_stream_create.argtypes = [vp, u32, dbl, u32, u32, ctypes.POINTER(vp)]
    L.wsa_stream_destroy.argtypes = [vp]
    L.wsa_stream_samples_per_step.argtypes = [vp]
    L.wsa_stream_samples_per_step.restype = u32
    L.wsa_stream_step.argtypes = [vp, vp, u64, vp, vp]
    L.wsa_stream_host_input.argtypes = [vp]
    L.wsa_stream_host_input.restype = ctypes.POINTER(ctypes.c_float)
    L.wsa_stream_step_host.argtypes = [vp, vp, vp]
    L.wsa_stream_collect.argtypes = [vp, vp, ctypes.POINTER(_StreamRows)]
    L.wsa_stream_enable_graph.argtypes = [vp, i32]
    L.wsa_stream_time_steps.argtypes = [vp, u32, vp, u32, vp, vp, vp]
    L.wsa_gather_create.argtypes = [vp, i32, i32, vp]
    L.wsa_gather_destroy.argtypes = [vp]
    L.wsa_gather_rows.argtypes = [vp, vp, vp, vp]
    L.wsa_gather_copy_rows.argtypes = [vp, vp, vp, u32]
    L.wsa_model_create.argtypes = [vp, ctypes.POINTER(_ModelDesc), ctypes.POINTER(vp)]
    L.wsa_model_destroy.argtypes = [vp]
    L.wsa_classify_rows.argtypes = [vp, vp, u32, vp, vp]
    L.wsa_batch_classify.argtypes = [vp, vp, vp]
    L.wsa_batch_class_result.argtypes = [vp, vp, ctypes.POINTER(_ClassResult)]
    L.wsa_batch_copy_classes.argtypes = [vp, vp, vp, u32, vp, vp, vp, u32, vp]
    L.wsa_stream_set_model.argtypes = [vp, vp]
    L.wsa_stream_classes.argtypes = [vp, ctypes.POINTER(_StreamClassResult)]
    L.wsa_ensemble_create.argtypes = [vp, vp, u32, ctypes.POINTER(vp)]
    L.wsa_ensemble_destroy.argtypes = [vp]
    L.wsa_batch_classify_ensemble.argtypes = [vp, vp, vp]
    L.wsa_batch_ensemble_result.argtypes = [vp, vp, ctypes.POINTER(_EnsembleResult)]
    L.wsa_batch_copy_ensemble.argtypes = [vp, vp, ctypes.POINTER(_EnsembleHost)]
    L.wsa_stream_set_ensemble.argtypes = [vp, vp]
    L.wsa_stream_ensemble_classes.argtypes = [vp, ctypes.POINTER(_StreamEnsembleResult)]
    L.wsa_stream_create_mixed.argtypes = [vp, u32, vp, dbl, u32, u32, ctypes.POINTER(vp)]
    for name in ("wsa_stream_input_capacity", "wsa_stream_paced_input"):
        getattr(L, name).argtypes = [vp, u32]
    for name in ("wsa_stream_input_stride", "wsa_stream_step_frame_capacity"):
        getattr(L, name).argtypes = [vp]
    L.wsa_stream_frames_bound.argtypes = [u32, u32, dbl]
    for name in _U32_RESULT:
        getattr(L, name).restype = u32
    L.wsa_stream_step_n.argtypes = [vp, vp, u64, vp, vp, vp]
    L.wsa_stream_step_host_n.argtypes = [vp, vp, vp, vp]
    L.wsa_resample_ready.argtypes = [u64, dbl, dbl]
    L.wsa_resample_ready.restype = ctypes.c_uint64
    L.wsa_stream_copy_converted.argtypes = [vp, vp, u32, vp]
    L.wsa_trainer_create.argtypes = [vp, ctypes.POINTER(_ModelDesc), vp, vp, u32, u32, u32, dbl, ctypes.POINTER(vp)]
    L.wsa_trainer_destroy.argtypes = [vp]
    L.wsa_trainer_epoch.argtypes = [vp, vp, vp]
    L.wsa_trainer_stats.argtypes = [vp, vp, ctypes.POINTER(_TrainStats)]
    L.wsa_trainer_copy_weights.argtypes = [vp, vp, vp, vp]
    L.wsa_trainer_model.argtypes = [vp, vp, ctypes.POINTER(vp)]
    L.wsa_queue_synchronize.argtypes = [vp, vp]
    L.wsa_regress_rows.argtypes = [vp, dbl, dbl, vp, u32, vp, vp]
    L.wsa_batch_regress.argtypes = [vp, vp, dbl, dbl, vp]
    L.wsa_batch_copy_values.argtypes = [vp, vp, vp, u32, ctypes.POINTER(u32)]
    L.wsa_regress_trainer_create.argtypes = [vp, ctypes.POINTER(_ModelDesc), vp, vp, u32, u32, u32, dbl, dbl, dbl, ctypes.POINTER(vp)]
    L.wsa_dbstats_create.argtypes = [vp, vp, vp, u32, u32, vp, u32, ctypes.POINTER(vp)]
    L.wsa_wide_dbstats_create.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, ctypes.POINTER(vp)]
    L.wsa_level_feature_count.argtypes = [i32]
    L.wsa_level_feature_count.restype = i32
    L.wsa_dbstats_destroy.argtypes = [vp]
    L.wsa_dbstats_set_classes.argtypes = [vp, u32, vp, vp]
    L.wsa_dbstats_set_values.argtypes = [vp, u32, vp, vp]
    L.wsa_dbstats_predict_classes.argtypes = [vp, u32, vp, vp, vp]
    L.wsa_dbstats_decide_rows.argtypes = [vp, u32, vp, u32, vp, vp]
    L.wsa_dbstats_predict_values.argtypes = [vp, u32, vp, dbl, dbl, vp]
    L.wsa_dbstats_table.argtypes = [vp, vp, vp, vp, vp]
    L.wsa_dbstats_copy_classes.argtypes = [vp, u32, vp, vp]
    L.wsa_dbstats_copy_values.argtypes = [vp, u32, vp, vp]
    L.wsa_dbstats_copy_probs.argtypes = [vp, vp, vp, u32]
    L.wsa_knn_create.argtypes = [vp, i32, i32, u32, ctypes.POINTER(vp)]
    L.wsa_knn_destroy.argtypes = [vp]
    L.wsa_knn_add.argtypes = [vp, vp, vp, u32, vp]
    L.wsa_knn_count.argtypes = [vp, vp, ctypes.POINTER(u32), vp]
    L.wsa_knn_classify_rows.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, vp]
    L.wsa_knn_tile_info.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.wsa_batch_knn.argtypes = [vp, vp, u32, vp]
    L.wsa_batch_knn_result.argtypes = [vp, vp, ctypes.POINTER(_KnnResult)]
    L.wsa_batch_copy_knn.argtypes = [vp, vp, vp, vp, vp, vp, u32]
    L.wsa_batch_knn_fold.argtypes = [vp, vp]
    L.wsa_batch_knn_fold_result.argtypes = [vp, vp, ctypes.POINTER(_KnnFoldResult)]
    L.wsa_batch_copy_knn_fold.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    L.wsa_stream_set_knn.argtypes = [vp, vp, u32]
    L.wsa_stream_knn_classes.argtypes = [vp, ctypes.POINTER(_StreamKnnResult)]
    L.wsa_regress_group_create.argtypes = [vp, vp, vp, vp, u32, ctypes.POINTER(vp)]
    L.wsa_regress_group_destroy.argtypes = [vp]
    L.wsa_regress_group_rows.argtypes = [vp, vp, u32, vp, vp]
    L.wsa_batch_regress_group.argtypes = [vp, vp, vp]
    L.wsa_batch_value_result.argtypes = [vp, vp, ctypes.POINTER(_ValueResult)]
    L.wsa_batch_copy_value_fold.argtypes = [vp, vp, ctypes.POINTER(_ValueHost)]
    L.wsa_stream_set_regress.argtypes = [vp, vp]
    L.wsa_stream_values.argtypes = [vp, ctypes.POINTER(_StreamValueResult)]
    L.wsa_train_group_create.argtypes = [vp, vp, u32, ctypes.POINTER(vp)]
    L.wsa_train_group_destroy.argtypes = [vp]
    L.wsa_train_group_epoch.argtypes = [vp, vp, vp]
    L.wsa_train_group_stats.argtypes = [vp, vp, vp]
    L.wsa_train_group_launches.argtypes = [vp, ctypes.POINTER(u32)]
    L.wsa_train_group_launch_count.argtypes = [vp, vp, vp, vp, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.wsa_stream_set_input_format.argtypes = [vp, i32, vp]
    L.wsa_stream_host_input_packed.argtypes = [vp]
    L.wsa_stream_host_input_packed.restype = vp
    L.wsa_stream_input_stride_bytes.argtypes = [vp]
    L.wsa_stream_input_stride_bytes.restype = u32
    L.wsa_stream_step_packed.argtypes = [vp, vp, u64, vp, vp, vp]
    L.wsa_stream_time_steps_packed.argtypes = [vp, u32, vp, u32, vp, vp, vp]
    L.wsa_pcm_decode.argtypes = [i32, vp, u64, u32, vp]
    L.wsa_batch_run_host_packed.argtypes = [vp, vp, vp, vp, vp]
    L.wsa_batch_set_input_format.argtypes = [vp, vp, vp]
    L.wsa_batch_packed_offset.argtypes = [vp, u32]
    L.wsa_batch_packed_offset.restype = u64
    L.wsa_batch_run_packed.argtypes = [vp, vp, vp]
    L.wsa_pcm_decode_select.argtypes = [i32, vp, u64, u32, u32, vp]
    L.wsa_batch_set_input_channels.argtypes = [vp, vp, vp, vp, vp]
    L.wsa_batch_run_host_channels.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.wsa_stream_set_input_channels.argtypes = [vp, i32, vp, vp, vp]
    L.wsa_pcm_channels_tile_frames.argtypes = [i32, u32]
    L.wsa_featdb_create.argtypes = [vp, i32, u32, ctypes.POINTER(vp)]
    L.wsa_featdb_destroy.argtypes = [vp]
    L.wsa_featdb_clear.argtypes = [vp]
    L.wsa_featdb_count.argtypes = [vp, ctypes.POINTER(u32)]
    L.wsa_featdb_append_batch.argtypes = [vp, vp, vp, ctypes.POINTER(u32), ctypes.POINTER(u32), vp, u32]
    L.wsa_featdb_append_host.argtypes = [vp, vp, u32, vp]
    L.wsa_featdb_device_rows.argtypes = [vp, ctypes.POINTER(vp)]
    L.wsa_featdb_copy_rows.argtypes = [vp, vp, u32, u32, vp]
    L.wsa_featdb_gather.argtypes = [vp, vp, u32, vp, vp]
    L.wsa_featdb_ranges.argtypes = [vp, vp, u32, vp, vp, vp]
    L.wsa_featdb_tile_info.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.wsa_trainer_create_db.argtypes = [vp, ctypes.POINTER(_ModelDesc), vp, vp, vp, u32, u32, u32, dbl, ctypes.POINTER(vp)]
    L.wsa_regress_trainer_create_db.argtypes = [vp, ctypes.POINTER(_ModelDesc), vp, vp, vp, u32, u32, u32, dbl, dbl, dbl, ctypes.POINTER(vp)]
    L.wsa_featdb_dbstats_create.argtypes = [vp, vp, u32, u32, vp, u32, vp, u32, ctypes.POINTER(vp)]
    L.wsa_stream_set_featdb.argtypes = [vp, vp]
    L.wsa_stream_db_rows.argtypes = [vp, ctypes.POINTER(_StreamDbResult)]
    L.wsa_stream_featdb_tile_info.argtypes = [ctypes.POINTER(i32)] * 4
    for name in ABI_SYMBOLS:
        if name in _U32_RESULT or name in ("wsa_resample_ready", "wsa_level_feature_count", "wsa_batch_packed_offset", "wsa_pcm_channels_tile_frames"):
            continue
        if name not in ("wsa_abi_version", "wsa_last_error", "wsa_config_default", "wsa_destroy", "wsa_batch_destroy", "wsa_resample_length",
                        "wsa_stream_destroy", "wsa_stream_samples_per_step", "wsa_stream_host_input", "wsa_stream_host_input_packed", "wsa_gather_destroy", "wsa_host_free",
                        "wsa_model_destroy", "wsa_ensemble_destroy", "wsa_trainer_destroy", "wsa_dbstats_destroy", "wsa_knn_destroy",
                        "wsa_regress_group_destroy", "wsa_train_group_destroy", "wsa_featdb_destroy"):
            getattr(L, name).restype = ctypes.c_int
    _LIB = L
    return L


def pcm_format(fmt):
    """A WSA_PCM_* number from a number or one of 'f32', 'i16', 'mulaw', 'alaw', 'u8', 'i24', 'i32', 'f64'; anything else is refused."""
    if isinstance(fmt, str):
        if fmt not in _PCM_NAMES:
            raise WsaError(f"unknown input format {fmt!r} ('f32', 'i16', 'mulaw', 'alaw', 'u8', 'i24', 'i32', 'f64')")
        return _PCM_NAMES[fmt]
    if isinstance(fmt, (bool, float)) or int(fmt) not in _PCM_DTYPE:
        raise WsaError(f"unknown input format {fmt!r} (PCM_F32 0, PCM_I16 1, PCM_MULAW 2, PCM_ALAW 3, PCM_U8 8, PCM_I24 9, PCM_I32 10, PCM_F64 11)")
    return int(fmt)


def _pcm_array(fmt, f, array):
    """`array` as the contiguous flat samples of format `f`; the wrong sample type is refused, never converted."""
    a = np.ascontiguousarray(array)
    if a.dtype != _PCM_DTYPE[f]:
        raise WsaError(f"format {fmt!r} takes {np.dtype(_PCM_DTYPE[f]).name} samples, not {a.dtype.name}")
    return a.reshape(-1)


def channel_select(select, channels=None):
    """A PK-3 `select` word from a channel index or 'mix' (or CHANNEL_MIX); with `channels` given, an index at or above it is refused."""
    if isinstance(select, str):
        if select != "mix":
            raise WsaError(f"select {select!r}: a channel index or 'mix'")
        return CHANNEL_MIX
    if isinstance(select, (bool, float)) or not 0 <= int(select) <= CHANNEL_MIX:
        raise WsaError(f"select {select!r}: a channel index or 'mix'")
    s = int(select)
    if channels is not None and s != CHANNEL_MIX and s >= int(channels):
        raise WsaError(f"select {s} is neither a channel below {int(channels)} nor 'mix'")
    return s


def pcm_decode(fmt, array, channels=1, select=0):
    """Specs PK-1 / PK-2 / PK-3 on the host (wsa_pcm_decode_select, no device): channel `select` (0 by default; 'mix': the mono mix) of the
    interleaved frames in `array` (int16 for 'i16', uint8 for the G.711 laws and 'u8', three uint8 per sample for 'i24', int32 for 'i32',
    float64 for 'f64', float32 for 'f32'; a trailing partial frame is ignored where it does not hold the selected channel) as float32 — the
    floats a stream set or a batch fed `array` analyses."""
    f = pcm_format(fmt)
    ch = int(channels)
    if not 1 <= ch <= 64:
        raise WsaError(f"channel count {ch} outside 1 .. 64")
    sel = channel_select(select, ch)
    a = _pcm_array(fmt, f, array)
    size = a.size // _PCM_ELEMS.get(f, 1)            # whole samples
    last = ch - 1 if sel == CHANNEL_MIX else sel     # the last channel of a frame that is read
    n = (size - 1 - last) // ch + 1 if size > last else 0          # frames whose selected channel (the mix: every channel) is present
    out = np.zeros(n, np.float32)
    if lib().wsa_pcm_decode_select(f, a.ctypes.data, n, ch, sel, out.ctypes.data) != 0:
        raise WsaError("wsa_pcm_decode_select refused its arguments")
    return out


def pcm_channels_tile_frames(fmt, channels):
    """wsa_pcm_channels_tile_frames: the frames of one source a workgroup of batch_deinterleave_kernel takes at a time (spec PK-3)."""
    return int(lib().wsa_pcm_channels_tile_frames(pcm_format(fmt), int(channels)))


def level_feature_count(output_level):
    """wsa_level_feature_count: 53 (levels 5 and 13), 264 (level 11), 23 (level 12), 0 at any other level."""
    return int(lib().wsa_level_feature_count(int(output_level)))


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


class Analyzer:
    """One configured context on one GPU (wsa_ctx)."""

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
        from . import nnmodel
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

    def close(self):
        if self.h:
            self.L.wsa_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """A planned batch shape (wsa_batch).  `run*` take raw device pointers (e.g. torch data_ptr())."""

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

    def run_host_packed(self, clips, formats, channels=None, stream=0):
        """Clips in host memory as the bytes a file holds (spec PK-2): clip i in formats[i] ('f32', 'i16', 'mulaw', 'alaw', 'u8', 'i24', 'i32',
        'f64' or the numbers; one name for all clips is fine), interleaved over channels[i] channels, channel 0 analysed; unpacked on the device.
        The arrays have the format's sample type (as pcm_decode takes them) and hold at least the plan's frames."""
        fm, ch = self._formats(formats, channels)
        held = []
        ns_in = getattr(self, "n_samples_in", self.n_samples)
        for i, c in enumerate(clips):
            f = int(fm[i])
            a = _pcm_array(f, f, c) if f in _PCM_DTYPE else np.ascontiguousarray(c).reshape(-1)
            need = int(ns_in[i]) * (int(ch[i]) if ch is not None else 1) * _PCM_ELEMS.get(f, 1)
            if f in _PCM_DTYPE and a.size < need:
                raise WsaError(f"clip {i}: {a.size} elements, the plan's {int(ns_in[i])} frames need {need}")
            held.append(a)
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
        held, ptrs = [], []
        ns_in = getattr(self, "n_samples_in", self.n_samples)
        for i, c in enumerate(clips):
            if src is not None and int(src[i]) != i:
                ptrs.append(None)
                continue
            f = int(fm[i])
            a = _pcm_array(f, f, c) if f in _PCM_DTYPE else np.ascontiguousarray(c).reshape(-1)
            need = int(ns_in[i]) * (int(ch[i]) if ch is not None else 1) * _PCM_ELEMS.get(f, 1)
            if f in _PCM_DTYPE and a.size < need:
                raise WsaError(f"clip {i}: {a.size} elements, the plan's {int(ns_in[i])} frames need {need}")
            held.append(a)
            ptrs.append(a.ctypes.data)
        if len(ptrs) != len(self.n_samples):
            raise WsaError("one entry per clip (a consumer's may be None)")
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
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
        self.L.wsa_debug_batch_keep_counters.argtypes = [ctypes.c_void_p, ctypes.c_int32]
        self.an._check(self.L.wsa_debug_batch_keep_counters(self.h, int(on)))
        return self

    def tiers(self, stream=0):
        """Test entry: dict(flags, spans, redo) of the last run — the flag word (bit 1: the 140-entry track table overflowed), the number of spans and
        how many of them the paired tracker kernel handed to the one-span kernel.  Needs keep_counters() before the run, and is to be read before
        the first fetch of results (rows(), callbacks(), ...): a fetch that finds flag bit 1 reruns the back end, and these are the rerun's then."""
        out = (ctypes.c_uint32 * 3)()
        self.L.wsa_debug_batch_tiers.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
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

    def close(self):
        if self.h:
            self.L.wsa_batch_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _model_desc(spec):
    """(wsa_model_desc of an nnmodel.ModelSpec, the objects that own what it points to)."""
    from . import nnmodel
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


class Model:
    """wsa_model: a Dense classifier (the app's ml5 model) on the device of one context."""

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

    def close(self):
        if self.h:
            self.L.wsa_model_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Trainer:
    """wsa_trainer: minibatch SGD on the app's Dense classifiers (K7, spec TR-1).  `spec` holds the INITIAL weights, the ranges to
    normalise with and the legend; features [n][spec.units[0]] f64 (53, 264 or 23 wide) and labels [n] class indices are host arrays, the last n_val rows validation."""

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
        from . import nnmodel
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

    def close(self):
        if self.h:
            self.L.wsa_trainer_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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


class TrainGroup:
    """wsa_train_group: Trainers of one Analyzer stepped in lock step (K7g, spec TG-1): a group epoch is Trainer.epoch on every member,
    bit for bit, in about the launches of the longest one.  The members stay usable (stats, weights, model, a solo epoch between group
    epochs, all on the same stream); close the group before its members."""

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

    def close(self):
        if self.h:
            self.L.wsa_train_group_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DBSTATS_MAX_CLASSES, DBSTATS_MAX_HEADS, DBSTATS_CHUNK_ROWS = 256, 8, 256      # WSA_DBSTATS_* of include/wsa.h
_DB_CAT = np.dtype([("correct", "<u8"), ("wrong", "<u8"), ("blank", "<u8")])
_DB_CLASS = np.dtype([("count", "<u8"), ("correct", "<u8"), ("wrong", "<u8"), ("duration", "<f8"), ("first_row", "<u4"), ("reserved", "<u4")])
_DB_ORD = np.dtype([("true_n", "<u8"), ("pred_n", "<u8"), ("min", "<f8"), ("max", "<f8"), ("sq_sum", "<f8")])


class FeatureDBStats:
    """wsa_dbstats: one labelled feature DB on the device (K8, spec DS-1).  features [n][53] f64, or 264 / 23 wide: the rows of level 11 / 12 (None: a DB that is only counted) and
    durations [n] f64 are host arrays; vocab_sizes has one vocabulary size per categorical head, n_ord is the number of ordinal heads.
    Indices and values are what the device sees; webspeechanalyzer_amd.dbstats builds them from the app's rows."""

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

    def table(self, stream=0):
        """Synchronises; (cat [n_cat], cls [sum V], ord [n_ord]) as numpy records (wsa_dbstats_cat / _class / _ord)."""
        cat, cls, od = np.zeros(len(self.vocab), _DB_CAT), np.zeros(sum(self.vocab), _DB_CLASS), np.zeros(self.n_ord, _DB_ORD)
        self.an._check(self.L.wsa_dbstats_table(self.h, stream, cat.ctypes.data if len(cat) else None, cls.ctypes.data if len(cls) else None,
                                                od.ctypes.data if len(od) else None))
        return cat, cls, od

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

    def close(self):
        if self.h:
            self.L.wsa_dbstats_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FeatDB:
    """wsa_featdb: the feature columns of the app's feature DB on the device of one context (K10, spec FD-1): one allocation of
    capacity x width doubles, rows appended behind the ones it holds and never moved.  Strings stay with the caller
    (webspeechanalyzer_amd.featdb.DeviceDB keeps them); pass the same stream to every call."""

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

    def close(self):
        if self.h:
            self.L.wsa_featdb_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_featdb_append(db, level, meta, feat, clip_off=None, stream=0):
    """Test access to K10 on hand-built tables (csrc/featdb.hip wsa_debug_featdb_append; not part of include/wsa.h): meta [n][8] i32
    (None at levels 5 / 13 / 11), feat [n][stride] f64, clip_off [n_clips + 1] u32 (level 11).  The tables are uploaded with torch, the
    product's keep, scan and copy kernels run over them.  Returns (first DB row, kept)."""
    import torch
    L = lib()
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    L.wsa_debug_featdb_append.argtypes = [vp, i32, vp, vp, u32, vp, u32, u32, vp, ctypes.POINTER(u32), ctypes.POINTER(u32), vp, u32]
    L.wsa_debug_featdb_append.restype = ctypes.c_int
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
    L.wsa_debug_featdb_copy_capacity.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.wsa_debug_featdb_copy_capacity.restype = ctypes.c_int
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
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    L.wsa_debug_stream_featdb_step.argtypes = [vp, i32, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, u32]
    L.wsa_debug_stream_featdb_step.restype = ctypes.c_int
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


class KnnStore:
    """wsa_knn: the unit rows of an ml5 KNN classifier on the device (K9, spec KN-1).  Class indices are what the device sees;
    webspeechanalyzer_amd.knn maps labels to them."""

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

    def close(self):
        if self.h:
            self.L.wsa_knn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ensemble:
    """wsa_ensemble: the models of the app's `available_DBs`, in that order, classified and folded in one pass."""

    def __init__(self, an, models):
        self.an, self.L, self.models = an, an.L, list(models)
        arr = (ctypes.c_void_p * max(len(self.models), 1))(*[m.h if m is not None else None for m in self.models])
        self.h = ctypes.c_void_p()
        an._check(self.L.wsa_ensemble_create(an.h, ctypes.cast(arr, ctypes.c_void_p), len(self.models), ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.L.wsa_ensemble_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RegressGroup:
    """wsa_regress_group: 1 .. 8 regression Models with their output ranges, predicted in one grouped launch and folded by RG-1."""

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

    def close(self):
        if self.h:
            self.L.wsa_regress_group_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _GatherResult(ctypes.Structure):
    _fields_ = [("n_ranks", ctypes.c_uint32), ("n_rows", ctypes.c_uint32), ("rows_per_rank", ctypes.POINTER(ctypes.c_uint32)),
                ("d_row_meta", ctypes.c_void_p), ("d_row_feat", ctypes.c_void_p)]


class Gather:
    """wsa_gather: the feature rows of the batches of several contexts (one per GPU, this process) collected on the root's device
    with one grouped RCCL exchange (include/wsa.h)."""

    def __init__(self, analyzers, root=0):
        self.L = analyzers[0].L
        self.ans = list(analyzers)
        self.h = ctypes.c_void_p()
        arr = (ctypes.c_void_p * len(self.ans))(*[a.h for a in self.ans])
        st = self.L.wsa_gather_create(arr, len(self.ans), int(root), ctypes.byref(self.h))
        if st != 0:
            raise WsaError(f"wsa_gather_create failed ({st}): {self.L.wsa_last_error(self.ans[root].h).decode()}")
        self.root = root

    def rows(self, batches, streams=None):
        """-> (rows_per_rank, meta [n, 8] i32, feat [n, 53] f64) on the host, rank after rank"""
        n = len(self.ans)
        ba = (ctypes.c_void_p * n)(*[b.h for b in batches])
        sa = (ctypes.c_void_p * n)(*[int(s) for s in streams]) if streams is not None else None
        r = _GatherResult()
        self.ans[self.root]._check(self.L.wsa_gather_rows(self.h, ba, sa, ctypes.byref(r)))
        per = [int(r.rows_per_rank[i]) for i in range(n)]
        meta = np.zeros((r.n_rows, 8), np.int32)
        feat = np.zeros((r.n_rows, NFEAT), np.float64)
        self.ans[self.root]._check(self.L.wsa_gather_copy_rows(self.h, meta.ctypes.data, feat.ctypes.data, max(int(r.n_rows), 1)))
        return per, meta, feat

    def close(self):
        if self.h:
            self.L.wsa_gather_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ACTIVE, START, STOP = 1, 2, 4        # WSA_STREAM_* control bits


class Streams:
    """n concurrent launches advancing in lock step (wsa_stream): the reference's online path — one
    spectrum_push per frame with carried state, callbacks as segments close (dist/main.js:2 @B8752, @B28869)."""

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

    def set_input_format(self, fmt, channels=None):
        """The format of the samples the set is fed from now on (spec PK-1, wsa_stream_set_input_format): 'f32' (the default), 'i16', 'mulaw'
        or 'alaw' (or a PCM_* number); channels = interleaved channels per stream, one number or one per stream (1 .. 64, channel 0 is
        analysed).  Legal before the first step and between a collect() and the next step; the next step recaptures the graph."""
        f = pcm_format(fmt)
        ch = None
        if channels is not None:
            ch = np.ascontiguousarray(np.broadcast_to(np.asarray(channels, np.int64), (self.n,)) if np.ndim(channels) == 0 else channels, dtype=np.int64)
            if ch.shape != (self.n,):
                raise WsaError("channels as a sequence holds one count per stream")
            if ch.min() < 0 or ch.max() > 0xFFFFFFFF:
                raise WsaError(f"channel count {int(ch.min() if ch.min() < 0 else ch.max())} outside 1 .. 64")
            ch = ch.astype(np.uint32)
        self.an._check(self.L.wsa_stream_set_input_format(self.h, f, ch.ctypes.data if ch is not None else None))
        self.input_format = f
        self.channels = ch if ch is not None else np.ones(self.n, np.uint32)
        self.input_stride_bytes = int(self.L.wsa_stream_input_stride_bytes(self.h))

    def set_input_channels(self, fmt, channels=None, select=None, source=None):
        """set_input_format() with a select and a source per stream (spec PK-3, wsa_stream_set_input_channels): stream i takes channel select[i]
        ('mix': the mono mix; None: channel 0; one value for all is fine) of the packed row of stream source[i] (None: its own).  The host fills
        one row per source; counts and control bytes stay per stream."""
        f = pcm_format(fmt)
        ch = None
        if channels is not None:
            ch = np.ascontiguousarray(np.broadcast_to(np.asarray(channels, np.int64), (self.n,)) if np.ndim(channels) == 0 else channels, dtype=np.int64)
            if ch.shape != (self.n,):
                raise WsaError("channels as a sequence holds one count per stream")
            if ch.min() < 0 or ch.max() > 0xFFFFFFFF:
                raise WsaError(f"channel count {int(ch.min() if ch.min() < 0 else ch.max())} outside 1 .. 64")
            ch = ch.astype(np.uint32)
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

        def arr(ptr, ctype, dtype, shape):
            if not ptr:
                return None
            if not int(np.prod(shape)):
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=shape).copy()
        return dict(prob=arr(r.prob, ctypes.c_float, np.float32, (n, C)), cb=arr(r.cb, ctypes.c_int32, np.int32, (k, 4)),
                    cb_label=arr(r.cb_label, ctypes.c_int32, np.int32, (k,)), cb_conf=arr(r.cb_conf, ctypes.c_double, np.float64, (k,)),
                    stream_conf=arr(r.stream_conf, ctypes.c_double, np.float64, (int(r.n_streams), C)), labels=list(self._model.labels))

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

        def arr(ptr, ctype, dtype, shape):
            if not ptr:
                return None
            if not int(np.prod(shape)):
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=shape).copy()
        i32, f64 = (ctypes.c_int32, np.int32), (ctypes.c_double, np.float64)
        return dict(label=arr(r.label, *i32, (n,)), conf=arr(r.conf, *f64, (n, C)), nbr=arr(r.nbr, *i32, (n, k)), sim=arr(r.sim, ctypes.c_float, np.float32, (n, k)),
                    k_eff=int(r.k_eff), slices=int(r.slices), cb=arr(r.cb, *i32, (ncb, 4)), cb_label=arr(r.cb_label, *i32, (ncb,)),
                    cb_conf=arr(r.cb_conf, *f64, (ncb,)), stream_conf=arr(r.stream_conf, *f64, (int(r.n_streams), C)))

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

        def arr(ptr, ctype, dtype, shape):
            if not ptr:
                return None
            if not int(np.prod(shape)):
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=shape).copy()

        def per_head(ptrs, m):
            cols = [arr(ptrs[h], ctypes.c_double, np.float64, (m,)) for h in range(H)]
            return None if any(c is None for c in cols) else np.stack(cols) if cols else np.zeros((0, m))
        return dict(value=per_head(r.value, n), cb=arr(r.cb, ctypes.c_int32, np.int32, (k, 4)), cb_value=per_head(r.cb_value, k),
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
        kept = np.ctypeslib.as_array(ctypes.cast(r.kept, ctypes.POINTER(ctypes.c_int32)), shape=(na,)).copy() if na else np.zeros(0, np.int32)
        rep = None
        if r.replaced:
            rep = np.ctypeslib.as_array(ctypes.cast(r.replaced, ctypes.POINTER(ctypes.c_int32)), shape=(nr, 2)).copy() if nr else np.zeros((0, 2), np.int32)
        return dict(first_row=int(r.first_row), n_added=na, n_replaced=nr, not_fitted=int(r.not_fitted), kept=kept, replaced=rep)

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

        def arr(ptr, ctype, dtype, shape):
            if not int(np.prod(shape)):
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=shape).copy()
        out = dict(prob=[arr(r.prob[d], ctypes.c_float, np.float32, (n, C[d])) for d in range(nm)], labels=[list(m.labels) for m in self._ensemble.models])
        if not r.cb:
            return out
        i32, f64 = (ctypes.c_int32, np.int32), (ctypes.c_double, np.float64)
        out.update(cb_label=[arr(r.cb_label[d], *i32, (k,)) for d in range(nm)], cb_conf=[arr(r.cb_conf[d], *f64, (k,)) for d in range(nm)],
                   cb_all_max=[arr(r.cb_all_max[d], *f64, (k,)) for d in range(nm)],
                   stream_conf=[arr(r.stream_conf[d], *f64, (ns, C[d])) for d in range(nm)],
                   cb=arr(r.cb, *i32, (k, 4)), cb_db=arr(r.cb_db, *i32, (k,)), cb_top_label=arr(r.cb_top_label, *i32, (k,)),
                   cb_top_conf=arr(r.cb_top_conf, *f64, (k,)), cb_min_db=arr(r.cb_min_db, *i32, (k,)), cb_entropy=arr(r.cb_entropy, *f64, (k,)),
                   stream_min_db=arr(r.stream_min_db, *i32, (ns,)))
        return out

    def collect(self, stream=0):
        """Rows of the last step: dict(meta [n,8] i32, feat [n,53] f64, segments [m,4] i32) (copies)."""
        r = _StreamRows()
        self.an._check(self.L.wsa_stream_collect(self.h, stream, ctypes.byref(r)))
        n, m = r.n_rows, r.n_segments
        meta = np.ctypeslib.as_array(ctypes.cast(r.row_meta, ctypes.POINTER(ctypes.c_int32)), shape=(n, 8)).copy() if n else np.zeros((0, 8), np.int32)
        feat = np.ctypeslib.as_array(ctypes.cast(r.row_feat, ctypes.POINTER(ctypes.c_double)), shape=(n, NFEAT)).copy() if n else np.zeros((0, NFEAT))
        segs = np.ctypeslib.as_array(ctypes.cast(r.segments, ctypes.POINTER(ctypes.c_int32)), shape=(m, 4)).copy() if m else np.zeros((0, 4), np.int32)
        cuts = np.ctypeslib.as_array(ctypes.cast(r.stream_cuts, ctypes.POINTER(ctypes.c_uint32)), shape=(self.n,)).copy()
        out = dict(meta=meta, feat=feat, segments=segs, cuts=cuts, flags=int(r.status_flags))
        if r.utt_feat:                                  # level 11: one 264-vector per result of the step
            nu = int(r.n_utterance_rows)
            out["utt_meta"] = np.ctypeslib.as_array(ctypes.cast(r.utt_meta, ctypes.POINTER(ctypes.c_int32)), shape=(nu, 4)).copy() if nu else np.zeros((0, 4), np.int32)
            out["utt_feat"] = np.ctypeslib.as_array(ctypes.cast(r.utt_feat, ctypes.POINTER(ctypes.c_double)), shape=(nu, 264)).copy() if nu else np.zeros((0, 264))
        if r.track_off:                                 # level 3: ranked raw tracks of the step's segments (the layout of Batch.tracks())
            npt, nrk = int(r.n_track_points), int(r.n_track_ranked)
            out["track_off"] = np.ctypeslib.as_array(ctypes.cast(r.track_off, ctypes.POINTER(ctypes.c_uint64)), shape=(m + 1, 2)).copy()
            out["track_points"] = np.ctypeslib.as_array(ctypes.cast(r.track_points, ctypes.POINTER(ctypes.c_int32)), shape=(npt, 8)).copy() if npt else np.zeros((0, 8), np.int32)
            out["track_ranked"] = np.ctypeslib.as_array(ctypes.cast(r.track_ranked, ctypes.POINTER(ctypes.c_int32)), shape=(nrk,)).copy() if nrk else np.zeros((0,), np.int32)
            out["tracks"] = _track_records(out["track_off"], out["track_points"], out["track_ranked"], m)
        if r.formants and r.row_formant_off:           # levels 4 / 10: frames of row k = formants[formant_off[k]:formant_off[k + 1]]
            off = np.ctypeslib.as_array(ctypes.cast(r.row_formant_off, ctypes.POINTER(ctypes.c_uint32)), shape=(r.n_rows + 1,)).copy()
            out["formant_off"] = off
            out["formants"] = (np.ctypeslib.as_array(ctypes.cast(r.formants, ctypes.POINTER(ctypes.c_float)), shape=(int(off[-1]), 9)).copy()
                               if off[-1] else np.zeros((0, 9), np.float32))
        return out

    def close(self):
        if self.h:
            self.L.wsa_stream_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GATE_INT_RUNS, GATE_INT_GENERAL, GATE_F64, GATE_STREAM = 0, 1, 2, 3
GATE_STATE_WORDS = 16
GATE_SENTINEL = -2


def debug_regress_fold(meta, values, step_s, row_off, ctl=None, device=0, sentinel=-7.0):
    """Test access to the fold RG-1 on its own (csrc/debug_fold.hip wsa_debug_regress_fold; not part of include/wsa.h): hand-built row meta
    [n_rows, 8] i32 and value columns [H, n_rows] f64.  ctl None: a batch, row_off [n + 1]; else streams, row_off [n_steps, n + 1] counting
    from each step's first row and ctl [n_steps, n] control bytes.  Returns dict(n_cb (int, or [n_steps]), cb [K, 4], cb_value / cb_weight
    [H, K] over all K callbacks (the steps' one after the other), run_sum / run_weight / run_value [H, n] (streams: [n_steps, H, n]))."""
    L = lib()
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
    L.wsa_debug_regress_fold.argtypes = [i32, vp, vp, u32, u32, ctypes.c_double, u32, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
    L.wsa_debug_regress_fold.restype = ctypes.c_int
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
    L.wsa_debug_class_fold.argtypes = [ctypes.c_int32, ctypes.c_void_p]
    L.wsa_debug_class_fold.restype = ctypes.c_int
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
    L.wsa_debug_classify.argtypes = [ctypes.c_void_p]
    L.wsa_debug_classify.restype = ctypes.c_int
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
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.wsa_debug_knn_split.argtypes = [vp, vp, u32, u32, u32, vp, vp, vp, vp, vp]
    L.wsa_debug_knn_split.restype = ctypes.c_int
    store.an._check(L.wsa_debug_knn_split(store.h, d_feat, int(n_rows), int(k), int(slices), d_label, d_conf, d_nbr, d_sim, stream))


def debug_gate(variant, clips, settings, blocks=0, F=0, max_span=0, step_nfr=None, step_ctl=None, device=0):
    """Test access to the gate on its own (csrc/debug_gate.hip wsa_debug_gate; not part of include/wsa.h): clips = [frames_c, bands] u32 arrays, settings =
    the six gate settings by name, variant = GATE_*.  Streams (GATE_STREAM): step_nfr / step_ctl [n_steps, n_clips].  Returns the gate's outputs as the
    kernel left them: fr_info / fr_v / fr_fl (fr_span) per clip, seg_i [.., seg_cap, 8], seg_d [.., seg_cap, 2], seg_count, flags, counter0, seg_cap (ring,
    state per step); frames no step fed keep GATE_SENTINEL.  Raises WsaError on a refusal."""
    L = lib()
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    L.wsa_debug_gate.argtypes = [i32, i32, vp, vp, u32, i32, vp, u32, u32, u32, u32, vp, vp, vp] + [vp] * 9
    L.wsa_debug_gate.restype = ctypes.c_int
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
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    L.wsa_debug_peaks.argtypes = [i32, vp, u32, i32, i32, vp, vp, vp, vp]
    L.wsa_debug_peaks.restype = ctypes.c_int
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
    vp, i32, u32, u64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    L.wsa_debug_resample.argtypes = [i32, vp, u32, u64, u32, u32, vp, vp, dbl, i32, i32, i32, i32, vp, u64, vp, vp, u32, vp]
    L.wsa_debug_resample.restype = ctypes.c_int
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
    L.wsa_debug_fe_choice.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_char_p, ctypes.c_uint32]
    L.wsa_debug_fe_choice.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(64)
    rc = L.wsa_debug_fe_choice(analyzer.h, float(fs), buf, 64)
    if rc != 0:
        raise WsaError(f"wsa_debug_fe_choice: error {rc}")
    return buf.value.decode()


def debug_stream_spectra(streams, bands):
    """Test access (csrc/debug.hip wsa_debug_stream_spectra): the u32 frames the front end wrote in the stream set's last step,
    [n_streams, frames_per_step, bands]; call behind collect()."""
    L = lib()
    L.wsa_debug_stream_spectra.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.wsa_debug_stream_spectra.restype = ctypes.c_int
    out = np.zeros((streams.n, streams.frame_capacity, int(bands)), np.uint32)
    rc = L.wsa_debug_stream_spectra(streams.h, out.ctypes.data, out.size)
    if rc != 0:
        raise WsaError(f"wsa_debug_stream_spectra: error {rc}")
    return out


def debug_stream_ctl(streams):
    """Test access (csrc/debug.hip wsa_debug_stream_ctl; not part of include/wsa.h): the device control words of a plain stream set's last step,
    [3, n_streams] uint32 = nfr, off (samples), bits (1 START, 2 STOP, 4 active); call behind collect().  A mixed-rate set is refused."""
    L = lib()
    L.wsa_debug_stream_ctl.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    L.wsa_debug_stream_ctl.restype = ctypes.c_int
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
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    L.wsa_debug_stream_step_backend.argtypes = [vp, vp, vp, vp, u32, vp]
    L.wsa_debug_stream_step_backend.restype = ctypes.c_int
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
    L.wsa_debug_compact.argtypes = [ctypes.c_int32, ctypes.c_void_p]
    L.wsa_debug_compact.restype = ctypes.c_int
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
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    L.wsa_debug_span_order.argtypes = [i32, i32, vp, vp, u32, i32, vp, u32, vp] + [vp] * 6
    L.wsa_debug_span_order.restype = ctypes.c_int
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
