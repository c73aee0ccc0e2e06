"""The boundary itself: the structures and constants of include/wsa.h, the signature of every function it declares, and the loader."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # the package webspeechanalyzer_amd: lib/ and csrc/ live there
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


ABI_VERSION = 5            # WSA_ABI_VERSION of include/wsa.h this binding's structures follow
CHANNEL_MIX = 0xFFFFFFFF                                # WSA_CHANNEL_MIX: the `select` word that takes the mono mix (spec PK-3); 'mix' in the Python entries
PCM_F32, PCM_I16, PCM_MULAW, PCM_ALAW = 0, 1, 2, 3      # WSA_PCM_* of include/wsa.h
PCM_U8, PCM_I24, PCM_I32, PCM_F64 = 8, 9, 10, 11        # ... the file encodings of spec PK-2 (batches and pcm_decode; 4 .. 7 are unassigned)
_PCM_NAMES = {"f32": PCM_F32, "i16": PCM_I16, "mulaw": PCM_MULAW, "alaw": PCM_ALAW, "u8": PCM_U8, "i24": PCM_I24, "i32": PCM_I32, "f64": PCM_F64}
_PCM_DTYPE = {PCM_F32: np.float32, PCM_I16: np.int16, PCM_MULAW: np.uint8, PCM_ALAW: np.uint8,
              PCM_U8: np.uint8, PCM_I24: np.uint8, PCM_I32: np.int32, PCM_F64: np.float64}
_PCM_ELEMS = {PCM_I24: 3}                               # array elements per sample ('i24': three uint8)
TRAIN_GROUP_MAX = 32       # WSA_TRAIN_GROUP_MAX of include/wsa.h

P, st = ctypes.POINTER, ctypes.c_int                    # st: wsa_status (and int)
vp, i32, u32, u64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
# name: (restype, argtypes) of every function include/wsa.h declares, and of nothing else (tests/test_abi.py compares both ways, kind by kind);
# lib() declares them all at load.  A result that is no int must be named here: ctypes cuts a 64-bit or pointer result left at c_int.
ABI_TABLE = {
    "wsa_config_default": (None, [P(_Config)]),
    "wsa_abi_version": (st, []),
    "wsa_create": (st, [P(_Config), i32, P(vp)]),
    "wsa_destroy": (None, [vp]),
    "wsa_last_error": (ctypes.c_char_p, [vp]),
    "wsa_geometry_for": (st, [vp, dbl, P(_Geometry)]),
    "wsa_bins_hz": (st, [vp, dbl, vp, i32]),
    "wsa_batch_create": (st, [vp, u32, vp, dbl, P(vp)]),
    "wsa_batch_destroy": (None, [vp]),
    "wsa_batch_run": (st, [vp, vp, u64, vp]),
    "wsa_batch_run_host": (st, [vp, vp, vp]),
    "wsa_batch_result": (st, [vp, vp, P(_DeviceResult)]),
    "wsa_batch_copy_rows": (st, [vp, vp, vp, vp, u32, vp, u32, vp, vp]),
    "wsa_batch_copy_spectra": (st, [vp, vp, vp, u64, vp]),
    "wsa_batch_get_info": (st, [vp, P(_BatchInfo)]),
    "wsa_batch_stage_ms": (st, [vp, vp]),
    "wsa_batch_enable_timing": (st, [vp, i32]),
    "wsa_batch_run_frontend": (st, [vp, vp, u64, vp]),
    "wsa_batch_run_backend": (st, [vp, vp, vp]),
    "wsa_batch_enable_trace": (st, [vp, i32]),
    "wsa_batch_copy_trace": (st, [vp, vp, vp, u64]),
    "wsa_batch_copy_formants": (st, [vp, vp, vp, u64]),
    "wsa_batch_copy_utterance": (st, [vp, vp, vp, vp, u32, vp]),
    "wsa_batch_tracks_info": (st, [vp, vp, vp]),
    "wsa_batch_copy_tracks": (st, [vp, vp, vp, vp, u64, vp, u64]),
    "wsa_batch_create_resampled": (st, [vp, u32, vp, dbl, dbl, P(vp)]),
    "wsa_resample_length": (u64, [u64, dbl, dbl]),
    "wsa_batch_copy_pcm": (st, [vp, vp, vp, u64]),
    "wsa_batch_create_mixed": (st, [vp, u32, vp, vp, dbl, P(vp)]),
    "wsa_stream_create": (st, [vp, u32, dbl, u32, u32, P(vp)]),
    "wsa_stream_destroy": (None, [vp]),
    "wsa_stream_samples_per_step": (u32, [vp]),
    "wsa_stream_step": (st, [vp, vp, u64, vp, vp]),
    "wsa_stream_host_input": (P(ctypes.c_float), [vp]),
    "wsa_stream_step_host": (st, [vp, vp, vp]),
    "wsa_stream_collect": (st, [vp, vp, P(_StreamRows)]),
    "wsa_stream_enable_graph": (st, [vp, i32]),
    "wsa_batch_keep_spectra": (st, [vp, i32]),
    "wsa_batch_backend_reruns": (st, [vp, vp]),
    "wsa_stream_time_steps": (st, [vp, u32, vp, u32, vp, vp, vp]),
    "wsa_batch_run_host_i16": (st, [vp, vp, vp, vp]),
    "wsa_gather_create": (st, [vp, i32, i32, vp]),
    "wsa_gather_destroy": (None, [vp]),
    "wsa_gather_rows": (st, [vp, vp, vp, vp]),
    "wsa_gather_copy_rows": (st, [vp, vp, vp, u32]),
    "wsa_host_alloc": (st, [vp, u64, P(vp)]),
    "wsa_host_free": (None, [vp]),
    "wsa_queue_create": (st, [vp, P(vp)]),
    "wsa_queue_destroy": (None, [vp, vp]),
    # additions within version 5 (probe for wsa_model_create): the app's syllable classifier
    "wsa_model_create": (st, [vp, P(_ModelDesc), P(vp)]),
    "wsa_model_destroy": (None, [vp]),
    "wsa_classify_rows": (st, [vp, vp, u32, vp, vp]),
    "wsa_batch_classify": (st, [vp, vp, vp]),
    "wsa_batch_class_result": (st, [vp, vp, P(_ClassResult)]),
    "wsa_batch_copy_classes": (st, [vp, vp, vp, u32, vp, vp, vp, u32, vp]),
    # additions within version 5 (probe for wsa_stream_set_model): the classifier inside the stream step
    "wsa_stream_set_model": (st, [vp, vp]),
    "wsa_stream_classes": (st, [vp, P(_StreamClassResult)]),
    # additions within version 5 (probe for wsa_ensemble_create): every model DB of the app in one pass
    "wsa_ensemble_create": (st, [vp, vp, u32, P(vp)]),
    "wsa_ensemble_destroy": (None, [vp]),
    "wsa_batch_classify_ensemble": (st, [vp, vp, vp]),
    "wsa_batch_ensemble_result": (st, [vp, vp, P(_EnsembleResult)]),
    "wsa_batch_copy_ensemble": (st, [vp, vp, P(_EnsembleHost)]),
    "wsa_stream_set_ensemble": (st, [vp, vp]),
    "wsa_stream_ensemble_classes": (st, [vp, P(_StreamEnsembleResult)]),
    # additions within version 5 (probe for wsa_stream_create_mixed): streams of different rates, converted inside the step
    "wsa_stream_create_mixed": (st, [vp, u32, vp, dbl, u32, u32, P(vp)]),
    "wsa_stream_input_capacity": (u32, [vp, u32]),
    "wsa_stream_input_stride": (u32, [vp]),
    "wsa_stream_paced_input": (u32, [vp, u32]),
    "wsa_stream_step_frame_capacity": (u32, [vp]),
    "wsa_stream_step_n": (st, [vp, vp, u64, vp, vp, vp]),
    "wsa_stream_step_host_n": (st, [vp, vp, vp, vp]),
    "wsa_resample_ready": (u64, [u64, dbl, dbl]),
    "wsa_stream_frames_bound": (u32, [u32, u32, dbl]),
    "wsa_stream_copy_converted": (st, [vp, vp, u32, vp]),
    # additions within version 5 (probe for wsa_trainer_create): training the app's classifiers (K7, spec TR-1)
    "wsa_trainer_create": (st, [vp, P(_ModelDesc), vp, vp, u32, u32, u32, dbl, P(vp)]),
    "wsa_trainer_destroy": (None, [vp]),
    "wsa_trainer_epoch": (st, [vp, vp, vp]),
    "wsa_trainer_stats": (st, [vp, vp, P(_TrainStats)]),
    "wsa_trainer_copy_weights": (st, [vp, vp, vp, vp]),
    "wsa_trainer_model": (st, [vp, vp, P(vp)]),
    # additions within version 5 (probe for wsa_regress_trainer_create): the app's regression models (ords_*, spec TR-2)
    "wsa_regress_rows": (st, [vp, dbl, dbl, vp, u32, vp, vp]),
    "wsa_batch_regress": (st, [vp, vp, dbl, dbl, vp]),
    "wsa_batch_copy_values": (st, [vp, vp, vp, u32, P(u32)]),
    "wsa_regress_trainer_create": (st, [vp, P(_ModelDesc), vp, vp, u32, u32, u32, dbl, dbl, dbl, P(vp)]),
    "wsa_queue_synchronize": (st, [vp, vp]),
    # additions within version 5 (probe for wsa_dbstats_create): predicting a labelled feature DB and the app's results table (K8, spec DS-1)
    "wsa_dbstats_create": (st, [vp, vp, vp, u32, u32, vp, u32, P(vp)]),
    "wsa_dbstats_destroy": (None, [vp]),
    "wsa_dbstats_set_classes": (st, [vp, u32, vp, vp]),
    "wsa_dbstats_set_values": (st, [vp, u32, vp, vp]),
    "wsa_dbstats_predict_classes": (st, [vp, u32, vp, vp, vp]),
    "wsa_dbstats_decide_rows": (st, [vp, u32, vp, u32, vp, vp]),
    "wsa_dbstats_predict_values": (st, [vp, u32, vp, dbl, dbl, vp]),
    "wsa_dbstats_table": (st, [vp, vp, vp, vp, vp]),
    "wsa_dbstats_copy_classes": (st, [vp, u32, vp, vp]),
    "wsa_dbstats_copy_values": (st, [vp, u32, vp, vp]),
    "wsa_dbstats_copy_probs": (st, [vp, vp, vp, u32]),
    # additions within version 5 (probe for wsa_level_feature_count): models, training and DBs at the row widths of levels 11 and 12
    "wsa_level_feature_count": (i32, [i32]),
    "wsa_wide_dbstats_create": (st, [vp, vp, u32, vp, u32, u32, vp, u32, P(vp)]),
    # additions within version 5 (probe for wsa_knn_create): the app's ml5 KNN classifier (K9, spec KN-1)
    "wsa_knn_create": (st, [vp, i32, i32, u32, P(vp)]),
    "wsa_knn_destroy": (None, [vp]),
    "wsa_knn_add": (st, [vp, vp, vp, u32, vp]),
    "wsa_knn_count": (st, [vp, vp, P(u32), vp]),
    "wsa_knn_classify_rows": (st, [vp, vp, u32, u32, vp, vp, vp, vp, vp]),
    "wsa_knn_tile_info": (st, [P(i32), P(i32)]),
    "wsa_batch_knn": (st, [vp, vp, u32, vp]),
    "wsa_batch_knn_result": (st, [vp, vp, P(_KnnResult)]),
    "wsa_batch_copy_knn": (st, [vp, vp, vp, vp, vp, vp, u32]),
    # additions within version 5 (probe for wsa_stream_set_knn): KNN on live streams (K9s) and the fold of KNN results (spec KN-2)
    "wsa_batch_knn_fold": (st, [vp, vp]),
    "wsa_batch_knn_fold_result": (st, [vp, vp, P(_KnnFoldResult)]),
    "wsa_batch_copy_knn_fold": (st, [vp, vp, vp, vp, vp, u32, vp]),
    "wsa_stream_set_knn": (st, [vp, vp, u32]),
    "wsa_stream_knn_classes": (st, [vp, P(_StreamKnnResult)]),
    # additions within version 5 (probe for wsa_regress_group_create): V, A, D per callback in batches and streams (spec RG-1)
    "wsa_regress_group_create": (st, [vp, vp, vp, vp, u32, P(vp)]),
    "wsa_regress_group_destroy": (None, [vp]),
    "wsa_regress_group_rows": (st, [vp, vp, u32, vp, vp]),
    "wsa_batch_regress_group": (st, [vp, vp, vp]),
    "wsa_batch_value_result": (st, [vp, vp, P(_ValueResult)]),
    "wsa_batch_copy_value_fold": (st, [vp, vp, P(_ValueHost)]),
    "wsa_stream_set_regress": (st, [vp, vp]),
    "wsa_stream_values": (st, [vp, P(_StreamValueResult)]),
    # additions within version 5 (probe for wsa_train_group_create): a group of trainers in one pass of grouped launches (K7g, spec TG-1)
    "wsa_train_group_create": (st, [vp, vp, u32, P(vp)]),
    "wsa_train_group_destroy": (None, [vp]),
    "wsa_train_group_epoch": (st, [vp, vp, vp]),
    "wsa_train_group_stats": (st, [vp, vp, vp]),
    "wsa_train_group_launches": (st, [vp, P(u32)]),
    "wsa_train_group_launch_count": (st, [vp, vp, vp, vp, u32, P(u64)]),
    # additions within version 5 (probe for wsa_stream_set_input_format): 16-bit and G.711 PCM into streams, unpacked in the step (spec PK-1)
    "wsa_stream_set_input_format": (st, [vp, i32, vp]),
    "wsa_stream_host_input_packed": (vp, [vp]),
    "wsa_stream_input_stride_bytes": (u32, [vp]),
    "wsa_stream_step_packed": (st, [vp, vp, u64, vp, vp, vp]),
    "wsa_stream_time_steps_packed": (st, [vp, u32, vp, u32, vp, vp, vp]),
    "wsa_pcm_decode": (st, [i32, vp, u64, u32, vp]),
    # additions within version 5 (probe for wsa_batch_run_host_packed): every PCM encoding a WAV holds into batches, unpacked on the GPU (spec PK-2)
    "wsa_batch_run_host_packed": (st, [vp, vp, vp, vp, vp]),
    "wsa_batch_set_input_format": (st, [vp, vp, vp]),
    "wsa_batch_packed_offset": (u64, [vp, u32]),
    "wsa_batch_run_packed": (st, [vp, vp, vp]),
    # additions within version 5 (probe for wsa_batch_set_input_channels): any channel, every channel or the mono mix of interleaved PCM (spec PK-3)
    "wsa_pcm_decode_select": (st, [i32, vp, u64, u32, u32, vp]),
    "wsa_batch_set_input_channels": (st, [vp, vp, vp, vp, vp]),
    "wsa_batch_run_host_channels": (st, [vp, vp, vp, vp, vp, vp, vp]),
    "wsa_stream_set_input_channels": (st, [vp, i32, vp, vp, vp]),
    "wsa_pcm_channels_tile_frames": (u32, [i32, u32]),
    # additions within version 5 (probe for wsa_featdb_create): the feature DB that stays on the device (K10, spec FD-1)
    "wsa_featdb_create": (st, [vp, i32, u32, P(vp)]),
    "wsa_featdb_destroy": (None, [vp]),
    "wsa_featdb_clear": (st, [vp]),
    "wsa_featdb_count": (st, [vp, P(u32)]),
    "wsa_featdb_append_batch": (st, [vp, vp, vp, P(u32), P(u32), vp, u32]),
    "wsa_featdb_append_host": (st, [vp, vp, u32, vp]),
    "wsa_featdb_device_rows": (st, [vp, P(vp)]),
    "wsa_featdb_copy_rows": (st, [vp, vp, u32, u32, vp]),
    "wsa_featdb_gather": (st, [vp, vp, u32, vp, vp]),
    "wsa_featdb_ranges": (st, [vp, vp, u32, vp, vp, vp]),
    "wsa_featdb_tile_info": (st, [P(i32), P(i32), P(i32)]),
    "wsa_trainer_create_db": (st, [vp, P(_ModelDesc), vp, vp, vp, u32, u32, u32, dbl, P(vp)]),
    "wsa_regress_trainer_create_db": (st, [vp, P(_ModelDesc), vp, vp, vp, u32, u32, u32, dbl, dbl, dbl, P(vp)]),
    "wsa_featdb_dbstats_create": (st, [vp, vp, u32, u32, vp, u32, vp, u32, P(vp)]),
    # additions within version 5 (probe for wsa_stream_set_featdb): live streams collect into the device DB, inside the step (spec FD-2)
    "wsa_stream_set_featdb": (st, [vp, vp]),
    "wsa_stream_db_rows": (st, [vp, P(_StreamDbResult)]),
    "wsa_stream_featdb_tile_info": (st, [P(i32)] * 4),
}
ABI_SYMBOLS = list(ABI_TABLE)
# the same for include/wsa_eval.h (additions within version 5, probe for wsa_dbstats_confusion): evaluating a labelled DB (K8e, spec EV-1).
# A table of its own because the header is: tests/test_abi.py pins what wsa.h declares, tests/test_dbeval_host.py holds this one to its header.
EVAL_TABLE = {
    "wsa_dbstats_confusion": (st, [vp, u32, vp, vp]),
    "wsa_dbstats_agreement": (st, [vp, vp, vp]),
    "wsa_dbstats_set_files": (st, [vp, vp, vp, u32]),
    "wsa_dbstats_set_file_classes": (st, [vp, u32, vp]),
    "wsa_dbstats_set_file_values": (st, [vp, u32, vp]),
    "wsa_dbstats_fold_files": (st, [vp, u32, vp]),
    "wsa_dbstats_fold_file_values": (st, [vp, u32, vp]),
    "wsa_dbstats_file_table": (st, [vp, vp, vp, vp, vp]),
    "wsa_dbstats_file_confusion": (st, [vp, u32, vp, vp]),
    "wsa_dbstats_file_agreement": (st, [vp, vp, vp]),
    "wsa_dbstats_copy_file_sums": (st, [vp, u32, vp, vp, u32]),
    "wsa_dbstats_copy_file_classes": (st, [vp, u32, vp, vp]),
    "wsa_dbstats_copy_file_values": (st, [vp, u32, vp, vp]),
}
EVAL_SYMBOLS = list(EVAL_TABLE)
# the same for include/wsa_crossval.h (additions within version 5, probe for wsa_dbstats_set_folds): held-out prediction (K6f, spec CV-1);
# tests/test_crossval_host.py holds this one to its header
CROSSVAL_MAX_FOLDS = 32    # WSA_CROSSVAL_MAX_FOLDS (= WSA_TRAIN_GROUP_MAX)
CROSSVAL_TABLE = {
    "wsa_dbstats_set_folds": (st, [vp, vp, u32]),
    "wsa_dbstats_predict_classes_folds": (st, [vp, u32, vp, u32, vp, vp]),
    "wsa_dbstats_predict_values_folds": (st, [vp, u32, vp, u32, vp, vp, vp]),
    "wsa_crossval_tiles": (st, [vp, vp, u32, vp]),
}
CROSSVAL_SYMBOLS = list(CROSSVAL_TABLE)

_LIB = None


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
    L.wsa_abi_version.restype = ctypes.c_int
    if L.wsa_abi_version() != ABI_VERSION:
        raise WsaError(f"{path} has ABI version {L.wsa_abi_version()}, this binding is written against {ABI_VERSION} (include/wsa.h): rebuild the library")
    for name, (restype, argtypes) in list(ABI_TABLE.items()) + list(EVAL_TABLE.items()) + list(CROSSVAL_TABLE.items()):
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    from .debug import DEBUG_TABLE
    for name, (restype, argtypes) in DEBUG_TABLE.items():
        if hasattr(L, name):             # a test entry another build (WSA_LIB_DIR) lacks fails where it is called, as it always did
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _LIB = L
    return L
