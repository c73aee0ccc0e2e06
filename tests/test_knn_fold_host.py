"""CPU-side checks of the KNN stream / fold additions: the library exports the new symbols, and the Python host maps the class indices
of fold results back to ml5's labels — also when a number label sorts in front of the classes already stored —, and the Node host's
setPredictionKnn refuses bad arguments before it touches a device."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from webspeechanalyzer_amd import capi, knn

NEW_SYMBOLS = ["wsa_stream_set_knn", "wsa_stream_knn_classes", "wsa_batch_knn_fold", "wsa_batch_knn_fold_result", "wsa_batch_copy_knn_fold",
               "wsa_debug_knn_split"]


def test_library_exports_the_new_symbols():
    capi.build_library()
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert set(NEW_SYMBOLS[:-1]) <= set(capi.ABI_SYMBOLS) and "wsa_debug_knn_split" not in capi.ABI_SYMBOLS     # test access is not ABI


def test_fold_results_are_named_in_ml5s_class_order():
    # 10 arrives first, then 7, 2 and "b": numbers are their own class ids and are scanned ascending, the string (ml5 numbers it 0 by first
    # appearance, an id of its own here) ... so the device's class 0 is not the first label seen
    classes, index = knn.label_order([10, 7, 2, 10, 3])
    assert classes == ["2", "3", "7", "10"] and index.tolist() == [3, 2, 0, 3, 1]
    raw = dict(label=np.array([3, 0, -1], np.int32), conf=np.arange(3 * 64, dtype=np.float64).reshape(3, 64), k_eff=10,
               cb=np.zeros((4, 4), np.int32), cb_label=np.array([0, 3, -1, -2], np.int32), cb_conf=np.ones(4), stream_conf=np.ones((2, 64)))
    got = knn.name_results(classes, raw)
    assert got["label"] == ["10", "2", None] and got["index"] is raw["label"]
    assert got["cb_label"] == ["2", "10", None, None] and got["cb_index"].tolist() == [0, 3, -1, -2]
    assert got["conf"].shape == (3, 4) and got["stream_conf"].shape == (2, 4) and got["classes"] == classes and got["k_eff"] == 10
    # level 5: no fold tables
    got = knn.name_results(classes, dict(label=np.array([1], np.int32), conf=np.zeros((1, 64)), cb=None, cb_label=None, cb_conf=None, stream_conf=None))
    assert got["label"] == ["3"] and got["cb_label"] is None and got["stream_conf"] is None and "cb_index" not in got


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_set_prediction_knn_refuses_bad_arguments_without_a_device():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "js", "knn_refusals.js")
    r = subprocess.run([shutil.which("node"), script], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert "knn is a KNNClassifier" in got["not_a_classifier"]
    assert "rows of 264 features" in got["wide"] and "53-feature syllable rows of output_level 13" in got["wide"]
    assert got["k0"].endswith("k must be 1 .. 64, got 0") and got["k65"].endswith("got 65") and got["k_missing"].endswith("got undefined")
    assert "no example" in got["empty"] and "released" in got["released"]
    assert got["no_callback"] == "setPredictionKnn(knn | null, k, on_prediction)"
    assert got["fine"] is None and got["detach"] is None
